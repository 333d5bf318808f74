"""The host side of gc_yao_* (circuit.Garbler / circuit.Evaluator for S sessions per call) without a GPU: the layout against
the Python restatement (tests/py_yao_reference.py), what the geometry refuses, the skeleton and the piece table of M1 walked by
tests/cpp/yao_host_check.cpp (compiled from the engine's own mpc_amd/csrc/yao_skel.h), and the M3 arithmetic of
mpc_amd/csrc/yao_m3.h against Python's int.to_bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mpc_amd import engine
from mpc_amd.circuit import synthetic_levelised
from tests import py_yao_reference as ref
from tests import sha2pc_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_amd", "csrc")


def plan_of(c):
    return engine.Plan(c.Gates, c.NumWires, c.num_inputs, c.num_outputs)


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("yao_host_check")
    exe = d / "yao_host_check"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "yao_host_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return d, str(exe)


def test_layout_equals_the_restatement(aes_circ):
    small, _ = sha2pc_cases.small_circuit(3, 9)
    for circ, ng, ne in ((aes_circ, 128, 128), (small, 3, 9), (small, 0, 12)):
        for keylen in (16, 24, 32):
            g = ref.geometry(circ, ng, ne, keylen)
            assert engine.yao_layout(plan_of(circ), ng, ne, keylen) == [ref.len1(g), ref.len2(g), ref.slot3(g)]
    g = ref.geometry(aes_circ, 128, 128, 32)
    assert ref.len1(g) == 4 + 32 + (4 + 4 * aes_circ.NumGates + 16 * aes_circ.slab_rows()) + 16 * 128
    assert (ref.len2(g), ref.slot3(g)) == (2048, 20)


def test_geometry_refuses_what_create_refuses():
    small, _ = sha2pc_cases.small_circuit(3, 9)
    p = plan_of(small)
    for keylen in (0, 8, 20, 33):
        with pytest.raises(engine.EngineError) as e:
            engine.yao_layout(p, 3, 9, keylen)
        assert e.value.code == engine.GC_E_KEYSIZE
    for ng, ne, text in ((3, 8, b"input count"), (4, 9, b"input count"), (12, 0, b"without evaluator inputs")):
        with pytest.raises(engine.EngineError) as e:
            engine.yao_layout(p, ng, ne, 32)
        assert e.value.code == engine.GC_E_ARG and text in engine.lib().gc_last_error()
    with pytest.raises(engine.EngineError) as e:
        engine.yao_layout(None, 3, 9, 32)
    assert e.value.code == engine.GC_E_ARG
    # a handle needs a ctx and a circuit
    L, st = engine.lib(), C.c_int(0)
    assert not L.gc_yao_garbler_create(None, None, 3, 9, 32, 2, C.byref(st)) and st.value == engine.GC_E_ARG
    assert not L.gc_yao_evaluator_create(None, None, 3, 9, 32, 2, C.byref(st)) and st.value == engine.GC_E_ARG
    assert L.gc_yao_garbler_batch(None) is None and L.gc_yao_evaluator_batch(None) is None
    L.gc_yao_garbler_free(None)
    L.gc_yao_evaluator_free(None)
    tile, piece = engine.yao_kernel_shape()
    assert tile in (4, 8, 16, 32, 64) and piece % 16 == 0 and 64 <= piece <= 16384


def walk(host_check, circ, ng, keylen, piece):
    d, exe = host_check
    f = d / "rows.bin"
    np.ascontiguousarray(plan_of(circ).row_of_gate, "<u4").tofile(str(f))
    r = subprocess.run([exe, "pieces", str(keylen), str(ng), str(piece), str(f)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-400:] + r.stderr
    lines = r.stdout.splitlines()
    geom = tuple(int(v) for v in lines[0].split()[1:])
    pieces = [tuple(int(v) for v in l.split()[1:]) for l in lines if l.startswith("piece ")]
    cover = tuple(int(v) for v in [l for l in lines if l.startswith("cover ")][0].split()[1:])
    skel = bytes.fromhex([l for l in lines if l.startswith("skel ")][0].split()[1])
    return geom, pieces, cover, skel


def check_walk(host_check, circ, ng, keylen, piece):
    """-> rows across a piece boundary"""
    g = ref.geometry(circ, ng, circ.num_inputs - ng, keylen)
    geom, pieces, cover, skel = walk(host_check, circ, ng, keylen, piece)
    npieces = -(-ref.len1(g) // piece)
    at_tables = 4 + keylen
    at_labels = at_tables + ref.tables_bytes(g)
    assert geom == (ref.len1(g), at_tables, at_labels, npieces, piece)
    # every byte of the table section behind the gate count exactly once, nothing outside it
    mn, mx, across, outside = cover
    assert (mn, mx, outside) == (1, 1, 0)
    # each piece starts at the right gate and row: the first gate whose row word is at or behind its first byte, the first
    # row with a byte at or behind it
    goff = ref.gate_offsets(g)
    roff = [o + 4 + 16 * r for o, n in zip(goff, g.rows) for r in range(n)]
    assert len(pieces) == npieces
    want_across = 0
    for p, lo, hi, gate, row in pieces:
        assert (lo, hi) == (p * piece, min((p + 1) * piece, ref.len1(g)))
        assert gate == sum(1 for o in goff if o < lo) and row == sum(1 for o in roff if o + 16 <= lo)
        want_across += sum(1 for o in roff if o < hi < o + 16)
    assert across == want_across
    # the skeleton is M1 of an all-zero key, slab and labels
    zero = lambda key, rnd: (np.zeros(g.ng + g.ne, engine.WIRE), np.zeros(g.nout, engine.WIRE), np.zeros(sum(g.rows), engine.LABEL))
    m1, _ = ref.garbler_send(g, bytes(keylen), b"", [0] * ng, zero)
    assert skel == m1
    return across


def test_piece_table_of_the_small_circuit_with_a_row_across_a_boundary(host_check):
    small, _ = sha2pc_cases.small_circuit(3, 9)
    across = [check_walk(host_check, small, 3, keylen, piece) for keylen in (16, 24, 32) for piece in (64, 80, 256, 4096)]
    assert max(across) > 0  # a row lies across a piece boundary in some of them ...
    assert check_walk(host_check, small, 3, 32, 64) > 0  # ... and in this one


def test_piece_table_of_aes_128_at_the_kernels_piece_size(host_check, aes_circ):
    _, piece = engine.yao_kernel_shape()
    assert check_walk(host_check, aes_circ, 128, 32, piece) > 0
    check_walk(host_check, aes_circ, 0, 16, piece)


def test_piece_table_of_a_circuit_with_every_op(host_check):
    c = synthetic_levelised(9, 33, 0.3, seed=11, ninputs=24, or_frac=0.1, inv_frac=0.15, xnor_frac=0.1)
    for piece in (64, 112, 1024):
        check_walk(host_check, c, 5, 24, piece)


NOUTS = (1, 7, 8, 9, 11, 64, 65)


def results(nout):
    return sorted({0, 1, 1 << (nout - 1), (1 << nout) - 1})


def test_m3_pack_and_parse_against_int_to_bytes(host_check):
    _, exe = host_check
    hx = lambda b: b.hex() if b else "-"
    lines, want = [], []
    for nout in NOUTS:
        nb8 = (nout + 7) // 8
        for v in results(nout):
            data = v.to_bytes((v.bit_length() + 7) // 8, "big")  # result.Bytes()
            msg = len(data).to_bytes(4, "big") + data
            bits = v.to_bytes(nb8, "little")
            lines.append("pack %d %s" % (nout, hx(bits)))
            want.append("%d %s" % (len(msg), hx(msg)))
            lines.append("parse %d %d %s" % (nout, 4 + nb8, hx(msg)))
            want.append("1 %s" % hx(bits))
            # leading zero bytes and bits at index nout and above: SetBytes takes them, IO.Split drops them
            long = (v | 1 << nout | 1 << (8 * nb8 + 3)).to_bytes(nb8 + 2, "big")
            lines.append("parse %d %d %s" % (nout, 4 + nb8 + 2, hx((nb8 + 2).to_bytes(4, "big") + long)))
            want.append("1 %s" % hx(bits))
            # n too long for the room
            lines.append("parse %d %d %s" % (nout, 4 + nb8, hx((nb8 + 1).to_bytes(4, "big") + bytes(nb8))))
            want.append("0 -")
        assert ref.pack_result(None, (1 << (nout - 1)).to_bytes(nb8, "little"))[:4] == nb8.to_bytes(4, "big")
    r = subprocess.run([exe, "m3"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for l, g_, w in zip(lines, got, want):
        assert g_ == w, (l, g_, w)


def test_the_restatement_packs_as_the_header_does():
    for nout in NOUTS:
        g = ref.Geometry(0, 1, nout, 32, ())
        for v in results(nout):
            bits = v.to_bytes(ref.bits_bytes(g), "little")
            m3 = ref.pack_result(g, bits)
            assert ref.evaluator_result(g, m3 + bytes(ref.slot3(g) - len(m3)), ref.slot3(g)) == (bits, 0)
        assert ref.evaluator_result(g, (ref.slot3(g) - 3).to_bytes(4, "big") + bytes(16), ref.slot3(g))[1] == ref.LENGTH
