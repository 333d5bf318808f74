"""CPU check of mpc_amd/csrc/stream_wire.h, the one reader and one writer of the streamed gate wire format.
The header is compiled into a stand-alone program (tests/cpp/stream_wire_check.cpp) with the host compiler under
AddressSanitizer and UBSan; this side prepares a case file — the oracle's bytes, tests/hostile_fuzz.py's reading of them and
the class it expects for every hostile block — and the program replays it.  Nothing is loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from mpc_amd.circuit import GATE
from tests import hostile_fuzz as hf
from tests.test_oracle_stream import make_program
from tests.test_stream_batch_host import STEP_BYTES, alias_gates
from tests.util import drbg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("stream_wire") / "stream_wire_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(CPP, "stream_wire_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def replay(program, tmp_path, lines, walks, steps=0):
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.split() == [str(walks), "walks,", str(steps), "steps"]  # every line was replayed


def expected(block, ngates, ntmp, nwires):
    """(the status the walk must return, the bytes it takes if that is 'ok'): 'arg' where one of the gates the reference's
    reading gets through is refused by design (hostile_fuzz.stricter over exactly those gates: the walk meets it first), else
    that reading's own 'rows' / 'gate', else 'ok'.  stricter's "more gates than bytes" is the callers' test in front of the
    walk, not the walk's: it cannot come up over the gates that were read, each of which has its five bytes and more."""
    gates, err = hf.parse(block, ngates)
    why = hf.stricter(block, len(gates), ntmp, nwires)
    assert why != "more gates than bytes"
    cls = "arg" if why else err or "ok"
    return cls, gates[-1][6] + 16 * gates[-1][7] if cls == "ok" and gates else 0


def walk_line(block, ngates, ntmp, nwires, want=None):
    cls, used = expected(block, ngates, ntmp, nwires)
    assert want is None or cls in want, (cls, want)
    return "walk %d %d %d %s %d %s" % (ngates, ntmp, nwires, cls, used, bytes(block).hex() or "-")


@pytest.fixture(scope="module")
def round_trip_steps():
    """(gates, nwires, in, out, ntmp, numWires, the oracle's bytes) of the three steps of make_program at both bases and of the
    in-place step"""
    out = []
    for base in (0, 0x20000):
        steps, prim = make_program(base)
        og = oracle.Stream(drbg("sbk", 32), drbg("sbr", 16 * (len(prim) + 1)), prim)
        for (c, in_, out_), nbytes in zip(steps, STEP_BYTES[base]):
            data = og.garble(c.Gates, c.NumWires, in_, out_)
            assert len(data) == nbytes
            out.append((c.Gates, c.NumWires, in_, out_, c.NumWires, max(max(in_), max(out_)) + 1, data))
    og = oracle.Stream(drbg("alias", 32), drbg("alias-rnd", 64), [0, 1, 2])
    out.append((alias_gates(), 5, [0, 1], [0, 2], 5, 3, og.garble(alias_gates(), 5, [0, 1], [0, 2])))
    return out


def test_round_trip_against_the_oracle(program, tmp_path, round_trip_steps):
    """gate_form + put_gate_head write the oracle's bytes outside the rows and count its length; read_gate and walk_block read
    them as hostile_fuzz.parse does; ssa_gate_list is single-assignment; live_outputs marks the last writer of every id"""
    lines, widths = [], set()
    for gates, nwires, in_, out_, ntmp, numwires, data in round_trip_steps:
        parsed, err = hf.parse(data, len(gates))
        assert err is None and hf.stricter(data, len(gates), ntmp, numwires) is None
        widths |= {q[3] for q in parsed}
        lines.append("step %d %d %d %d %d %d" % (len(gates), nwires, len(in_), len(out_), ntmp, numwires))
        lines.append("gates " + " ".join("%d %d %d %d" % (g["in0"], g["in1"], g["out"], g["op"]) for g in gates))
        lines.append("in " + " ".join(map(str, in_)))
        lines.append("out " + " ".join(map(str, out_)))
        lines.append("bytes " + bytes(data).hex())
        lines.append("parse " + " ".join("%d %d %d %d %d %d %d %d %d" % ((p0, op, flags, short) + tuple((ids + [0])[:3]) + (rpos, nrows))
                                         for p0, op, flags, short, ids, idpos, rpos, nrows in parsed))
    assert widths == {True, False}
    replay(program, tmp_path, lines, 0, len(round_trip_steps))


def five_gates(base):
    """one gate of each operation — wires 0, 1 inputs; 2, 3, 4 tmp; 5, 6 outputs — as the oracle writes it: (bytes, ntmp,
    numWires, hostile_fuzz's reading).  base 0: every id in the 16-bit form; base 0x20000: the 32-bit form wherever a global
    wire is named"""
    gates = np.zeros(5, GATE)
    gates[0] = (0, 1, 2, 0, 0)  # XOR
    gates[1] = (2, 0, 3, 1, 0)  # XNOR
    gates[2] = (2, 3, 4, 2, 0)  # AND
    gates[3] = (4, 1, 5, 3, 0)  # OR
    gates[4] = (4, 0, 6, 4, 0)  # INV
    in_, out_ = [base + 7, base + 9], [base + 11, base + 12]
    og = oracle.Stream(drbg("five", 32), drbg("five-rnd", 16 * 3), in_)
    data = og.garble(gates, 7, in_, out_)
    parsed, err = hf.parse(data, 5)
    assert err is None and [q[1] for q in parsed] == [0, 1, 2, 3, 4]
    assert {q[3] for q in parsed} == ({True} if base == 0 else {True, False})
    return bytes(data), 7, base + 13, parsed


def patched(data, at, value, size):
    b = bytearray(data)
    b[at:at + size] = value.to_bytes(size, "big")
    return bytes(b)


@pytest.mark.parametrize("base", [0, 0x20000])
def test_refusals_at_the_smallest_shapes(program, tmp_path, base):
    data, ntmp, nwires, parsed = five_gates(base)
    valid = walk_line(data, 5, ntmp, nwires, ("ok",))
    lines = ["fresh", valid]
    # cut off at every length: never accepted, never read beyond the bytes
    for n in range(len(data)):
        lines.append(walk_line(data[:n], 5, ntmp, nwires, ("rows", "gate")))
        assert (lines[-1].split()[4] == "gate") == (hf.parse(data[:n], 5)[1] == "gate")
    # an unknown operation, in every gate's place
    for q in parsed:
        for op in range(5, 16):
            lines.append(walk_line(patched(data, q[0], (data[q[0]] & 0xf0) | op, 1), 5, ntmp, nwires, ("gate",)))
    xnor, or_ = parsed[1], parsed[3]
    sz = lambda q: 2 if q[3] else 4
    # a tmp operand >= ntmp (by the header, and by the id); a tmp read before it is written; a global id == nwires (by the
    # header: the largest id the block names, and by the id, operand and output)
    stale = patched(data, xnor[5][0], 4, sz(xnor))  # XNOR reads tmp 4, which AND writes after it
    lines.append(walk_line(data, 5, 4, nwires, ("arg",)))
    lines.append(walk_line(patched(data, xnor[5][0], ntmp, sz(xnor)), 5, ntmp, nwires, ("arg",)))
    lines.append(walk_line(stale, 5, ntmp, nwires, ("arg",)))
    # (... and a tmp OUTPUT == ntmp that no gate reads: OR and INV read tmp 2 and 3 instead of AND's 4)
    unread = patched(patched(data, or_[5][0], 2, sz(or_)), parsed[4][5][0], 3, sz(parsed[4]))
    lines.append(walk_line(unread, 5, 4, nwires, ("arg",)))
    lines.append(walk_line(unread, 5, 5, nwires, ("ok",)))
    lines.append(walk_line(data, 5, ntmp, nwires - 1, ("arg",)))
    lines.append(walk_line(patched(data, or_[5][1], nwires, sz(or_)), 5, ntmp, nwires, ("arg",)))
    lines.append(walk_line(patched(data, or_[5][2], nwires, sz(or_)), 5, ntmp, nwires, ("arg",)))
    lines.append(walk_line(patched(data, or_[5][2], nwires - 1, sz(or_)), 5, ntmp, nwires, ("ok",)))
    # a tmp written by the block before is not this block's: the valid block, then the stale read, on one set of stamps
    lines += [valid, walk_line(stale, 5, ntmp, nwires, ("arg",)), valid]
    # ... nor one written 2^32 generations ago: the counter wraps between the two blocks, with the same answers
    lines += ["fresh", valid, "gen %d" % 0xFFFFFFFF, walk_line(stale, 5, ntmp, nwires, ("arg",)), valid]
    replay(program, tmp_path, lines, sum(l.startswith("walk") for l in lines))


def test_mutants_are_classified_as_the_python_reader_classifies_them(program, tmp_path, round_trip_steps):
    """300 mutants of the round-trip blocks (tests/hostile_fuzz.mutate, fixed seed), on one set of stamps: ok / rows / gate / arg
    as parse + stricter say, every one of them"""
    rng = np.random.default_rng(20)
    lines, classes = ["fresh"], {}
    for _ in range(300):
        gates, _, _, _, ntmp, numwires, data = round_trip_steps[int(rng.integers(0, len(round_trip_steps)))]
        mut, ngates, what = hf.mutate(rng, data, len(gates))
        lines.append(walk_line(mut, ngates, ntmp, numwires))
        cls = lines[-1].split()[4]
        classes[cls] = classes.get(cls, 0) + 1
    assert sum(classes.values()) == 300 and all(classes.get(c, 0) >= 10 for c in ("ok", "rows", "gate", "arg")), classes
    replay(program, tmp_path, lines, 300)
