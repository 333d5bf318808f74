"""The sha2pc entry points (gc_sha2pc_*) are declared in include/gcengine.h, exported by libgcengine.so, the header is still
plain C99 and the ABI version has not moved; gc_sha2pc_layout_plan gives the encoded lengths of sha2pc/encoding.go for
sha256xor and the formulas' values for other geometries; argument errors are refused before any device is touched.  No GPU
needed."""
import ctypes as C
import os
import re
import subprocess

import pytest

from mpc_amd import engine
from mpc_amd.circuit import synthetic_levelised

NAMES = ["gc_sha2pc_garbler_create", "gc_sha2pc_evaluator_create", "gc_sha2pc_garbler_free", "gc_sha2pc_evaluator_free",
         "gc_sha2pc_layout", "gc_sha2pc_layout_plan", "gc_sha2pc_garbler_round1_dev", "gc_sha2pc_evaluator_round2_dev",
         "gc_sha2pc_garbler_round3_dev", "gc_sha2pc_evaluator_round4_dev", "gc_sha2pc_garbler_round1",
         "gc_sha2pc_evaluator_round2", "gc_sha2pc_garbler_round3", "gc_sha2pc_evaluator_round4"]


def squeeze(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def test_the_entry_points_are_declared_and_exported():
    header = squeeze(open(engine.HEADER).read())
    L = engine.lib()
    assert "typedef struct gc_sha2pc_garbler gc_sha2pc_garbler;" in header
    assert "typedef struct gc_sha2pc_evaluator gc_sha2pc_evaluator;" in header
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, header), n
        assert hasattr(L, n), "libgcengine.so does not export %s" % n
    for code, v in (("MAGIC", 1), ("CURVE", 2), ("SESSION", 3), ("SETUP", 4), ("POINT", 5), ("LABEL", 6)):
        assert re.search(r"GC_SHA2PC_%s = %d\b" % (code, v), header) and getattr(engine, "SHA2PC_" + code) == v
    assert L.gc_abi_version() == engine.ABI_VERSION == 2 and "#define GC_ABI_VERSION 2" in header


def test_the_header_still_compiles_as_c99(tmp_path):
    src = tmp_path / "sha2pc_abi.c"
    body = ['#include "gcengine.h"', "typedef void (*fn)(void);", "fn table[] = {"]
    body += ["    (fn)%s," % n for n in NAMES]
    body += ["};", "int main(void) { return sizeof table == 0 || GC_SHA2PC_LABEL != 6; }"]
    src.write_text("\n".join(body) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-Wno-cast-function-type", "-I",
                        os.path.dirname(engine.HEADER), "-c", str(src), "-o", str(tmp_path / "sha2pc_abi.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_layout_of_sha256xor(sha_circ):
    plan = engine.Plan(sha_circ.Gates, sha_circ.NumWires, sha_circ.num_inputs, sha_circ.num_outputs)
    assert plan.info.slab_rows == 42914
    assert engine.sha2pc_layout(plan, 256, 256) == ([80, 8240, 707146], [0, 0, 6], 32)


@pytest.mark.parametrize("ne", [1, 9, 67])
def test_layout_follows_the_formulas(ne):
    ng = 5
    c = synthetic_levelised(4, 11, 0.3, 7, ninputs=ng + ne, or_frac=0.2, inv_frac=0.15)
    plan = engine.Plan(c.Gates, c.NumWires, c.num_inputs, c.num_outputs)
    rows, nout = c.slab_rows(), c.num_outputs
    assert plan.info.slab_rows == rows and nout == 11
    ln, lead, db = engine.sha2pc_layout(plan, ng, ne)
    assert ln == [80, 16 + 32 * ne + (ne + 7) // 8, 42 + 16 * rows + 16 * ng + 32 * nout + 32 * ne]
    assert lead == [0, 0, 6] and db == 2
    assert (lead[2] + 42) % 16 == 0  # the tables, and with them every later field, on a multiple of 16


def test_argument_errors_need_no_device(sha_circ):
    L = engine.lib()
    plan = engine.Plan(sha_circ.Gates, sha_circ.NumWires, sha_circ.num_inputs, sha_circ.num_outputs)
    ln = (C.c_size_t * 3)()
    assert L.gc_sha2pc_layout_plan(None, 256, 256, ln, None, None) == engine.GC_E_ARG
    assert L.gc_sha2pc_layout(None, 256, 256, ln, None, None) == engine.GC_E_ARG
    assert L.gc_sha2pc_layout_plan(plan.h, 256, 255, ln, None, None) == engine.GC_E_ARG
    assert b"input count" in L.gc_last_error()
    assert L.gc_sha2pc_layout_plan(plan.h, 512, 0, ln, None, None) == engine.GC_E_ARG
    assert L.gc_sha2pc_layout_plan(plan.h, 2 ** 32 - 1, 513, ln, None, None) == engine.GC_E_ARG  # no 32-bit wrap
    assert L.gc_sha2pc_layout_plan(plan.h, 256, 256, None, None, None) == engine.GC_OK
    st = C.c_int(0)
    assert not L.gc_sha2pc_garbler_create(None, None, 256, 256, 4, C.byref(st)) and st.value == engine.GC_E_ARG
    st = C.c_int(0)
    assert not L.gc_sha2pc_evaluator_create(None, None, 256, 256, 4, C.byref(st)) and st.value == engine.GC_E_ARG
    L.gc_sha2pc_garbler_free(None)
    L.gc_sha2pc_evaluator_free(None)
    assert L.gc_sha2pc_garbler_round1_dev(None, None, None, None, None, None, 80, None) == engine.GC_E_ARG
    assert L.gc_sha2pc_evaluator_round2_dev(None, None, 80, None, None, None, None, None, 8240, None) == engine.GC_E_ARG
    assert L.gc_sha2pc_garbler_round3_dev(None, None, None, None, None, 8240, None, None, None, None, 707152, None) == engine.GC_E_ARG
    assert L.gc_sha2pc_evaluator_round4_dev(None, None, None, None, None, None, 707152, None, None) == engine.GC_E_ARG
    assert L.gc_sha2pc_garbler_round1(None, None, None, None, None, None, None, None) == engine.GC_E_ARG
    assert L.gc_sha2pc_evaluator_round2(None, None, None, None, None, None, None, None, None) == engine.GC_E_ARG
    assert L.gc_sha2pc_garbler_round3(None, None, None, None, None, None, None, None, None, None, None) == engine.GC_E_ARG
    assert L.gc_sha2pc_evaluator_round4(None, None, None, None, None, None, None, None, None) == engine.GC_E_ARG
