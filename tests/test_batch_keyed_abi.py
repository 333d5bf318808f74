"""The per-instance-key batch calls (gc_batch_garble_keyed / gc_batch_eval_keyed / gc_batch_keyed_supported) through the
layers that need no GPU: the C header (still plain C99), the library's exports, the Python, Go and C++ mirrors, and the
documents that state their scope."""
import os
import re
import subprocess

import pytest

from mpc_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["gc_batch_garble_keyed", "gc_batch_eval_keyed", "gc_batch_keyed_supported"]


def header():
    text = open(os.path.join(ROOT, "include", "gcengine.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def test_the_three_prototypes_are_in_the_header():
    h = header()
    assert "int gc_batch_garble_keyed(gc_batch *, const void *d_keys, size_t keylen, const void *d_rnd);" in h
    assert "int gc_batch_eval_keyed(gc_batch *evaluator, const void *d_keys, size_t keylen, const gc_batch *tables);" in h
    assert "int gc_batch_keyed_supported(const gc_batch *);" in h
    # additive: the version and the one-key twins are what they were
    assert "#define GC_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "gcengine.h")).read()
    assert "int gc_batch_garble(gc_batch *, const uint8_t *key, size_t keylen, const void *d_rnd);" in h
    assert "int gc_batch_eval(gc_batch *evaluator, const uint8_t *key, size_t keylen, const gc_batch *tables);" in h
    # the host-only view of the flattened geometry that the keyed tests predict tiles from: additive as well
    assert "int gc_plan_flat_geometry(const gc_plan *, uint32_t *unit_stride16, uint32_t *max_parts);" in h


def test_header_compiles_as_c99_and_the_calls_can_be_named_from_c(tmp_path):
    src = tmp_path / "keyed.c"
    src.write_text('#include "gcengine.h"\n'
                   "int use(gc_batch *g, gc_batch *e, const void *k, const void *r) {\n"
                   "    if (!gc_batch_keyed_supported(g)) return GC_E_ARG;\n"
                   "    if (gc_batch_garble_keyed(g, k, 32, r) != GC_OK) return GC_E_KEYSIZE;\n"
                   "    return gc_batch_eval_keyed(e, k, 32, g);\n"
                   "}\n"
                   "int geometry(const gc_plan *p) {\n"
                   "    uint32_t stride16, parts;\n"
                   "    return gc_plan_flat_geometry(p, &stride16, &parts) == GC_OK ? (int)(stride16 + parts) : -1;\n"
                   "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                        str(src), "-o", str(tmp_path / "keyed.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_exports_the_calls_and_null_handles_are_argument_errors():
    L = engine.lib()
    for name in CALLS:
        assert hasattr(L, name), name
    assert L.gc_batch_keyed_supported(None) == 0
    assert L.gc_batch_garble_keyed(None, None, 32, None) == engine.GC_E_ARG
    assert L.gc_batch_eval_keyed(None, None, 32, None) == engine.GC_E_ARG
    assert hasattr(L, "gc_plan_flat_geometry")
    assert L.gc_plan_flat_geometry(None, None, None) == engine.GC_E_ARG


def test_python_binding_has_the_methods():
    for m in ("garble_keyed", "eval_keyed", "keyed_supported"):
        assert callable(getattr(engine.Batch, m)), m
    assert callable(engine.Plan.flat_geometry) and callable(engine.DeviceCircuit.flat_geometry)


@pytest.mark.parametrize("path,names", [
    ("go/circuit/batch_hip.go", ["GarbleBatchKeys", "EvalBatchKeys", "C.gc_batch_garble_keyed(", "C.gc_batch_eval_keyed(",
                                 "C.gc_batch_keyed_supported("]),
    ("include/mpc_host.hpp", ["GarbleBatchKeys", "EvalBatchKeys", "gc_batch_garble_keyed(", "gc_batch_eval_keyed(",
                              "gc_batch_keyed_supported("]),
])
def test_go_and_cpp_mirrors_name_the_calls(path, names):
    text = open(os.path.join(ROOT, path)).read()
    for n in names:
        assert n in text, "%s does not name %s" % (path, n)


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "host.cpp"
    src.write_text('#include "mpc_host.hpp"\n'
                   "void use(gc_batch *g, gc_batch *e, const void *k, const void *r) {\n"
                   "    if (!mpc::circuit::BatchKeysSupported(g)) return;\n"
                   "    mpc::circuit::GarbleBatchKeys(g, k, 32, r);\n"
                   "    mpc::circuit::EvalBatchKeys(e, k, 32, g);\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "host.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_documents_state_the_scope_and_the_reference_lines():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 15\b.*key", design, re.M | re.I)
    sec = design[re.search(r"^## 15\b", design, re.M).start():]
    for word in ("k_expand_keys", "k_garble_flat_keyed", "k_eval_flat_keyed", "gc_batch_keyed_supported", "Out of scope"):
        assert word in sec, word
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    row = [l for l in integ.splitlines() if "garbler.go:47-53,64" in l and l.startswith("|")]
    assert row and "gc_batch_garble_keyed" in row[0] and "gc_batch_eval_keyed" in row[0]
    assert "gc_batch_garble_keyed" in open(os.path.join(ROOT, "README.md")).read()
