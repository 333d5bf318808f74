"""gc_batch_keyed_path / gc_batch_set_keyed_path (which kernels the per-instance-key batch calls run: the flattened ones with the
wires in LDS, or the level-walking ones with the wires in HBM) through the layers that need no GPU: the C header (still plain
C99), the library's exports, the Python, Go and C++ mirrors, and DESIGN.md."""
import os
import re
import subprocess

import pytest

from mpc_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    text = open(os.path.join(ROOT, "include", "gcengine.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def test_the_two_prototypes_are_in_the_header_and_the_abi_version_stays():
    h = header()
    assert "int gc_batch_keyed_path(const gc_batch *);" in h
    assert "int gc_batch_set_keyed_path(gc_batch *, int path);" in h
    assert "int gc_batch_keyed_supported(const gc_batch *);" in h
    assert "#define GC_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "gcengine.h")).read()


def test_header_compiles_as_c99_and_the_calls_can_be_named_from_c(tmp_path):
    src = tmp_path / "keyed_path.c"
    src.write_text('#include "gcengine.h"\n'
                   "int use(gc_batch *g) {\n"
                   "    if (gc_batch_keyed_path(g) == 0 && gc_batch_set_keyed_path(g, 2) != GC_OK) return GC_E_ARG;\n"
                   "    return gc_batch_keyed_path(g);\n"
                   "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                        str(src), "-o", str(tmp_path / "keyed_path.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_exports_the_calls_and_null_handles_are_refused():
    L = engine.lib()
    assert L.gc_batch_keyed_path(None) == 0
    assert L.gc_batch_set_keyed_path(None, 2) == engine.GC_E_ARG
    assert L.gc_batch_keyed_supported(None) == 0


def test_python_binding():
    assert isinstance(engine.Batch.keyed_path, property)
    assert callable(engine.Batch.set_keyed_path)


@pytest.mark.parametrize("path,names", [
    ("go/circuit/batch_hip.go", ["func (p *BatchPipeline) KeysPath() int", "func (p *BatchPipeline) SetKeysPath(path int) error",
                                 "C.gc_batch_keyed_path(", "C.gc_batch_set_keyed_path("]),
    ("include/mpc_host.hpp", ["BatchKeysPath", "SetBatchKeysPath", "gc_batch_keyed_path(", "gc_batch_set_keyed_path("]),
    ("mpc_amd/engine.py", ['"gc_batch_keyed_path"', '"gc_batch_set_keyed_path"']),
])
def test_mirrors_name_the_calls(path, names):
    text = open(os.path.join(ROOT, path)).read()
    for n in names:
        assert n in text, "%s does not name %s" % (path, n)


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "host.cpp"
    src.write_text('#include "mpc_host.hpp"\n'
                   "int use(gc_batch *g) {\n"
                   "    if (mpc::circuit::BatchKeysPath(g) == 0) mpc::circuit::SetBatchKeysPath(g, 2);\n"
                   "    return mpc::circuit::BatchKeysPath(g);\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "host.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_design_names_the_kernels_and_the_scope_call():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[re.search(r"^## 15\b", design, re.M).start():]
    sec = sec[: re.search(r"^## 16\b", sec, re.M).start()]
    for word in ("k_garble_hbm_keyed", "k_eval_hbm_keyed", "gc_batch_keyed_path", "gc_batch_set_keyed_path"):
        assert word in sec, word
    out = design[design.rindex("Out of scope"):]
    for word in ("pipelined", "cooperative", "schedules 0 and 2", "forces path 2", "narrower LDS tile"):
        assert word in out, word
