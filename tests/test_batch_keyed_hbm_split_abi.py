"""gc_batch_set_keyed_hbm_form / gc_batch_keyed_hbm_form / gc_batch_debug_keyed_hbm_hash_waves (which form of the keyed HBM-wire
kernels a path-2 pass runs: the plain one or the split one with hash waves and free waves on wide levels) through the layers
that need no GPU: the C header (still plain C99), the library's exports, the Python, Go and C++ mirrors, INTEGRATION.md."""
import os
import re
import subprocess

import pytest

from mpc_amd import engine
from tests.test_abi_plan import _go_calls, _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("gc_batch_set_keyed_hbm_form", "gc_batch_keyed_hbm_form", "gc_batch_debug_keyed_hbm_hash_waves")


def header():
    text = open(os.path.join(ROOT, "include", "gcengine.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def test_the_three_prototypes_are_in_the_header_and_the_abi_version_stays():
    h = header()
    assert "int gc_batch_set_keyed_hbm_form(gc_batch *, int form);" in h
    assert "int gc_batch_keyed_hbm_form(const gc_batch *);" in h
    assert "int gc_batch_debug_keyed_hbm_hash_waves(gc_batch *, uint32_t garble_h, uint32_t eval_h);" in h
    assert "#define GC_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "gcengine.h")).read()
    protos = _prototypes()
    assert protos["gc_batch_set_keyed_hbm_form"] == ["ptr", "scalar"] and protos["gc_batch_keyed_hbm_form"] == ["ptr"]
    assert protos["gc_batch_debug_keyed_hbm_hash_waves"] == ["ptr", "scalar", "scalar"]


def test_header_compiles_as_c99_and_the_calls_can_be_named_from_c(tmp_path):
    src = tmp_path / "keyed_form.c"
    src.write_text('#include "gcengine.h"\n'
                   "int use(gc_batch *g) {\n"
                   "    if (gc_batch_set_keyed_hbm_form(g, 2) != GC_OK) return GC_E_ARG;\n"
                   "    if (gc_batch_debug_keyed_hbm_hash_waves(g, 12u, 9u) != GC_OK) return GC_E_ARG;\n"
                   "    return gc_batch_keyed_hbm_form(g);\n"
                   "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                        str(src), "-o", str(tmp_path / "keyed_form.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_exports_the_calls_and_null_handles_are_refused():
    L = engine.lib()
    assert L.gc_batch_keyed_hbm_form(None) == 0
    assert L.gc_batch_set_keyed_hbm_form(None, 2) == engine.GC_E_ARG
    assert L.gc_batch_debug_keyed_hbm_hash_waves(None, 0, 0) == engine.GC_E_ARG


def test_python_binding():
    assert isinstance(engine.Batch.keyed_hbm_form, property)
    assert callable(engine.Batch.set_keyed_hbm_form) and callable(engine.Batch.debug_keyed_hbm_hash_waves)


@pytest.mark.parametrize("path,names", [
    ("go/circuit/batch_hip.go", ["func (p *BatchPipeline) KeysHbmForm() int", "func (p *BatchPipeline) SetKeysHbmForm(form int) error",
                                 "func (p *BatchPipeline) DebugKeysHbmHashWaves(garble, eval uint32) error"]
     + ["C.%s(" % c for c in CALLS]),
    ("include/mpc_host.hpp", ["BatchKeysHbmForm", "SetBatchKeysHbmForm"] + ["%s(" % c for c in CALLS[:2]]),
    ("mpc_amd/engine.py", ['"%s"' % c for c in CALLS]),
    ("mpc_amd/csrc/kernels.h", ["launch_fused_hbm_keyed_split("]),
])
def test_mirrors_name_the_calls(path, names):
    text = open(os.path.join(ROOT, path)).read()
    for n in names:
        assert n in text, "%s does not name %s" % (path, n)


def test_go_shim_calls_both_batches_with_the_prototypes_arguments():
    protos = _prototypes()
    calls = [(n, a) for n, a in _go_calls(open(os.path.join(ROOT, "go", "circuit", "batch_hip.go")).read()) if n in CALLS]
    for name in CALLS:
        mine = [a for n, a in calls if n == name]
        assert sorted(a[0] for a in mine) == ["p.ev", "p.gb"], name  # the garbler's and the evaluator's batch
        for a in mine:
            assert len(a) == len(protos[name])
    for a in [a for n, a in calls if n == "gc_batch_set_keyed_hbm_form"]:
        assert a[1] == "C.int(form)"
    for a in [a for n, a in calls if n == "gc_batch_debug_keyed_hbm_hash_waves"]:
        assert a[1:] == ["C.uint32_t(garble)", "C.uint32_t(eval)"]


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "host.cpp"
    src.write_text('#include "mpc_host.hpp"\n'
                   "int use(gc_batch *g) {\n"
                   "    if (mpc::circuit::BatchKeysHbmForm(g) == 1) mpc::circuit::SetBatchKeysHbmForm(g, 2);\n"
                   "    return mpc::circuit::BatchKeysHbmForm(g);\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "host.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_integration_rows():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    head = doc[: doc.index("<!-- abi-index:begin -->")]
    rows = [l for l in head.splitlines() if l.startswith("|") and "`gc_batch_set_keyed_hbm_form`" in l]
    assert len(rows) == 1, "one row of the table of additive calls"
    for word in ("`gc_batch_keyed_hbm_form`", "`gc_batch_debug_keyed_hbm_hash_waves`", "KeysHbmForm", "SetKeysHbmForm",
                 "tests/test_gpu_batch_keyed_hbm_split.py"):
        assert word in rows[0], word
    index = doc[doc.index("<!-- abi-index:begin -->"):]
    for c in CALLS:
        assert re.search(r"^\| `%s` \| \d+ \|" % c, index, re.M), c


def test_design_says_what_was_built():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[re.search(r"^## 15\b", design, re.M).start():]
    sec = sec[: re.search(r"^## 16\b", sec, re.M).start()]
    for word in ("k_garble_hbm_keyed_split", "k_eval_hbm_keyed_split", "gc_batch_set_keyed_hbm_form", "hbm_keyed_split.h"):
        assert word in sec, word
