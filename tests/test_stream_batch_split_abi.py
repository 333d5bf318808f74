"""The entry points of DESIGN.md §21 — gc_stream_batch_out_create_split, gc_stream_batch_out_split_stats and the two
_set_fallback calls — are declared in include/gcengine.h with the prototypes of the design, exported, bound in Python with
arguments of the same kind, named by the C++ mirror and by the Go stub, and answer a NULL handle with GC_E_ARG.  No GPU is
needed: nothing here reaches the device (that _split_stats of an unsplit handle is zeros needs a handle, so it is checked in
tests/test_gpu_stream_batch_split.py)."""
import ctypes as C
import os
import re
import subprocess

from mpc_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = {
    "gc_stream_batch_out_create_split":
        "gc_stream_batch_out * (gc_stream_batch *, size_t window_bytes, uint32_t nwindows, int *status)",
    "gc_stream_batch_out_split_stats":
        "int (const gc_stream_batch_out *, uint64_t *split_steps, uint64_t *segments)",
    "gc_stream_batch_set_fallback":
        "int (gc_stream_batch *, int on)",
    "gc_stream_eval_batch_set_fallback":
        "int (gc_stream_eval_batch *, int on)",
}


def squeeze(text):
    return re.sub(r"\s*([(),*])\s*", r"\1", re.sub(r"\s+", " ", text)).strip()


def header_text():
    text = open(os.path.join(ROOT, "include", "gcengine.h")).read()
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_the_header_declares_the_prototypes_of_the_design():
    text = header_text()
    assert re.search(r"#define GC_ABI_VERSION 2\b", text)
    for name, want in PROTOS.items():
        m = re.search(r"([A-Za-z_][A-Za-z0-9_ ]*?\*?)\s*\b%s\s*\(([^()]*)\)\s*;" % name, text)
        assert m, name
        ret, params = want.split(" (", 1)
        assert squeeze(m.group(1)) == squeeze(ret), name
        assert squeeze("(" + m.group(2) + ")") == squeeze("(" + params), name


def test_the_header_still_compiles_as_c99(tmp_path):
    src = tmp_path / "split_abi.c"
    body = ['#include "gcengine.h"', "typedef void (*fn)(void);", "fn table[] = {"]
    body += ["    (fn)%s," % n for n in PROTOS]
    body += ["};",
             "int use(gc_stream_batch *s, gc_stream_eval_batch *e) {",
             "    int st = 0; uint64_t a = 0, b = 0;",
             "    gc_stream_batch_out *h = gc_stream_batch_out_create_split(s, 1 << 20, 3, &st);",
             "    return st + gc_stream_batch_out_split_stats(h, &a, &b) + gc_stream_batch_set_fallback(s, 1) +",
             "           gc_stream_eval_batch_set_fallback(e, 1) + (int)(a + b) + (int)(sizeof table);",
             "}"]
    src.write_text("\n".join(body) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-Wno-cast-function-type", "-I",
                        os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "split_abi.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_binds_them_with_arguments_of_the_same_kind():
    text = header_text()
    L = engine.lib()
    for name in PROTOS:
        params = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % name, text).group(1).split(",")
        fn = getattr(L, name)
        assert len(fn.argtypes) == len(params), name
        for k, (t, p) in enumerate(zip(fn.argtypes, params)):
            is_ptr = t is C.c_void_p or t is C.c_char_p or hasattr(t, "contents")
            assert is_ptr == ("*" in p), "%s argument %d" % (name, k + 1)
    assert hasattr(engine.StreamBatchOut, "split_stats")
    assert hasattr(engine.StreamBatch, "set_fallback") and hasattr(engine.StreamEvalBatch, "set_fallback")
    import inspect
    assert inspect.signature(engine.StreamBatch.out).parameters["split"].default is False


def test_the_cpp_mirror_and_the_go_stub_name_them():
    hpp = open(os.path.join(ROOT, "include", "mpc_host.hpp")).read()
    go = open(os.path.join(ROOT, "go", "circuit", "stream_batch_hip.go")).read()
    for name in PROTOS:
        assert name + "(" in hpp, "include/mpc_host.hpp does not call %s" % name
        assert "C." + name + "(" in go, "go/circuit/stream_batch_hip.go does not call %s" % name


def test_the_documents_name_them():
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in PROTOS:
        assert integration.count("`%s`" % name) >= 1, name
    assert re.search(r"^## 21\. ", design, flags=re.M) and "k_sb_serialise_range" in design


def test_null_handles_are_refused():
    L = engine.lib()
    st = C.c_int(0)
    assert not L.gc_stream_batch_out_create_split(None, 1 << 20, 3, C.byref(st)) and st.value == engine.GC_E_ARG
    a, b = C.c_uint64(7), C.c_uint64(7)
    assert L.gc_stream_batch_out_split_stats(None, C.byref(a), C.byref(b)) == engine.GC_E_ARG
    assert L.gc_stream_batch_set_fallback(None, 1) == engine.GC_E_ARG
    assert L.gc_stream_eval_batch_set_fallback(None, 1) == engine.GC_E_ARG
