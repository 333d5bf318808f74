"""The entry points of DESIGN.md §20 — gc_stream_eval_batch_return_labels(_dev) and gc_stream_eval_batch_in_* — are declared in
include/gcengine.h with the prototypes of the design, exported, bound in Python with arguments of the same kind, named by the
C++ mirror and by the Go stub, and answer a NULL handle with GC_E_ARG.  No GPU is needed: nothing here reaches the device."""
import ctypes as C
import os
import re
import subprocess

from mpc_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = {
    "gc_stream_eval_batch_return_labels_dev":
        "int (gc_stream_eval_batch *, const uint32_t *ids, uint32_t n, void *d_labels_out)",
    "gc_stream_eval_batch_return_labels":
        "int (gc_stream_eval_batch *, const uint32_t *ids, uint32_t n, gc_label *labels_out)",
    "gc_stream_eval_batch_in_create":
        "gc_stream_eval_batch_in * (gc_stream_eval_batch *, uint32_t ref_session, size_t max_message_bytes, int *status)",
    "gc_stream_eval_batch_in_free":
        "void (gc_stream_eval_batch_in *)",
    "gc_stream_eval_batch_in_feed":
        "int (gc_stream_eval_batch_in *, const uint8_t *chunk, size_t stride, size_t len, size_t *taken, uint32_t *next_op)",
    "gc_stream_eval_batch_in_stats":
        "int (const gc_stream_eval_batch_in *, uint64_t *steps, uint64_t *bytes_per_session, uint64_t *uploads, "
        "uint64_t *carried_bytes)",
}


def squeeze(text):
    return re.sub(r"\s*([(),*])\s*", r"\1", re.sub(r"\s+", " ", text)).strip()


def header_text():
    text = open(os.path.join(ROOT, "include", "gcengine.h")).read()
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_the_header_declares_the_prototypes_of_the_design():
    text = header_text()
    assert re.search(r"typedef struct gc_stream_eval_batch_in gc_stream_eval_batch_in;", text)
    assert re.search(r"#define GC_ABI_VERSION 2\b", text)
    for name, want in PROTOS.items():
        m = re.search(r"([A-Za-z_][A-Za-z0-9_ ]*?\*?)\s*\b%s\s*\(([^()]*)\)\s*;" % name, text)
        assert m, name
        ret, params = want.split(" (", 1)
        assert squeeze(m.group(1)) == squeeze(ret), name
        assert squeeze("(" + m.group(2) + ")") == squeeze("(" + params), name


def test_the_header_still_compiles_as_c99(tmp_path):
    src = tmp_path / "intake_abi.c"
    body = ['#include "gcengine.h"', "typedef void (*fn)(void);", "fn table[] = {"]
    body += ["    (fn)%s," % n for n in PROTOS]
    body += ["};",
             "int use(gc_stream_eval_batch_in *h, const uint8_t *p, size_t n) {",
             "    size_t taken = 0; uint32_t op = 0;",
             "    return gc_stream_eval_batch_in_feed(h, p, n, n, &taken, &op) + (int)taken + (int)op + (int)(sizeof table);",
             "}"]
    src.write_text("\n".join(body) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-Wno-cast-function-type", "-I",
                        os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "intake_abi.o")],
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
    for method in ("return_labels", "return_labels_dev", "intake"):
        assert hasattr(engine.StreamEvalBatch, method)
    for method in ("feed", "stats", "close", "word_bytes_taken"):
        assert hasattr(engine.StreamEvalBatchIn, method)


def test_the_cpp_mirror_and_the_go_stub_name_them():
    hpp = open(os.path.join(ROOT, "include", "mpc_host.hpp")).read()
    go = open(os.path.join(ROOT, "go", "circuit", "stream_batch_hip.go")).read()
    for name in PROTOS:
        assert name + "(" in hpp, "include/mpc_host.hpp does not call %s" % name
        assert "C." + name + "(" in go, "go/circuit/stream_batch_hip.go does not call %s" % name
    assert "class StreamEvalBatchIn" in hpp and "type StreamEvalBatchIn struct" in go and "io.Reader" in go
    assert "func (in *StreamEvalBatchIn) Return(" in go  # the OpReturn handler on return_labels


def test_the_documents_name_them():
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in PROTOS:
        assert integration.count("`%s`" % name) >= 1, name
    assert "gc_stream_eval_batch_in_create / _free / _feed / _stats" in integration
    assert re.search(r"^## 20\. ", design, flags=re.M) and "gc_stream_eval_batch_in_feed" in design


def test_null_handles_are_refused():
    L = engine.lib()
    ids = (C.c_uint32 * 2)(1, 2)
    lab = (C.c_uint8 * 64)()
    assert L.gc_stream_eval_batch_return_labels_dev(None, ids, 2, lab) == engine.GC_E_ARG
    assert L.gc_stream_eval_batch_return_labels(None, ids, 2, lab) == engine.GC_E_ARG
    st = C.c_int(0)
    assert not L.gc_stream_eval_batch_in_create(None, 0, 1 << 20, C.byref(st)) and st.value == engine.GC_E_ARG
    taken, op = C.c_size_t(7), C.c_uint32(7)
    assert L.gc_stream_eval_batch_in_feed(None, lab, 64, 16, C.byref(taken), C.byref(op)) == engine.GC_E_ARG
    v = [C.c_uint64(0) for _ in range(4)]
    assert L.gc_stream_eval_batch_in_stats(None, *[C.byref(x) for x in v]) == engine.GC_E_ARG
    L.gc_stream_eval_batch_in_free(None)  # (as free(NULL))
