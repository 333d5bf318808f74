"""The entry points of the per-session cursors of the device random streams (gc_rand_*_cur*) are in include/gcengine.h with
the agreed prototypes, libgcengine.so exports them, the header is still plain C99, the ABI version has not moved, and the
argument checks that come before anything touches a device answer as the header says.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from mpc_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = """
int gc_rand_cur_set_dev(gc_rand *, void *d_cur, uint64_t pos);
int gc_rand_fill_cur_dev(gc_rand *, void *d_cur, size_t nbytes, void *d_out, size_t stride, void *d_status);
int gc_rand_scalars_cur_dev(gc_rand *, void *d_cur, const uint8_t max[32], size_t count, void *d_out, void *d_status);
int gc_rand_fill_cur(gc_rand *, uint64_t *cur, size_t nbytes, uint8_t *out, size_t stride, size_t *bad_session);
int gc_rand_scalars_cur(gc_rand *, uint64_t *cur, const uint8_t max[32], size_t count, uint8_t *out, size_t *bad_session);
"""


def squeeze(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def new_names():
    return re.findall(r"\b(gc_rand_[a-z_]+)\(", PROTOTYPES)


def test_the_prototypes_are_in_the_header():
    header = squeeze(open(engine.HEADER).read())
    protos = PROTOTYPES.strip().splitlines()
    assert len(protos) == 5 == len(set(new_names()))
    for p in protos:
        assert squeeze(p) in header, p


def test_the_library_exports_them_and_the_abi_version_stays():
    L = engine.lib()
    for n in new_names():
        assert hasattr(L, n), "libgcengine.so does not export %s" % n
    assert L.gc_abi_version() == engine.ABI_VERSION == 2
    assert "#define GC_ABI_VERSION 2" in squeeze(open(engine.HEADER).read())


def test_the_header_still_compiles_as_c99(tmp_path):
    src = tmp_path / "rand_cursor_abi.c"
    body = ['#include "gcengine.h"', "typedef void (*fn)(void);", "fn table[] = {"]
    body += ["    (fn)%s," % n for n in new_names()]
    body += ["};", "int main(void) { return sizeof table == 0; }"]
    src.write_text("\n".join(body) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-Wno-cast-function-type",
                        "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "rand_cursor_abi.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_refusals_without_a_gpu():
    """what is refused before anything touches a device.  A handle cannot exist without a device, so every call here has a
    NULL one; the refusals that need a handle (zero sizes, stride, alignment, max of 0 and 1 on a live handle) are held on
    the device by tests/test_gpu_rand_cursor.py."""
    L = engine.lib()
    cur = np.zeros(4, np.uint64)
    out = np.zeros((3, 64), np.uint8)
    st = np.zeros(2, np.uint64)
    pc, po, ps = (a.ctypes.data_as(C.c_void_p) for a in (cur, out, st))
    odd = C.c_void_p(cur.ctypes.data + 4)  # a misaligned cursor array
    bad = C.c_size_t(engine._NONE)
    for mx in (0, 1, 2, engine.P256_N):
        m = np.frombuffer(mx.to_bytes(32, "big"), np.uint8).ctypes.data_as(C.c_void_p)
        for c in (pc, odd, None):
            assert L.gc_rand_scalars_cur_dev(None, c, m, 1, po, ps) == engine.GC_E_ARG
            assert L.gc_rand_scalars_cur(None, c, m, 1, po, C.byref(bad)) == engine.GC_E_ARG
        assert L.gc_rand_scalars_cur_dev(None, pc, m, 0, po, ps) == engine.GC_E_ARG  # count = 0 is nothing on a HANDLE
    assert L.gc_rand_scalars_cur_dev(None, pc, None, 1, po, ps) == engine.GC_E_ARG
    for c in (pc, odd, None):
        assert L.gc_rand_cur_set_dev(None, c, 0) == engine.GC_E_ARG
        assert L.gc_rand_fill_cur_dev(None, c, 16, po, 64, ps) == engine.GC_E_ARG
        assert L.gc_rand_fill_cur(None, c, 16, po, 64, None) == engine.GC_E_ARG
    assert L.gc_rand_fill_cur_dev(None, pc, 0, po, 0, ps) == engine.GC_E_ARG
    assert L.gc_rand_fill_cur_dev(None, pc, 16, po, 64, None) == engine.GC_E_ARG
    assert bad.value == engine._NONE and not cur.any() and not out.any() and not st.any()


def test_the_python_binding_refuses_a_modulus_past_256_bits():
    import pytest
    for mx in (1 << 256, -1):
        with pytest.raises(engine.EngineError) as e:
            engine._max32(mx)
        assert e.value.code == engine.GC_E_ARG
    assert engine._max32(engine.P256_N).tobytes() == engine.P256_N.to_bytes(32, "big")
