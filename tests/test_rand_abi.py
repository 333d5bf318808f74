"""The entry points of the device random streams (gc_rand_*) are in include/gcengine.h with the agreed prototypes,
libgcengine.so exports them, the header is still plain C99, the ABI version has not moved, the argument checks that come
before anything touches a device answer as the header says, and the grid cap the GPU tests size themselves from is where the
binding looks.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from mpc_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = """
gc_rand *gc_rand_create(gc_ctx *, const uint8_t *seeds, size_t keylen, const uint8_t *ivs, size_t S, int *status);
gc_rand *gc_rand_create_dev(gc_ctx *, const void *d_seeds, size_t keylen, const void *d_ivs, size_t S, int *status);
void gc_rand_free(gc_rand *);
int gc_rand_info(const gc_rand *, size_t *S, size_t *keylen, uint64_t *pos);
int gc_rand_seek(gc_rand *, uint64_t pos);
int gc_rand_fill_dev(gc_rand *, size_t nbytes, void *d_out, size_t stride);
int gc_rand_fill(gc_rand *, size_t nbytes, uint8_t *out, size_t stride);
int gc_rand_gmw_shares_dev(gc_rand *, size_t words, void *d_a, void *d_b);
"""


def squeeze(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def new_names():
    return re.findall(r"\b(gc_rand_[a-z_]+)\(", PROTOTYPES)


def test_the_prototypes_are_in_the_header():
    header = squeeze(open(engine.HEADER).read())
    assert "typedef struct gc_rand gc_rand;" in header
    protos = PROTOTYPES.strip().splitlines()
    assert len(protos) == 8 == len(set(new_names()))
    for p in protos:
        assert squeeze(p) in header, p


def test_the_library_exports_them_and_the_abi_version_stays():
    L = engine.lib()
    for n in new_names():
        assert hasattr(L, n), "libgcengine.so does not export %s" % n
    assert L.gc_abi_version() == engine.ABI_VERSION == 2
    assert "#define GC_ABI_VERSION 2" in squeeze(open(engine.HEADER).read())


def test_the_header_still_compiles_as_c99(tmp_path):
    src = tmp_path / "rand_abi.c"
    body = ['#include "gcengine.h"', "typedef void (*fn)(void);", "fn table[] = {"]
    body += ["    (fn)%s," % n for n in new_names()]
    body += ["};", "int main(void) { return sizeof table == 0; }"]
    src.write_text("\n".join(body) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-Wno-cast-function-type",
                        "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "rand_abi.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_and_zero_arguments_are_refused_without_a_gpu():
    """the checks that come before anything touches a device: a NULL ctx, handle or array"""
    L = engine.lib()
    seeds = np.zeros((3, 32), np.uint8)
    p = seeds.ctypes.data_as(C.c_void_p)
    for create in (L.gc_rand_create, L.gc_rand_create_dev):
        st = C.c_int(0)
        assert not create(None, p, 32, None, 3, C.byref(st)) and st.value == engine.GC_E_ARG
        st = C.c_int(0)
        assert not create(None, None, 32, None, 3, C.byref(st)) and st.value == engine.GC_E_ARG
        assert not create(None, p, 32, None, 0, None)  # a NULL status is allowed
    assert L.gc_rand_info(None, None, None, None) == engine.GC_E_ARG
    assert L.gc_rand_seek(None, 0) == engine.GC_E_ARG
    assert L.gc_rand_fill_dev(None, 16, None, 16) == engine.GC_E_ARG
    assert L.gc_rand_fill_dev(None, 0, None, 0) == engine.GC_E_ARG  # nbytes = 0 does nothing on a HANDLE; there is none
    assert L.gc_rand_fill(None, 16, p, 16) == engine.GC_E_ARG
    assert L.gc_rand_gmw_shares_dev(None, 4, None, None) == engine.GC_E_ARG
    L.gc_rand_free(None)  # a no-op


def test_the_grid_cap_is_exported_to_python():
    grid, threads, run = engine.rand_kernel_shape()
    assert grid >= 1 and threads % 64 == 0 and run == 64
    from tests.util import kernel_constants
    assert (grid, threads) == kernel_constants("kRandGrid", "kRandThreads")
