"""The multi-session KOS entry points (gc_kos_multi_*) are in include/gcengine.h with the agreed prototypes, libgcengine.so
exports them, the header is still plain C99, the ABI version has not moved, NULL and zero arguments are refused before any
device is touched, and the launch shape the GPU tests size themselves from is where tests.util.kernel_constants looks.  No
GPU needed."""
import ctypes as C
import os
import re
import subprocess

from mpc_amd import engine
from tests.util import kernel_constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = """
int gc_kos_multi_receiver_tags(gc_ctx *, const gc_label *seed2, const gc_label *result, const uint8_t *b, const gc_label *choice_vec, const uint8_t *bcv, size_t S, size_t per, gc_label *tags_out);
int gc_kos_multi_receiver_tags_dev(gc_ctx *, const void *d_seed2, const void *d_result, const void *d_choice_packed, const void *d_choice_vec, const void *d_bcv_packed, size_t S, size_t per, void *d_tags_out);
int gc_kos_multi_sender_check(gc_ctx *, const gc_label *seed2, const gc_label *result, const gc_label *choice_vec, const gc_label *delta, const gc_label *tags, size_t S, size_t per, uint8_t *ok_out, size_t *bad_session);
int gc_kos_multi_sender_check_dev(gc_ctx *, const void *d_seed2, const void *d_result, const void *d_choice_vec, const void *d_delta, const void *d_tags, size_t S, size_t per, void *d_ok, void *d_status);
"""


def squeeze(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def new_names():
    return re.findall(r"\b(gc_kos_multi[a-z_]*)\(", PROTOTYPES)


def test_the_prototypes_are_in_the_header():
    header = squeeze(open(engine.HEADER).read())
    protos = PROTOTYPES.strip().splitlines()
    assert len(protos) == 4 == len(set(new_names()))
    for p in protos:
        assert squeeze(p) in header, p


def test_the_header_no_longer_sends_callers_to_the_one_session_check():
    text = re.sub(r"\s+", " ", open(engine.HEADER).read().replace(" * ", " "))
    assert "a KOS check over the handle are not offered" not in text
    assert "gc_kos_*_dev runs per session on slices" not in text


def test_the_library_exports_them_and_the_abi_version_stays():
    L = engine.lib()
    for n in new_names():
        assert hasattr(L, n), "libgcengine.so does not export %s" % n
    assert L.gc_abi_version() == engine.ABI_VERSION == 2
    assert "#define GC_ABI_VERSION 2" in squeeze(open(engine.HEADER).read())


def test_the_header_still_compiles_as_c99(tmp_path):
    src = tmp_path / "kos_multi_abi.c"
    body = ['#include "gcengine.h"', "typedef void (*fn)(void);", "fn table[] = {"]
    body += ["    (fn)%s," % n for n in new_names()]
    body += ["};", "int main(void) { return sizeof table == 0; }"]
    src.write_text("\n".join(body) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-Wno-cast-function-type",
                        "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "kos_multi_abi.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_and_zero_arguments_are_refused_without_a_gpu():
    """the checks that come before anything touches a device"""
    L, E = engine.lib(), engine.GC_E_ARG
    assert L.gc_kos_multi_receiver_tags(None, None, None, None, None, None, 3, 128, None) == E
    assert L.gc_kos_multi_receiver_tags_dev(None, None, None, None, None, None, 3, 128, None) == E
    assert L.gc_kos_multi_sender_check(None, None, None, None, None, None, 3, 128, None, None) == E
    assert L.gc_kos_multi_sender_check_dev(None, None, None, None, None, None, 3, 128, None, None) == E
    assert L.gc_kos_multi_receiver_tags_dev(None, None, None, None, None, None, 0, 0, None) == E  # a NULL ctx, whatever S is
    bad = C.c_size_t(7)
    assert L.gc_kos_multi_sender_check(None, None, None, None, None, None, 0, 128, None, C.byref(bad)) == E and bad.value == 7


def test_the_launch_shape_is_a_set_of_kernel_constants():
    threads, grid, wave_max = kernel_constants("kKosMultiThreads", "kKosMultiGrid", "kKosMultiWaveMax")
    assert threads == 1024 and grid >= 1
    assert wave_max >= 256 + 128, "a session of 128 OTs and its choice vector is one wave's work"
