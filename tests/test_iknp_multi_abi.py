"""The multi-session IKNP / COT entry points (gc_iknp_multi_*, gc_cot_multi_*) are in include/gcengine.h with the agreed
prototypes, libgcengine.so exports them, the header is still plain C99, the ABI version has not moved, and the grid cap the
GPU tests size themselves from is where tests.util.kernel_constants looks.  No GPU needed."""
import os
import re
import subprocess

from mpc_amd import engine
from tests.util import kernel_constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = """
gc_iknp_multi *gc_iknp_multi_sender_create(gc_ctx *, const gc_label *delta, const gc_label *k0, size_t S, int *status);
gc_iknp_multi *gc_iknp_multi_sender_create_dev(gc_ctx *, const void *d_delta, const void *d_k0, size_t S, int *status);
gc_iknp_multi *gc_iknp_multi_receiver_create(gc_ctx *, const gc_wire *base, size_t S, int *status);
gc_iknp_multi *gc_iknp_multi_receiver_create_dev(gc_ctx *, const void *d_base, size_t S, int *status);
void gc_iknp_multi_free(gc_iknp_multi *);
int gc_iknp_multi_info(const gc_iknp_multi *, size_t *S, int *receiver, uint64_t *pos);
int gc_iknp_multi_receive(gc_iknp_multi *, const uint8_t *choice, size_t per, uint8_t *u_out, gc_label *labels_out);
int gc_iknp_multi_send(gc_iknp_multi *, const uint8_t *u_in, size_t u_len, size_t per, gc_label *labels_out);
int gc_iknp_multi_receive_dev(gc_iknp_multi *, const void *d_choice_packed, size_t per, void *d_u_out, void *d_labels_out);
int gc_iknp_multi_send_dev(gc_iknp_multi *, const void *d_u_in, size_t per, void *d_labels_out);
int gc_cot_multi_send_pads(gc_ctx *, const gc_label *seed, const gc_label *delta, const gc_label *data, const gc_wire *wires, size_t S, size_t per, gc_label *out);
int gc_cot_multi_send_pads_dev(gc_ctx *, const void *d_seed, const void *d_delta, const void *d_data, const void *d_wires, size_t S, size_t per, void *d_out);
int gc_cot_multi_receive_unpad(gc_ctx *, const gc_label *seed, const uint8_t *flags, const gc_label *sent, gc_label *result, size_t S, size_t per);
int gc_cot_multi_receive_unpad_dev(gc_ctx *, const void *d_seed, const void *d_flags, const void *d_sent, void *d_result, size_t S, size_t per);
"""


def squeeze(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def new_names():
    return re.findall(r"\b(gc_[a-z_]+multi[a-z_]*)\(", PROTOTYPES)


def test_the_prototypes_are_in_the_header():
    header = squeeze(open(engine.HEADER).read())
    assert "typedef struct gc_iknp_multi gc_iknp_multi;" in header
    protos = [p for p in PROTOTYPES.strip().splitlines()]
    assert len(protos) == 14 == len(set(new_names()))
    for p in protos:
        assert squeeze(p) in header, p


def test_the_library_exports_them_and_the_abi_version_stays():
    L = engine.lib()
    for n in new_names():
        assert hasattr(L, n), "libgcengine.so does not export %s" % n
    assert L.gc_abi_version() == engine.ABI_VERSION == 2
    assert "#define GC_ABI_VERSION 2" in squeeze(open(engine.HEADER).read())


def test_the_header_still_compiles_as_c99(tmp_path):
    src = tmp_path / "iknp_multi_abi.c"
    body = ['#include "gcengine.h"', "typedef void (*fn)(void);", "fn table[] = {"]
    body += ["    (fn)%s," % n for n in new_names()]
    body += ["};", "int main(void) { return sizeof table == 0; }"]
    src.write_text("\n".join(body) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-Wno-cast-function-type",
                        "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "iknp_multi_abi.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_and_zero_arguments_are_refused_without_a_gpu():
    """the checks that come before anything touches a device"""
    L = engine.lib()
    import ctypes as C
    st = C.c_int(0)
    assert not L.gc_iknp_multi_sender_create(None, None, None, 3, C.byref(st)) and st.value == engine.GC_E_ARG
    assert not L.gc_iknp_multi_receiver_create_dev(None, None, 0, C.byref(st)) and st.value == engine.GC_E_ARG
    assert L.gc_iknp_multi_info(None, None, None, None) == engine.GC_E_ARG
    assert L.gc_iknp_multi_receive_dev(None, None, 128, None, None) == engine.GC_E_ARG
    assert L.gc_iknp_multi_send(None, None, 0, 128, None) == engine.GC_E_ARG
    assert L.gc_cot_multi_send_pads_dev(None, None, None, None, None, 3, 128, None) == engine.GC_E_ARG
    assert L.gc_cot_multi_receive_unpad(None, None, None, None, None, 3, 128) == engine.GC_E_ARG
    L.gc_iknp_multi_free(None)  # a no-op


def test_the_grid_cap_is_a_kernel_constant():
    grid, threads = kernel_constants("kIknpMultiGrid", "kIknpThreads")
    assert grid >= 1 and threads == 1024
