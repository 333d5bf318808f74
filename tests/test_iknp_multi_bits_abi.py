"""The bit-COT entry points of the multi-session IKNP handle and the triple folds over S peers (gc_iknp_multi_*_bits*,
gc_gmw_triples_multi_*) are in include/gcengine.h with the agreed prototypes, libgcengine.so exports them, the ctypes table
of mpc_amd.engine has them with matching parameter kinds, the Go shims call them with the right arity, the header is still
plain C99, the ABI version has not moved, NULL arguments are refused before any device is touched, and the launch shapes the
GPU tests size themselves from are where tests.util.kernel_constants looks.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

from mpc_amd import engine
from tests.test_abi_plan import _go_calls, _prototypes
from tests.util import kernel_constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = """
int gc_iknp_multi_receive_bits_dev(gc_iknp_multi *, const void *d_choices, size_t choice_stride, size_t per, void *d_u_out, void *d_result);
int gc_iknp_multi_send_bits_dev(gc_iknp_multi *, const void *d_u_in, size_t per, void *d_result);
int gc_iknp_multi_receive_bits(gc_iknp_multi *, const uint64_t *choices, size_t choice_stride, size_t per, uint8_t *u_out, uint64_t *result);
int gc_iknp_multi_send_bits(gc_iknp_multi *, const uint8_t *u_in, size_t u_len, size_t per, uint64_t *result);
int gc_gmw_triples_multi_sender_u_dev(gc_iknp_multi *sender, const void *d_a, void *d_u, size_t words);
int gc_gmw_triples_multi_sender_fold_dev(gc_ctx *, const void *d_s, const void *d_u, const void *d_v, void *d_c, size_t S, size_t words);
int gc_gmw_triples_multi_receiver_fold_dev(gc_ctx *, const void *d_r, void *d_c, size_t S, size_t words);
"""


def squeeze(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def new_names():
    return re.findall(r"\b(gc_[a-z_]+multi[a-z_]*)\(", PROTOTYPES)


def test_the_prototypes_are_in_the_header():
    header = squeeze(open(engine.HEADER).read())
    protos = PROTOTYPES.strip().splitlines()
    assert len(protos) == 7 == len(set(new_names()))
    for p in protos:
        assert squeeze(p) in header, p


def test_the_header_no_longer_says_bit_cot_is_not_offered():
    text = re.sub(r"\s+", " ", open(engine.HEADER).read().replace(" * ", " "))
    assert "bit-COT and ROT are not offered" not in text
    assert "ROT are not offered" in text, "ROT over the multi handle is still not built"


def test_the_library_exports_them_and_the_abi_version_stays():
    L = engine.lib()
    for n in new_names():
        assert hasattr(L, n), "libgcengine.so does not export %s" % n
    assert L.gc_abi_version() == engine.ABI_VERSION == 2
    assert "#define GC_ABI_VERSION 2" in squeeze(open(engine.HEADER).read())


def test_the_ctypes_table_agrees_with_the_prototypes():
    """every new function is in the table engine.lib() applies, returns int, and takes a pointer where the header has a
    pointer and a size_t where it has a scalar"""
    L, protos = engine.lib(), _prototypes()
    for n in new_names():
        f = getattr(L, n)
        assert f.restype is C.c_int32 or f.restype is C.c_int, (n, f.restype)
        kinds = ["ptr" if a is C.c_void_p else "scalar" for a in f.argtypes]
        assert kinds == protos[n], (n, kinds, protos[n])
        assert all(a is C.c_size_t for a, k in zip(f.argtypes, kinds) if k == "scalar"), n


def test_the_go_shims_call_them_with_the_right_arity():
    """go/ is source only: the multi IKNP shim has ReceiveBits / SendBits, the GMW shim the batch over all peers, and between
    them they call every new entry point with as many arguments as its prototype has"""
    protos, called = _prototypes(), {}
    for rel in ("go/ot/iknp_multi_hip.go", "go/gmw/triples_hip.go"):
        text = open(os.path.join(ROOT, rel)).read()
        for name, args in _go_calls(text):
            if name in new_names():
                assert len(args) == len(protos[name]), (rel, name, args)
                called.setdefault(name, rel)
    assert sorted(called) == sorted(new_names()), sorted(set(new_names()) - set(called))
    ot = open(os.path.join(ROOT, "go", "ot", "iknp_multi_hip.go")).read()
    assert "func (m *hipIKNPMulti) ReceiveBits(" in ot and "func (m *hipIKNPMulti) SendBits(" in ot
    assert "func tripleBatchMulti(" in open(os.path.join(ROOT, "go", "gmw", "triples_hip.go")).read()


def test_the_header_still_compiles_as_c99(tmp_path):
    src = tmp_path / "iknp_multi_bits_abi.c"
    body = ['#include "gcengine.h"', "typedef void (*fn)(void);", "fn table[] = {"]
    body += ["    (fn)%s," % n for n in new_names()]
    body += ["};", "int main(void) { return sizeof table == 0; }"]
    src.write_text("\n".join(body) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-Wno-cast-function-type",
                        "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "iknp_multi_bits_abi.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_arguments_are_refused_without_a_gpu():
    """the checks that come before anything touches a device"""
    L, E = engine.lib(), engine.GC_E_ARG
    assert L.gc_iknp_multi_receive_bits_dev(None, None, 0, 128, None, None) == E
    assert L.gc_iknp_multi_send_bits_dev(None, None, 128, None) == E
    assert L.gc_iknp_multi_receive_bits(None, None, 0, 128, None, None) == E
    assert L.gc_iknp_multi_send_bits(None, None, 0, 128, None) == E
    assert L.gc_iknp_multi_receive_bits_dev(None, None, 0, 0, None, None) == E  # a NULL handle, whatever per is
    assert L.gc_gmw_triples_multi_sender_u_dev(None, None, None, 4) == E
    assert L.gc_gmw_triples_multi_sender_fold_dev(None, None, None, None, None, 3, 4) == E
    assert L.gc_gmw_triples_multi_receiver_fold_dev(None, None, None, 3, 4) == E


def test_the_launch_shapes_are_kernel_constants():
    threads, grid, fthreads, fgrid = kernel_constants("kIknpBitsSendThreads", "kIknpBitsSendGrid", "kGmwMultiFoldThreads",
                                                      "kGmwMultiFoldGrid")
    assert threads % 64 == 0 and fthreads % 64 == 0 and grid >= 1 and fgrid >= 1
