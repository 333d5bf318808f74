"""GPU tests of the packed-IKNP VOLE kernels (gc_vole_*, mpc_amd/csrc/vole_kernels.hip) against the plain-Python restatement
of vole/vole.go (tests/py_vole_reference.py): byte parity of the host and device forms for thirteen moduli from 3 to
2^256 - 1 at ragged sizes, with hostile values (>= p, 2^256 - 1) in x, y and the u-message and all-zero / all-ones labels;
the VOLE relation for every element at 2^21 + 3; the whole Mul of both sides from the device IKNP in HBM; the in-place
receiver; misuse."""
import ctypes as C

import numpy as np
import pytest

import oracle
from mpc_amd import engine
from mpc_amd.circuit import LABEL
from tests import py_vole_reference as vole
from tests.test_gpu_ot import base_setup
from tests.test_vole_mod import MODULI, REFUSED
from tests.util import drbg

pytestmark = pytest.mark.gpu

TOP = 1 << 256
P256 = vole.P256
SIZES = [0, 1, 20, 63, 64, 65, 255, 256, 257, 1024, 65537]
NLAB = max(SIZES)


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


def oracle_pad(label):
    key = label[0].to_bytes(8, "big") + label[1].to_bytes(8, "big")
    return oracle.aes_encrypt(key, bytes(16)) + oracle.aes_encrypt(key, bytes(15) + b"\x01")


def make_labels(seed, n):
    """n seeded labels, all-zero and all-ones ones among them (first, second, and around the sizes' edges)"""
    raw = np.frombuffer(drbg(seed, 16 * n), np.uint64).reshape(n, 2)
    lab = np.zeros(n, LABEL)
    lab["d0"], lab["d1"] = raw[:, 0], raw[:, 1]
    for k, i in enumerate([0, 1, 62, 63, 64, 255, 256, 1023, n - 2, n - 1]):
        if 0 <= i < n:
            lab[i] = (0, 0) if k % 2 == 0 else (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF)
    return lab


def as_tuples(lab):
    return [(int(a), int(b)) for a, b in zip(lab["d0"], lab["d1"])]


@pytest.fixture(scope="module")
def label_set():
    """the labels and their pads, once (pads do not depend on p): the oracle's AES, cross-checked with the Python AES on
    the first 256"""
    lab = make_labels("vole/labels", NLAB)
    tl = as_tuples(lab)
    pads = [oracle_pad(l) for l in tl]
    for i in range(256):
        assert vole.label_pad(tl[i]) == pads[i], i
    return lab, pads


def edge_values(p):
    e = [0, 1, p - 1, p, p + 1, TOP - 1, 2 * p, TOP - p, TOP - 1 - (TOP - 1) % p,
         int.from_bytes(b"\xff" * 16 + bytes(16), "big"), int.from_bytes(bytes(16) + b"\xff" * 16, "big"),
         int.from_bytes(b"\xff\x00" * 16, "big"), int.from_bytes(b"\x00\xff" * 16, "big")]
    return [v for v in e if 0 <= v < TOP]


def column(p, m, seed, rot=0):
    """m values below 2^256: the edge values at the front and the back (rotated by rot, so x, y and u meet different
    pairs), seeded uniform values between, every third one reduced below p"""
    raw = np.random.default_rng(list(drbg("%s/%d/%d" % (seed, p % 1000003, m), 8))).integers(0, 256, (m, 32), dtype=np.uint8)
    vals = [int.from_bytes(raw[i].tobytes(), "big") for i in range(m)]
    for i in range(0, m, 3):
        vals[i] %= p
    e = edge_values(p)
    e = e[rot % len(e):] + e[:rot % len(e)]
    for k, v in enumerate(e):
        if k < m:
            vals[k] = v
        if m - 1 - k > len(e):
            vals[m - 1 - k] = v
    return vals


def to_arr(vals):
    return np.frombuffer(b"".join(v.to_bytes(32, "big") for v in vals), np.uint8).reshape(len(vals), 32)


def b32(vals):
    return b"".join(vole.bytes32(v) for v in vals)


@pytest.mark.parametrize("p", MODULI, ids=lambda p: "%d_bits" % p.bit_length())
def test_byte_parity_host_and_dev(ctx, label_set, p):
    lab_all, pads_all = label_set
    for m in SIZES:
        lab, pads = lab_all[:m], pads_all[:m]
        xs, ys, us_in = column(p, m, "x"), column(p, m, "y", 5), column(p, m, "u", 9)
        x, y, u_in = to_arr(xs), to_arr(ys), to_arr(us_in)
        rs, u_msg = vole.sender_mul(pads, xs, y.tobytes(), p)
        us = vole.receiver_reduce(u_in.tobytes(), m, p)
        what = "p %#x m %d" % (p, m)
        # host forms
        r_h, u_h = engine.vole_sender_mul(ctx, p, lab, x, y)
        assert r_h.tobytes() == b32(rs), what
        assert u_h.tobytes() == u_msg, what
        assert engine.vole_receiver_reduce(ctx, p, u_in).tobytes() == b32(us), what
        # device forms
        d_lab, d_x, d_y, d_u = ctx.to_device(lab), ctx.to_device(x), ctx.to_device(y), ctx.to_device(u_in)
        d_r, d_um, d_us = ctx.zeros((m, 32)), ctx.zeros((m, 32)), ctx.zeros((m, 32))
        engine.vole_sender_mul_dev(ctx, p, d_lab, d_x, d_y, m, d_r, d_um)
        engine.vole_receiver_reduce_dev(ctx, p, d_u, m, d_us)
        ctx.sync()
        assert d_r.numpy().tobytes() == b32(rs), what
        assert d_um.numpy().tobytes() == u_msg, what
        assert d_us.numpy().tobytes() == b32(us), what
        assert d_u.numpy().tobytes() == u_in.tobytes(), what  # the input is not written
        for d in (d_lab, d_x, d_y, d_u, d_r, d_um, d_us):
            d.close()


def test_relation_for_every_element_past_2_21(ctx):
    """m = 2^21 + 3 (grid-stride loop, many passes per lane): u - r == x * y mod p for every element, r and u below p,
    the receiver's reduction of u is u; byte parity at 4 096 seeded indices, the first and last 16 among them"""
    m, p = (1 << 21) + 3, P256
    lab = make_labels("vole/big", m)
    rng = np.random.default_rng(2021)
    x = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    y = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    x[-1], y[-1], y[0] = 0xFF, 0xFF, 0xFF
    d_lab, d_x, d_y = ctx.to_device(lab), ctx.to_device(x), ctx.to_device(y)
    d_r, d_u, d_us = ctx.zeros((m, 32)), ctx.zeros((m, 32)), ctx.zeros((m, 32))
    engine.vole_sender_mul_dev(ctx, p, d_lab, d_x, d_y, m, d_r, d_u)
    engine.vole_receiver_reduce_dev(ctx, p, d_u, m, d_us)
    ctx.sync()
    rb, ub, usb = d_r.numpy().tobytes(), d_u.numpy().tobytes(), d_us.numpy().tobytes()
    assert usb == ub
    xb, yb = x.tobytes(), y.tobytes()
    fb = int.from_bytes
    bad = []
    for i in range(m):
        s = slice(32 * i, 32 * i + 32)
        r, u = fb(rb[s], "big"), fb(ub[s], "big")
        if r >= p or u >= p or (u - r - fb(xb[s], "big") * fb(yb[s], "big")) % p:
            bad.append(i)
            if len(bad) > 8:
                break
    assert not bad, bad
    idx = sorted(set(range(16)) | set(range(m - 16, m)) | set(np.random.default_rng(7).integers(0, m, 4096 - 32).tolist()))
    tl = as_tuples(lab[idx])
    rs, u_msg = vole.sender_mul([oracle_pad(l) for l in tl], [fb(x[i].tobytes(), "big") for i in idx], y[idx].tobytes(), p)
    got_r = b"".join(rb[32 * i:32 * i + 32] for i in idx)
    got_u = b"".join(ub[32 * i:32 * i + 32] for i in idx)
    assert got_r == b32(rs) and got_u == u_msg
    for d in (d_lab, d_x, d_y, d_r, d_u, d_us):
        d.close()


@pytest.mark.parametrize("m", [20, 1024])
def test_end_to_end_from_device_iknp(ctx, m):
    """the whole Mul of both sides in HBM: gc_iknp_receive_dev with all-false choices, gc_iknp_send_dev, then the two VOLE
    calls on the labels where they are — byte for byte the restatement's Mul on the Python IKNP, and the relation holds"""
    p = P256
    base, delta, k0 = base_setup("vole-e2e-%d" % m)
    xs, ys = column(p, m, "e2e-x"), column(p, m, "e2e-y", 3)
    rx, tx = engine.IKNPReceiver(ctx, base), engine.IKNPSender(ctx, delta, k0)
    chunks = (m + 511) // 512
    d_c, d_iu = ctx.zeros(chunks * 64), ctx.zeros(chunks * 8192)
    d_lr, d_ls = ctx.zeros((m, 16)), ctx.zeros((m, 16))
    y_msg = b32(ys)
    d_x, d_y = ctx.to_device(to_arr(xs)), ctx.to_device(y_msg)
    d_r, d_um, d_us = ctx.zeros((m, 32)), ctx.zeros((m, 32)), ctx.zeros((m, 32))
    rx.receive_dev(d_c, m, d_iu, d_lr)
    tx.send_dev(d_iu, m, d_ls)
    engine.vole_sender_mul_dev(ctx, p, d_ls, d_x, d_y, m, d_r, d_um)
    engine.vole_receiver_reduce_dev(ctx, p, d_um, m, d_us)
    ctx.sync()
    bt = [((int(w["l0"]["d0"]), int(w["l0"]["d1"])), (int(w["l1"]["d0"]), int(w["l1"]["d1"]))) for w in base]
    ref = vole.mul(xs, ys, p, bt, delta, as_tuples(k0))
    assert d_iu.numpy()[:len(ref["u"])].tobytes() == ref["u"]
    assert as_tuples(d_ls.download(LABEL, (m,))) == ref["labels_s"]
    assert as_tuples(d_lr.download(LABEL, (m,))) == ref["labels_r"] == ref["labels_s"]
    assert d_r.numpy().tobytes() == b32(ref["rs"])
    assert d_um.numpy().tobytes() == ref["u_msg"]
    assert d_us.numpy().tobytes() == b32(ref["us"])
    for i in range(m):
        assert (ref["us"][i] - ref["rs"][i]) % p == xs[i] * ys[i] % p, i
    rx.close()
    tx.close()


@pytest.mark.parametrize("p", [3, (1 << 127) - 1, P256, (1 << 256) - 1], ids=lambda p: "%d_bits" % p.bit_length())
def test_receiver_in_place(ctx, p):
    for m in (1, 257, 65537):
        us_in = column(p, m, "inplace")
        u = to_arr(us_in)
        d = ctx.to_device(u)
        engine.vole_receiver_reduce_dev(ctx, p, d, m, d)
        ctx.sync()
        assert d.numpy().tobytes() == b32(vole.receiver_reduce(u.tobytes(), m, p)), m
        d.close()


def _vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.ptr)


def test_misuse(ctx):
    L = engine.lib()
    m = 4
    lab, x, y = make_labels("vole/misuse", m), np.ones((m, 32), np.uint8), np.ones((m, 32), np.uint8)
    r, u = np.zeros((m, 32), np.uint8), np.zeros((m, 32), np.uint8)
    d_lab, d_x, d_y, d_r, d_u = ctx.to_device(lab), ctx.to_device(x), ctx.to_device(y), ctx.zeros((m, 32)), ctx.zeros((m, 32))
    good = engine.vole_modulus(P256)
    # refused moduli: every form, before any launch
    for bad in REFUSED:
        pb = engine.vole_modulus(bad)
        assert L.gc_vole_sender_mul(ctx.h, _vp(pb), _vp(lab), _vp(x), _vp(y), m, _vp(r), _vp(u)) == engine.GC_E_ARG, bad
        assert L.gc_vole_sender_mul_dev(ctx.h, _vp(pb), _vp(d_lab), _vp(d_x), _vp(d_y), m, _vp(d_r), _vp(d_u)) == engine.GC_E_ARG
        assert L.gc_vole_receiver_reduce(ctx.h, _vp(pb), _vp(u), m, _vp(r)) == engine.GC_E_ARG
        assert L.gc_vole_receiver_reduce_dev(ctx.h, _vp(pb), _vp(d_u), m, _vp(d_r)) == engine.GC_E_ARG
        with pytest.raises(engine.EngineError) as e:
            engine.vole_sender_mul(ctx, bad, lab, x, y)
        assert e.value.code == engine.GC_E_ARG
        with pytest.raises(engine.EngineError) as e:
            engine.vole_receiver_reduce(ctx, bad, u)
        assert e.value.code == engine.GC_E_ARG
    assert not r.any() and not u.any()
    for big in (1 << 256, (1 << 256) + 1, -3):  # does not fit 32 bytes
        with pytest.raises(engine.EngineError) as e:
            engine.vole_sender_mul(ctx, big, lab, x, y)
        assert e.value.code == engine.GC_E_ARG
    # NULL pointers with m > 0
    args = [_vp(good), _vp(lab), _vp(x), _vp(y), m, _vp(r), _vp(u)]
    dargs = [_vp(good), _vp(d_lab), _vp(d_x), _vp(d_y), m, _vp(d_r), _vp(d_u)]
    for k in (0, 1, 2, 3, 5, 6):
        a, da = list(args), list(dargs)
        a[k] = da[k] = None
        assert L.gc_vole_sender_mul(ctx.h, *a) == engine.GC_E_ARG, k
        assert L.gc_vole_sender_mul_dev(ctx.h, *da) == engine.GC_E_ARG, k
    assert L.gc_vole_sender_mul(None, *args) == engine.GC_E_ARG
    rargs, rdargs = [_vp(good), _vp(u), m, _vp(r)], [_vp(good), _vp(d_u), m, _vp(d_r)]
    for k in (0, 1, 3):
        a, da = list(rargs), list(rdargs)
        a[k] = da[k] = None
        assert L.gc_vole_receiver_reduce(ctx.h, *a) == engine.GC_E_ARG, k
        assert L.gc_vole_receiver_reduce_dev(ctx.h, *da) == engine.GC_E_ARG, k
    assert L.gc_vole_receiver_reduce_dev(None, *rdargs) == engine.GC_E_ARG
    # m = 0: GC_OK, nothing written (NULL data pointers allowed)
    r[:] = 0xAB
    d_r.zero(0xAB)
    assert L.gc_vole_sender_mul(ctx.h, _vp(good), None, None, None, 0, None, None) == engine.GC_OK
    assert L.gc_vole_sender_mul(ctx.h, _vp(good), _vp(lab), _vp(x), _vp(y), 0, _vp(r), _vp(u)) == engine.GC_OK
    assert L.gc_vole_sender_mul_dev(ctx.h, _vp(good), _vp(d_lab), _vp(d_x), _vp(d_y), 0, _vp(d_r), _vp(d_u)) == engine.GC_OK
    assert L.gc_vole_receiver_reduce(ctx.h, _vp(good), _vp(u), 0, _vp(r)) == engine.GC_OK
    assert L.gc_vole_receiver_reduce_dev(ctx.h, _vp(good), None, 0, None) == engine.GC_OK
    assert L.gc_vole_receiver_reduce_dev(ctx.h, _vp(good), _vp(d_u), 0, _vp(d_r)) == engine.GC_OK
    ctx.sync()
    assert (r == 0xAB).all() and not u.any()
    assert (d_r.numpy() == 0xAB).all()
    for d in (d_lab, d_x, d_y, d_r, d_u):
        d.close()
