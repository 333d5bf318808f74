"""The Chou-Orlandi receiver behind a session handle (gc_co_base_*, mpc_amd/csrc/co_base_kernels.hip, co_table.h): b * G and
b * A summed from fixed-base window tables instead of walked by the ladder.  Byte parity with the restated reference on the
pool of tests/test_gpu_co.py (its expected values are computed once per module), every OT of more than one grid sweep against
the ladder calls on the same device buffers, coordinates with leading zero bytes, Go's round constants, several handles on
one ctx, the hand-over to IKNP, and misuse."""
import ctypes as C

import numpy as np
import pytest

import oracle
from mpc_amd import engine
from mpc_amd.circuit import LABEL, WIRE
from tests import go_transcript as gt
from tests import py_co_reference as co
from tests.test_gpu_co import (HOSTILE, ID0S, SIZES, ct_bytes, expected_ct, expected_labels, label_raw, labels_from_bytes,
                               masks_xor, pick, points_array, scalars_array)
from tests.test_gpu_co import pool  # noqa: F401  (the module-scoped fixture: one session, 257 OTs with the edge scalars)
from tests.test_py_co_reference import go_session, round2_hash
from tests.util import drbg, kernel_constants

pytestmark = pytest.mark.gpu

TAB_THREADS, TAB_GRID = kernel_constants("kCoTabThreads", "kCoTabGrid")
TAB_SWEEP = TAB_GRID * TAB_THREADS
N_TAB = TAB_SWEEP + TAB_THREADS + 37  # the second trip has a full workgroup and one with 37 live lanes
TOP = 1 << 256
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def base(ctx, pool):  # noqa: F811
    b = engine.CoBase(ctx, co.point_bytes(pool["A"]))
    yield b
    b.close()


def run_host(ctx, base, pool, n, id0, cts):  # noqa: F811
    sc, ch = scalars_array(pool["scalars"][:n]), pool["choice"][:n]
    pts = base.choices(sc, ch)
    labels = base.decrypt(sc, ch, np.frombuffer(b"".join(cts), np.uint8), id0)
    return pts, labels


def run_dev(ctx, base, pool, n, id0, cts):  # noqa: F811
    m = max(n, 1)
    d_sc = ctx.to_device(scalars_array(pool["scalars"][:m]))
    d_ch = ctx.to_device(pool["choice"][:m].copy())
    d_ct = ctx.to_device(np.frombuffer(b"".join(cts) if n else bytes(32), np.uint8).copy())
    d_pts, d_lab = ctx.empty((m, 64)).zero(SENTINEL), ctx.empty((m, 16)).zero(SENTINEL)
    base.choices_dev(d_sc, d_ch, n, d_pts)
    base.decrypt_dev(d_sc, d_ch, d_ct, n, id0, d_lab)
    ctx.sync()
    pts, lab = d_pts.numpy(), d_lab.numpy()
    if n == 0:  # nothing written
        assert (pts == SENTINEL).all() and (lab == SENTINEL).all()
        return pts[:0], np.zeros(0, LABEL)
    return pts, np.frombuffer(lab.tobytes(), LABEL)


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("id0", ID0S)
@pytest.mark.parametrize("n", SIZES)
def test_byte_parity(ctx, base, pool, n, id0, form):  # noqa: F811
    cts = expected_ct(pool, n, id0)  # the sender's bytes for these OTs (32 zero bytes where the receiver sent infinity)
    pts, labels = (run_host if form == "host" else run_dev)(ctx, base, pool, n, id0, cts)
    assert len(pts) == n and len(labels) == n
    assert [bytes(p) for p in pts] == [co.point_bytes(p) for p in pool["B"][:n]], "choice points differ"
    assert label_raw(labels) == expected_labels(pool, n, id0, cts), "decrypted labels differ"
    for i in range(n):  # decrypt(encrypt) = L_choice
        if i not in pool["infinite"]:
            assert label_raw(labels[i:i + 1])[0] == pool["pairs"][i][pool["choice"][i]], i
    if n >= 63:  # b = 0 mod N: infinity without the choice, A itself with it
        assert not pts[52].any() and bytes(pts[3]) == bytes(pts[24]) == co.point_bytes(pool["A"])


def test_host_form_leaves_outputs_alone_at_zero(base):
    L, p = engine.lib(), engine._p
    sc, ch, ct = np.zeros((1, 32), np.uint8), np.zeros(1, np.uint8), np.zeros((1, 32), np.uint8)
    out_pts, out_lab = np.full((1, 64), SENTINEL, np.uint8), np.full(16, SENTINEL, np.uint8)
    assert L.gc_co_base_choices(base.h, p(sc), p(ch), 0, p(out_pts)) == engine.GC_OK
    assert L.gc_co_base_decrypt(base.h, p(sc), p(ch), p(ct), 0, 9, p(out_lab)) == engine.GC_OK
    assert (out_pts == SENTINEL).all() and (out_lab == SENTINEL).all()
    assert len(base.choices([], [])) == 0 and len(base.decrypt([], [], np.zeros(0, np.uint8), 3)) == 0


def test_past_one_grid_sweep(ctx):
    """N_TAB OTs through the device-pointer forms: every lane of the first TAB_THREADS + 37 makes a second trip of its
    grid-stride loop.  Points and labels equal the ladder calls' outputs on the same device buffers for every OT; slices of
    the scalars are forced to all-zero windows, all-ones windows and values at and above N, on both sides of the sweep edge."""
    n, id0 = N_TAB, (1 << 32) - 7  # the id carries into its high word at OT 7
    assert n > TAB_SWEEP + TAB_THREADS and (n - TAB_SWEEP) % TAB_THREADS != 0
    rng = np.random.default_rng(20241017)
    a = int.from_bytes(drbg("co_base/sweep/a", 32), "big")
    A, _ = co.sender_setup(a)
    Ab = co.point_bytes(A)
    scalars = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    forced = {}
    for lo in (100, TAB_SWEEP - 300, TAB_SWEEP + 5, n - 250):
        for k in range(64):  # one non-zero window (every other one zero), then its complement: one zero window among all-ones
            forced[lo + k] = 1 << (4 * k) if k < 63 else 7 << 252
            forced[lo + 64 + k] = (co.N - 1) & ~(15 << (4 * k))
        edge = [0, co.N, co.N + 1, TOP - 1, co.N - 1, 1, co.N + (1 << 200) + 12345, (1 << 255) - 1, 15 << 252]
        for k, v in enumerate(edge):
            forced[lo + 128 + k] = v
        for k in range(32):  # at and above N with random low halves
            forced[lo + 140 + k] = co.N + int.from_bytes(bytes(scalars[lo + 140 + k][8:]), "big")
    for at, v in forced.items():
        assert 0 <= v < TOP and 0 <= at < n
        scalars[at] = np.frombuffer(v.to_bytes(32, "big"), np.uint8)
    assert sum(1 for v in forced.values() if v >= co.N) > 100
    choice = rng.integers(0, 2, n).astype(np.uint8)
    ct = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d_sc, d_ch, d_ct = ctx.to_device(scalars), ctx.to_device(choice), ctx.to_device(ct)
    d_pts, d_lab = ctx.empty((n, 64)).zero(SENTINEL), ctx.empty((n, 16)).zero(SENTINEL)
    d_pts_ref, d_lab_ref = ctx.empty((n, 64)).zero(0x5A), ctx.empty((n, 16)).zero(0x5A)
    base = engine.CoBase(ctx, Ab)
    base.choices_dev(d_sc, d_ch, n, d_pts)
    base.decrypt_dev(d_sc, d_ch, d_ct, n, id0, d_lab)
    engine.co_receiver_choices_dev(ctx, Ab, d_sc, d_ch, n, d_pts_ref)
    engine.co_receiver_decrypt_dev(ctx, Ab, d_sc, d_ch, d_ct, n, id0, d_lab_ref)
    ctx.sync()
    base.close()
    pts, pts_ref, lab, lab_ref = d_pts.numpy(), d_pts_ref.numpy(), d_lab.numpy(), d_lab_ref.numpy()
    bad = np.flatnonzero((pts != pts_ref).any(axis=1))
    assert bad.size == 0, "choice points differ from the ladder's at %d OTs, the first %d" % (bad.size, bad[0])
    bad = np.flatnonzero((lab != lab_ref).any(axis=1))
    assert bad.size == 0, "labels differ from the ladder's at %d OTs, the first %d" % (bad.size, bad[0])
    # and the ladder's bytes are the restatement's: a few of the forced scalars on each side of the edge, the id past 2^32
    for i in (0, 7, 100, 163, 100 + 128, 100 + 129, TAB_SWEEP + 5 + 131, n - 250 + 140, n - 1):
        b, c = int.from_bytes(bytes(scalars[i]), "big"), int(choice[i])
        assert bytes(pts[i]) == co.point_bytes(co.receiver_choices(A, [b], [c])[0]), "choice point %d" % i
        want = masks_xor(co.mul(A, b), id0 + i, bytes(ct[i][16:] if c else ct[i][:16]))
        assert label_raw(np.frombuffer(lab[i].tobytes(), LABEL)) == [want], "label %d" % i


def test_short_coordinates(ctx):
    """b * A whose coordinates have leading zero bytes: deriveMask hashes x.Bytes() and y.Bytes(), not 32 bytes each"""
    A, _ = co.sender_setup(co.SHORT_A_SCALAR)
    ks = sorted(co.SHORT_MULTIPLES)
    short = {k: co.mul(A, k) for k in ks}
    for k in ks:
        assert co.coord_lengths(short[k]) == co.SHORT_MULTIPLES[k]
    id0 = 1000
    cts = [drbg("co/short/ct%d" % k, 32) for k in ks]
    choice = np.array([i & 1 for i in range(len(ks))], np.uint8)
    base = engine.CoBase(ctx, co.point_bytes(A))
    labels = base.decrypt(ks, choice, np.frombuffer(b"".join(cts), np.uint8), id0)
    base.close()
    want = [masks_xor(short[k], id0 + i, cts[i][16:] if choice[i] else cts[i][:16]) for i, k in enumerate(ks)]
    assert label_raw(labels) == want


def test_go_pinned_rounds(ctx, sha_circ):
    """sha2pc's TestDeterministicTranscript with the handle as the receiver of ot.CO: the choice points hash to Go's
    `expRound2`, and the labels decrypted from the pinned ciphertexts are the evaluator's"""
    dc = engine.DeviceCircuit(ctx, sha_circ)
    seen = {}

    def garble(key, rnd):
        g = dc.garble(key, rnd, batch=1)
        io = g["io"][0]
        seen["in"] = io[:512].copy()
        return {"in": io[:512], "out": io[512:]}, g["slab"][0]

    t = gt.transcript(sha_circ, garble, "transcript")
    dc.close()
    want = gt.CASES["transcript"][1]
    assert (t["round1"], t["round2"], t["round3"]) == want
    session, bits = go_session()
    choice = np.array(bits, np.uint8)
    base = engine.CoBase(ctx, co.point_bytes(session["A"]))
    pts = base.choices(t["scalars"], choice)
    assert round2_hash(session, [co.point_from_bytes(bytes(p)) for p in pts]) == want[1]
    wires = np.ascontiguousarray(seen["in"][256:], dtype=WIRE)
    ct = np.frombuffer(b"".join(t["ciphertexts"]), np.uint8)  # the bytes under `expRound3`
    labels = base.decrypt(t["scalars"], choice, ct)
    base.close()
    assert (labels == pick(wires, choice)).all()


def session_case(tag, n):
    a = int.from_bytes(drbg("co_base/%s/a" % tag, 32), "big")
    A, _ = co.sender_setup(a)
    scalars = [int.from_bytes(drbg("co_base/%s/b%d" % (tag, i), 32), "big") for i in range(n)]
    choice = (np.frombuffer(drbg("co_base/%s/choice" % tag, n), np.uint8) & 1).astype(np.uint8)
    cts = [drbg("co_base/%s/ct%d" % (tag, i), 32) for i in range(n)]
    id0 = 40 + len(tag)
    B = co.receiver_choices(A, scalars, list(choice))
    labels = co.receiver_decrypt(A, scalars, list(choice), cts, id0)
    return dict(A=co.point_bytes(A), scalars=scalars, choice=choice, ct=np.frombuffer(b"".join(cts), np.uint8), id0=id0,
                points=[co.point_bytes(p) for p in B], labels=labels)


def check_session(handle, s):
    assert [bytes(p) for p in handle.choices(s["scalars"], s["choice"])] == s["points"]
    assert label_raw(handle.decrypt(s["scalars"], s["choice"], s["ct"], s["id0"])) == s["labels"]


def test_handles_are_independent(ctx):
    """two handles with different A alive on one ctx, their calls interleaved; one freed, a third created"""
    s1, s2, s3 = session_case("one", 9), session_case("two", 9), session_case("three", 9)
    assert s1["A"] != s2["A"] != s3["A"]
    h1, h2 = engine.CoBase(ctx, s1["A"]), engine.CoBase(ctx, s2["A"])
    p1 = h1.choices(s1["scalars"], s1["choice"])
    p2 = h2.choices(s2["scalars"], s2["choice"])
    l1 = h1.decrypt(s1["scalars"], s1["choice"], s1["ct"], s1["id0"])
    l2 = h2.decrypt(s2["scalars"], s2["choice"], s2["ct"], s2["id0"])
    assert [bytes(p) for p in p1] == s1["points"] and [bytes(p) for p in p2] == s2["points"]
    assert label_raw(l1) == s1["labels"] and label_raw(l2) == s2["labels"]
    h1.close()
    h3 = engine.CoBase(ctx, s3["A"])
    check_session(h3, s3)
    check_session(h2, s2)
    h2.close()
    check_session(h3, s3)
    h3.close()
    h3.close()  # a second close is a no-op


def test_binding_refuses_to_free_a_handle_after_its_ctx(pool):  # noqa: F811
    """gc_co_base_free waits for the ctx stream, so the Python handle keeps its Context and will not free past it"""
    c = engine.Context(0)
    h = engine.CoBase(c, co.point_bytes(pool["A"]))
    assert h.ctx is c
    h.close()
    h = engine.CoBase(c, co.point_bytes(pool["A"]))
    c.close()
    with pytest.raises(engine.EngineError) as e:
        h.close()
    assert e.value.code == engine.GC_E_ARG and h.h


def test_base_ots_feed_iknp(ctx):
    """128 base OTs with the handle as the receiver; its labels are the k0 of gc_iknp_sender_create as they are, and a
    1 000-OT extension pairs up (as tests/test_gpu_co.py)"""
    n = 128
    wires = np.zeros(n, WIRE)
    wires["l0"] = labels_from_bytes([drbg("co/iknp/l0/%d" % i, 16) for i in range(n)])
    wires["l1"] = labels_from_bytes([drbg("co/iknp/l1/%d" % i, 16) for i in range(n)])
    delta = oracle.label_from_bytes(drbg("co/iknp/delta", 16))
    choice = np.array([oracle.label_bit(delta, i) for i in range(n)], np.uint8)
    a = int.from_bytes(drbg("co/iknp/a", 32), "big")
    A, AaInv = engine.co_sender_setup(a)
    d_sc = ctx.to_device(np.frombuffer(drbg("co/iknp/scalars", 32 * n), np.uint8).reshape(n, 32))
    d_ch, d_w = ctx.to_device(choice), ctx.to_device(wires)
    d_pts, d_ct, d_k0, d_status = ctx.zeros((n, 64)), ctx.zeros((n, 32)), ctx.zeros((n, 16)), ctx.zeros(2, np.uint64)
    base = engine.CoBase(ctx, A)
    base.choices_dev(d_sc, d_ch, n, d_pts)
    engine.co_sender_encrypt_dev(ctx, a, AaInv, d_pts, d_w, n, 0, d_ct, d_status)
    base.decrypt_dev(d_sc, d_ch, d_ct, n, 0, d_k0)
    ctx.sync()
    base.close()
    assert int(d_status.numpy()[0]) == 0
    k0 = np.frombuffer(d_k0.numpy().tobytes(), LABEL)
    assert (k0 == pick(wires, choice)).all()
    m = 1000
    b = (np.frombuffer(drbg("co/iknp/b", m), np.uint8) & 1).astype(np.uint8)
    rcv, snd = engine.IKNPReceiver(ctx, wires), engine.IKNPSender(ctx, delta, k0)
    u, got = rcv.receive(b)
    sent = snd.send(u, m)
    x0 = sent["d0"] ^ np.where(b == 1, np.uint64(delta[0]), np.uint64(0))
    x1 = sent["d1"] ^ np.where(b == 1, np.uint64(delta[1]), np.uint64(0))
    assert (got["d0"] == x0).all() and (got["d1"] == x1).all()  # rcvd = sent ^ b * delta
    rcv.close(); snd.close()


def test_misuse(ctx, base, pool):  # noqa: F811
    L, p = engine.lib(), engine._p
    E_ARG, E_POINT, OK = engine.GC_E_ARG, engine.GC_E_POINT, engine.GC_OK
    n = 4
    A = engine.co_point(pool["A"])
    sc, ch = scalars_array(pool["scalars"][:n]), pool["choice"][:n].copy()
    ct, out_pts, out_lab = np.zeros((n, 32), np.uint8), np.zeros((n, 64), np.uint8), np.zeros(n, LABEL)
    st = C.c_int(77)
    assert not L.gc_co_base_create(None, p(A), C.byref(st)) and st.value == E_ARG
    st.value = 77
    assert not L.gc_co_base_create(ctx.h, None, C.byref(st)) and st.value == E_ARG
    assert not L.gc_co_base_create(None, None, None)  # status may be NULL
    for badA in (HOSTILE["off_curve"], HOSTILE["x_equals_p"], co.INF):
        assert not co.valid_point(badA)
        st.value = 77
        assert not L.gc_co_base_create(ctx.h, p(engine.co_point(badA)), C.byref(st)) and st.value == E_POINT
        with pytest.raises(engine.EngineError) as e:
            engine.CoBase(ctx, badA)
        assert e.value.code == E_POINT and "ot: point not on curve" in str(e.value)
    L.gc_co_base_free(None)
    good_ch = [base.h, p(sc), p(ch), n, p(out_pts)]
    assert L.gc_co_base_choices(*good_ch) == OK
    for k in (0, 1, 2, 4):
        args = list(good_ch)
        args[k] = None
        assert L.gc_co_base_choices(*args) == E_ARG, k
    good_dec = [base.h, p(sc), p(ch), p(ct), n, 0, p(out_lab)]
    assert L.gc_co_base_decrypt(*good_dec) == OK
    for k in (0, 1, 2, 3, 6):
        args = list(good_dec)
        args[k] = None
        assert L.gc_co_base_decrypt(*args) == E_ARG, k
    d = ctx.zeros(64 * n)
    vp = C.c_void_p
    good_ch = [base.h, vp(d.ptr), vp(d.ptr), n, vp(d.ptr)]
    for k in (0, 1, 2, 4):
        args = list(good_ch)
        args[k] = None
        assert L.gc_co_base_choices_dev(*args) == E_ARG, k
    good_dec = [base.h, vp(d.ptr), vp(d.ptr), vp(d.ptr), n, 0, vp(d.ptr)]
    for k in (0, 1, 2, 3, 6):
        args = list(good_dec)
        args[k] = None
        assert L.gc_co_base_decrypt_dev(*args) == E_ARG, k
    # n = 0: GC_OK with no other pointer, nothing written; a NULL handle is refused all the same
    assert L.gc_co_base_choices(base.h, None, None, 0, None) == OK
    assert L.gc_co_base_decrypt(base.h, None, None, None, 0, 5, None) == OK
    assert L.gc_co_base_choices_dev(base.h, None, None, 0, None) == OK
    assert L.gc_co_base_decrypt_dev(base.h, None, None, None, 0, 5, None) == OK
    assert L.gc_co_base_choices(None, None, None, 0, None) == E_ARG
    assert L.gc_co_base_decrypt_dev(None, None, None, None, 0, 5, None) == E_ARG
    ctx.sync()
    assert (d.numpy() == 0).all()
