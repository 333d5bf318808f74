"""The Chou-Orlandi base OT for several sessions per call (gc_co_multi_*, mpc_amd/csrc/co_multi_kernels.hip, co_multi.h)
against the restated reference (tests/py_co_reference.py), called per session: byte parity of setup, choices, encrypt and
decrypt in host and device-pointer form over shapes that put a session, a wave and a workgroup edge in every relation to
each other; session s of a multi call against the one-session calls on that session alone; bad sessions and bad points
inside one wave; more than one grid sweep; Go's round constants with the pinned session between two others; misuse.

The restatement costs about 4 ms per scalar multiplication, so the curve results are computed once per module, on a pool
of 65 sessions from which every shape (S, per) takes the first `per` OTs of its first S sessions: the id of OT j of a
session is id0 + j whatever the shape, so the bytes for any shape and id0 follow by hashing alone."""
import ctypes as C

import numpy as np
import pytest

from mpc_amd import engine
from mpc_amd.circuit import LABEL, WIRE
from tests import go_transcript as gt
from tests import py_co_reference as co
from tests.test_gpu_co import (HOSTILE, ID0S, ct_bytes, expected_ct, expected_labels, label_raw, masks_xor, pick,
                               points_array, scalars_array, wires_of)
from tests.test_gpu_co import pool  # noqa: F401  (the module-scoped fixture: one session, 257 OTs with the edge scalars)
from tests.test_py_co_reference import go_session, round2_hash
from tests.util import drbg, kernel_constants

pytestmark = pytest.mark.gpu

THREADS, GRID = kernel_constants("kCoMultiThreads", "kCoMultiGrid")
SWEEP = THREADS * GRID  # OTs (setup: sessions) of one trip of the capped grid
TOP = 1 << 256
ONES = (1 << 64) - 1
CLEAN = [0, ONES, 0, ONES]
SENTINEL = 0xA5
# (S, per): every lane its own session, past a wave; sessions that straddle the 64-lane edge; wave-aligned sessions; a session
# across the 256-lane workgroup edge; the IKNP shape
SHAPES = [(65, 1), (43, 3), (3, 64), (4, 65), (2, 128)]
# OTs of pool session s: what the shapes above and the (8, 8) hostile case take from it
POOL_OTS = [128, 128, 65, 65] + [8] * 4 + [3] * 35 + [1] * 22
# the receiver's edge scalars as OT 0 of sessions 1 .. 6: different sessions of one wave in every shape with S > 6
EDGE_B = {1: (0, 1), 2: (1, 0), 3: (co.N - 1, 1), 4: (co.N, 0), 5: (co.N + 1, 1), 6: (TOP - 1, 0)}  # s: (b, choice)
# sender scalars at and above N (taken mod N)
EDGE_A = {7: co.N + 5, 8: TOP - 1, 9: 1, 10: co.N - 1}


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


def make_session(tag, n, a=None, edge=None):
    """one session of n OTs in the form of tests/test_gpu_co.py's pool, so that its expected_ct / expected_labels apply"""
    if a is None:
        a = int.from_bytes(drbg("co_multi/%s/a" % tag, 32), "big")
    A, AaInv = co.sender_setup(a)
    scalars = [int.from_bytes(drbg("co_multi/%s/b%d" % (tag, j), 32), "big") for j in range(n)]
    choice = (np.frombuffer(drbg("co_multi/%s/choice" % tag, n), np.uint8) & 1).astype(np.uint8)
    if edge is not None:
        scalars[0], choice[0] = edge
    pairs = [(drbg("co_multi/%s/l0/%d" % (tag, j), 16), drbg("co_multi/%s/l1/%d" % (tag, j), 16)) for j in range(n)]
    B = co.receiver_choices(A, scalars, list(choice))
    D = [co.mul(A, b) for b in scalars]
    infinite = [j for j, p in enumerate(B) if p == co.INF]
    S = [co.INF if j in infinite else co.mul(p, a) for j, p in enumerate(B)]
    T = [co.add(s, AaInv) for s in S]
    return dict(a=a, A=A, AaInv=AaInv, scalars=scalars, choice=choice, pairs=pairs, wires=wires_of(pairs), B=B, D=D, S=S, T=T,
                infinite=infinite)


@pytest.fixture(scope="module")
def sessions():
    assert len(POOL_OTS) == 65 and all(POOL_OTS[s] >= per for S, per in SHAPES + [(8, 8)] for s in range(S))
    out = [make_session("s%d" % s, n, EDGE_A.get(s), EDGE_B.get(s)) for s, n in enumerate(POOL_OTS)]
    assert out[4]["infinite"] == [0] and out[1]["B"][0] == out[1]["A"]  # b = N without the choice, b = 0 with it
    assert all(not out[s]["infinite"] for s in range(65) if s != 4)
    return out


def gather(sess, per):
    """the arrays of a multi call that serves the first `per` OTs of every session of the list"""
    return dict(
        a=scalars_array([s["a"] for s in sess]), A=points_array([s["A"] for s in sess]),
        AaInv=points_array([s["AaInv"] for s in sess]),
        scalars=scalars_array([b for s in sess for b in s["scalars"][:per]]).reshape(-1, 32),
        choice=np.concatenate([s["choice"][:per] for s in sess] + [np.zeros(0, np.uint8)]),
        wires=np.concatenate([s["wires"][:per] for s in sess] + [np.zeros(0, WIRE)]))


def expected(sess, per, id0):
    """-> points, ciphertexts, labels (lists of bytes, session-major) and the OT indices i of the bad points"""
    pts, cts, labels, bad = [], [], [], []
    for k, s in enumerate(sess):
        c = expected_ct(s, per, id0)
        pts += [co.point_bytes(p) for p in s["B"][:per]]
        cts += c
        labels += expected_labels(s, per, id0, c)
        bad += [k * per + j for j in s["infinite"] if j < per]
    return pts, cts, labels, bad


def run_host(ctx, g, S, per, id0):
    A, AaInv = engine.co_multi_sender_setup(ctx, g["a"])
    pts = engine.co_multi_receiver_choices(ctx, A, g["scalars"], g["choice"], S, per)
    bad = None
    try:
        ct = engine.co_multi_sender_encrypt(ctx, g["a"], AaInv, pts, g["wires"], S, per, id0)
    except engine.CoPointError as e:
        ct, bad = e.ct, e.bad_index
        assert e.code == engine.GC_E_POINT and "ot: point not on curve" in str(e)
    labels = engine.co_multi_receiver_decrypt(ctx, A, g["scalars"], g["choice"], ct, S, per, id0)
    return A, AaInv, pts, ct, labels, bad


def run_dev(ctx, g, S, per, id0):
    """-> A, AaInv, points, ct, labels, the four status blocks"""
    n = S * per
    d_a, d_sc, d_ch, d_w = ctx.to_device(g["a"]), ctx.to_device(g["scalars"]), ctx.to_device(g["choice"]), ctx.to_device(g["wires"])
    d_A, d_ainv = ctx.empty((S, 64)).zero(SENTINEL), ctx.empty((S, 64)).zero(SENTINEL)
    d_pts, d_ct, d_lab = ctx.empty((n, 64)).zero(SENTINEL), ctx.empty((n, 32)).zero(SENTINEL), ctx.empty((n, 16)).zero(SENTINEL)
    d_st = [ctx.empty(4, np.uint64).zero(SENTINEL) for _ in range(4)]
    engine.co_multi_sender_setup_dev(ctx, d_a, S, d_A, d_ainv, d_st[0])
    engine.co_multi_receiver_choices_dev(ctx, d_A, d_sc, d_ch, S, per, d_pts, d_st[1])
    engine.co_multi_sender_encrypt_dev(ctx, d_a, d_ainv, d_pts, d_w, S, per, id0, d_ct, d_st[2])
    engine.co_multi_receiver_decrypt_dev(ctx, d_A, d_sc, d_ch, d_ct, S, per, id0, d_lab, d_st[3])
    ctx.sync()
    labels = np.frombuffer(d_lab.numpy().tobytes(), LABEL)
    return d_A.numpy(), d_ainv.numpy(), d_pts.numpy(), d_ct.numpy(), labels, [[int(v) for v in d.numpy()] for d in d_st]


def check_parity(ctx, sess, S, per, id0, form):
    assert len(sess) == S
    g = gather(sess, per)
    want_pts, want_ct, want_labels, want_bad = expected(sess, per, id0)
    if form == "host":
        A, AaInv, pts, ct, labels, bad = run_host(ctx, g, S, per, id0)
        assert bad == (want_bad[0] if want_bad else None)
    else:
        A, AaInv, pts, ct, labels, st = run_dev(ctx, g, S, per, id0)
        assert st[0] == CLEAN and st[1] == CLEAN and st[3] == CLEAN
        assert st[2] == [len(want_bad), want_bad[0] if want_bad else ONES, 0, ONES]
    assert [bytes(p) for p in A] == [co.point_bytes(s["A"]) for s in sess], "A differs"
    assert [bytes(p) for p in AaInv] == [co.point_bytes(s["AaInv"]) for s in sess], "AaInv differs"
    assert [bytes(p) for p in pts] == want_pts, "choice points differ"
    assert ct_bytes(ct) == want_ct, "ciphertexts differ"
    assert label_raw(labels) == want_labels, "decrypted labels differ"
    for k, s in enumerate(sess):  # decrypt(encrypt) = L_choice
        for j in range(per):
            if j not in s["infinite"]:
                assert label_raw(labels[k * per + j:k * per + j + 1])[0] == s["pairs"][j][s["choice"][j]], (k, j)


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("id0", ID0S)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "%dx%d" % v)
def test_byte_parity(ctx, sessions, shape, id0, form):
    S, per = shape
    check_parity(ctx, sessions[:S], S, per, id0, form)


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("id0", ID0S)
def test_one_session_is_todays_session(ctx, pool, id0, form):  # noqa: F811
    """(1, 257): the bytes tests/test_gpu_co.py expects of the one-session calls on its pool"""
    check_parity(ctx, [pool], 1, 257, id0, form)


@pytest.mark.parametrize("shape", [(0, 5), (5, 0)], ids=lambda v: "%dx%d" % v)
def test_nothing_is_written_at_zero(ctx, sessions, shape):
    S, per = shape
    L, p = engine.lib(), engine._p
    g = gather(sessions[:5], 1)
    # device form: sentinel-filled outputs and status blocks stay as they are
    d = {k: ctx.to_device(v) for k, v in g.items()}
    out = {k: ctx.empty((5, w)).zero(SENTINEL) for k, w in (("A", 64), ("ainv", 64), ("pts", 64), ("ct", 32), ("lab", 16))}
    d_st = ctx.empty(4, np.uint64).zero(SENTINEL)
    if S == 0:
        engine.co_multi_sender_setup_dev(ctx, d["a"], 0, out["A"], out["ainv"], d_st)
    engine.co_multi_receiver_choices_dev(ctx, d["A"], d["scalars"], d["choice"], S, per, out["pts"], d_st)
    engine.co_multi_sender_encrypt_dev(ctx, d["a"], d["AaInv"], out["pts"], d["wires"], S, per, 3, out["ct"], d_st)
    engine.co_multi_receiver_decrypt_dev(ctx, d["A"], d["scalars"], d["choice"], out["ct"], S, per, 3, out["lab"], d_st)
    ctx.sync()
    assert all((b.numpy() == SENTINEL).all() for b in out.values())
    assert (d_st.numpy().view(np.uint8) == SENTINEL).all()
    # host form: the same of host arrays, bad_index and bad_session included; no pointer is needed
    h_pts, h_ct, h_lab = np.full((5, 64), 0x77, np.uint8), np.full((5, 32), 0x77, np.uint8), np.full((5, 16), 0x77, np.uint8)
    h_A, h_ainv = np.full((5, 64), 0x77, np.uint8), np.full((5, 64), 0x77, np.uint8)
    bad, bad_s = C.c_size_t(99), C.c_size_t(98)
    if S == 0:
        assert L.gc_co_multi_sender_setup(ctx.h, p(g["a"]), 0, p(h_A), p(h_ainv), C.byref(bad_s)) == engine.GC_OK
        assert L.gc_co_multi_sender_setup(ctx.h, None, 0, None, None, None) == engine.GC_OK
    assert L.gc_co_multi_receiver_choices(ctx.h, p(g["A"]), p(g["scalars"]), p(g["choice"]), S, per, p(h_pts),
                                          C.byref(bad_s)) == engine.GC_OK
    assert L.gc_co_multi_sender_encrypt(ctx.h, p(g["a"]), p(g["AaInv"]), p(h_pts), p(g["wires"]), S, per, 3, p(h_ct),
                                        C.byref(bad), C.byref(bad_s)) == engine.GC_OK
    assert L.gc_co_multi_receiver_decrypt(ctx.h, p(g["A"]), p(g["scalars"]), p(g["choice"]), p(h_ct), S, per, 3, p(h_lab),
                                          C.byref(bad_s)) == engine.GC_OK
    assert L.gc_co_multi_receiver_choices(ctx.h, None, None, None, S, per, None, None) == engine.GC_OK
    assert L.gc_co_multi_sender_encrypt(ctx.h, None, None, None, None, S, per, 3, None, None, None) == engine.GC_OK
    assert L.gc_co_multi_receiver_decrypt(ctx.h, None, None, None, None, S, per, 3, None, None) == engine.GC_OK
    assert L.gc_co_multi_sender_encrypt_dev(ctx.h, None, None, None, None, S, per, 3, None, None) == engine.GC_OK
    assert L.gc_co_multi_receiver_choices_dev(ctx.h, None, None, None, S, per, None, None) == engine.GC_OK
    assert L.gc_co_multi_receiver_decrypt_dev(ctx.h, None, None, None, None, S, per, 3, None, None) == engine.GC_OK
    assert all((a == 0x77).all() for a in (h_pts, h_ct, h_lab, h_A, h_ainv)) and (bad.value, bad_s.value) == (99, 98)
    assert len(engine.co_multi_receiver_choices(ctx, g["A"][:S], [], [], S, per)) == 0
    assert len(engine.co_multi_sender_encrypt(ctx, g["a"][:S], g["AaInv"][:S], [], np.zeros(0, WIRE), S, per)) == 0


def test_sessions_do_not_leak(ctx, sessions):
    """(4, 65), device against device: session s of the multi calls equals the one-session gc_co_* calls on that session
    alone, with that session's constants as host arguments and its OTs numbered from id0"""
    S, per, id0 = 4, 65, (1 << 32) - 3
    sess = sessions[:S]
    g = gather(sess, per)
    A, AaInv, pts, ct, labels, st = run_dev(ctx, g, S, per, id0)
    assert st == [CLEAN] * 4
    for k, s in enumerate(sess):
        lo, hi = k * per, (k + 1) * per
        A1, AaInv1 = engine.co_sender_setup(s["a"])
        assert bytes(A1) == bytes(A[k]) and bytes(AaInv1) == bytes(AaInv[k])
        d_sc, d_ch, d_w = ctx.to_device(g["scalars"][lo:hi]), ctx.to_device(g["choice"][lo:hi]), ctx.to_device(g["wires"][lo:hi])
        d_pts, d_ct, d_lab = ctx.zeros((per, 64)), ctx.zeros((per, 32)), ctx.zeros((per, 16))
        d_status = ctx.zeros(2, np.uint64)
        engine.co_receiver_choices_dev(ctx, A1, d_sc, d_ch, per, d_pts)
        engine.co_sender_encrypt_dev(ctx, s["a"], AaInv1, d_pts, d_w, per, id0, d_ct, d_status)
        engine.co_receiver_decrypt_dev(ctx, A1, d_sc, d_ch, d_ct, per, id0, d_lab)
        ctx.sync()
        assert [int(v) for v in d_status.numpy()] == [0, ONES]
        assert (d_pts.numpy() == pts[lo:hi]).all(), "choice points of session %d" % k
        assert (d_ct.numpy() == ct[lo:hi]).all(), "ciphertexts of session %d" % k
        assert d_lab.numpy().tobytes() == labels[lo:hi].tobytes(), "labels of session %d" % k


def test_hostile_inputs_inside_one_wave(ctx, sessions):
    """(8, 8), 64 OTs: one wave.  Sender: session 1 has a = 0 mod N, session 3 an AaInv off the curve; both hold an off-curve
    point too, which is not counted.  The good sessions hold a point off the curve (0, 2), B = A_s (2, 4: T is infinity and
    hashes as the bare id) and B = -A_s (4, 1: S = AaInv_s, the addition doubles on that lane alone); session 4's OT 0 is
    the pool's point at infinity.  Receiver: session 5 has an A with x = p."""
    S, per, id0 = 8, 8, 77
    sess = sessions[:S]
    g = gather(sess, per)
    n = S * per
    at = lambda s, j: s * per + j  # noqa: E731
    points = [p for s in sess for p in s["B"][:per]]
    Ss = [p for s in sess for p in s["S"][:per]]
    off = HOSTILE["off_curve"]
    points[at(0, 2)] = points[at(1, 5)] = points[at(3, 0)] = off
    for s, j, p in ((2, 4, sess[2]["A"]), (4, 1, co.neg(sess[4]["A"]))):
        points[at(s, j)], Ss[at(s, j)] = p, co.mul(p, sess[s]["a"])
    assert co.add(Ss[at(2, 4)], sess[2]["AaInv"]) == co.INF and Ss[at(4, 1)] == sess[4]["AaInv"]
    a = g["a"].copy()
    a[1] = np.frombuffer(co.N.to_bytes(32, "big"), np.uint8)
    AaInv = g["AaInv"].copy()
    x, y = sess[3]["AaInv"]
    AaInv[3] = np.frombuffer(co.point_bytes((x, (y + 1) % co.P)), np.uint8)
    bad_sessions, bad_points = {1, 3}, [at(0, 2), at(4, 0)]
    want = []
    for i in range(n):
        s, j = divmod(i, per)
        if s in bad_sessions or i in bad_points:
            want.append(bytes(32))
            continue
        assert co.valid_point(points[i])
        T = co.add(Ss[i], sess[s]["AaInv"])
        want.append(masks_xor(Ss[i], id0 + j, sess[s]["pairs"][j][0]) + masks_xor(T, id0 + j, sess[s]["pairs"][j][1]))
    pts = points_array(points)
    # the sender's setup: session 1 is bad, its points are zero, the others are the restatement's
    d_a, d_A, d_ainv, d_st = ctx.to_device(a), ctx.empty((S, 64)).zero(SENTINEL), ctx.empty((S, 64)).zero(SENTINEL), \
        ctx.empty(4, np.uint64).zero(SENTINEL)
    engine.co_multi_sender_setup_dev(ctx, d_a, S, d_A, d_ainv, d_st)
    ctx.sync()
    assert [int(v) for v in d_st.numpy()] == [0, ONES, 1, 1]
    for k in range(S):
        assert bytes(d_A.numpy()[k]) == (bytes(64) if k == 1 else co.point_bytes(sess[k]["A"])), k
        assert bytes(d_ainv.numpy()[k]) == (bytes(64) if k == 1 else co.point_bytes(sess[k]["AaInv"])), k
    with pytest.raises(engine.CoSessionError) as e:
        engine.co_multi_sender_setup(ctx, a)
    assert e.value.code == engine.GC_E_ARG and e.value.bad_session == 1
    assert (e.value.out[0] == d_A.numpy()).all() and (e.value.out[1] == d_ainv.numpy()).all()
    # encrypt, device form: all four status words, zeros in the bad sessions and at the bad points, every other OT untouched
    d_ct = ctx.empty((n, 32)).zero(SENTINEL)
    engine.co_multi_sender_encrypt_dev(ctx, d_a, ctx.to_device(AaInv), ctx.to_device(pts), ctx.to_device(g["wires"]), S, per, id0,
                                       d_ct, d_st)
    ctx.sync()
    assert [int(v) for v in d_st.numpy()] == [2, at(0, 2), 2, 1]
    assert ct_bytes(d_ct.numpy()) == want
    # host form: a bad session wins, GC_E_ARG; the lowest bad point is reported next to it
    with pytest.raises(engine.CoSessionError) as e:
        engine.co_multi_sender_encrypt(ctx, a, AaInv, pts, g["wires"], S, per, id0)
    assert e.value.code == engine.GC_E_ARG and e.value.bad_session == 1 and e.value.bad_index == at(0, 2)
    assert ct_bytes(e.value.out) == want
    # ... and with good sessions only, a bad point alone is GC_E_POINT
    with pytest.raises(engine.CoPointError) as e:
        engine.co_multi_sender_encrypt(ctx, g["a"], g["AaInv"], pts, g["wires"], S, per, id0)
    assert e.value.code == engine.GC_E_POINT and e.value.bad_index == at(0, 2)
    got = ct_bytes(e.value.ct)
    assert [got[i] for i in range(n) if i // per not in bad_sessions] == [want[i] for i in range(n) if i // per not in bad_sessions]
    assert not e.value.ct[at(1, 5)].any() and e.value.ct[at(1, 4)].any() and e.value.ct[at(3, 1)].any()
    # the receiver with A_5 = (p, sqrt b): zeros in session 5 alone, GC_E_POINT
    A = g["A"].copy()
    assert not co.valid_point(HOSTILE["x_equals_p"])
    A[5] = np.frombuffer(co.point_bytes(HOSTILE["x_equals_p"]), np.uint8)
    want_pts, want_ct, want_labels, _ = expected(sess, per, id0)
    cts = np.frombuffer(b"".join(want_ct), np.uint8)
    d_pts, d_lab = ctx.empty((n, 64)).zero(SENTINEL), ctx.empty((n, 16)).zero(SENTINEL)
    d_st2 = ctx.empty(4, np.uint64).zero(SENTINEL)
    d_Ab, d_sc, d_ch = ctx.to_device(A), ctx.to_device(g["scalars"]), ctx.to_device(g["choice"])
    engine.co_multi_receiver_choices_dev(ctx, d_Ab, d_sc, d_ch, S, per, d_pts, d_st)
    engine.co_multi_receiver_decrypt_dev(ctx, d_Ab, d_sc, d_ch, ctx.to_device(cts), S, per, id0, d_lab, d_st2)
    ctx.sync()
    assert [int(v) for v in d_st.numpy()] == [0, ONES, 1, 5] and [int(v) for v in d_st2.numpy()] == [0, ONES, 1, 5]
    in5 = lambda i: i // per == 5  # noqa: E731
    assert [bytes(p) for p in d_pts.numpy()] == [bytes(64) if in5(i) else want_pts[i] for i in range(n)]
    lab = label_raw(np.frombuffer(d_lab.numpy().tobytes(), LABEL))
    assert lab == [bytes(16) if in5(i) else want_labels[i] for i in range(n)]
    with pytest.raises(engine.CoSessionError) as e:
        engine.co_multi_receiver_choices(ctx, A, g["scalars"], g["choice"], S, per)
    assert e.value.code == engine.GC_E_POINT and e.value.bad_session == 5 and "ot: point not on curve" in str(e.value)
    assert (e.value.out == d_pts.numpy()).all()
    with pytest.raises(engine.CoSessionError) as e:
        engine.co_multi_receiver_decrypt(ctx, A, g["scalars"], g["choice"], cts, S, per, id0)
    assert e.value.code == engine.GC_E_POINT and e.value.bad_session == 5
    assert label_raw(e.value.out) == lab


def test_past_one_grid_sweep(ctx):
    """Sessions of 127 OTs (no multiple of the wave) through the device-pointer forms, so many that S * per exceeds one trip
    of the capped grid by a full workgroup and a ragged one: those lanes make a second trip of the grid-stride loop, inside
    sessions that began in the first.  The setup kernel has one lane per SESSION: its grid here is S / 256 workgroups, one
    trip (tests/test_gpu_co_multi.py::test_setup_past_one_grid_sweep makes its second).  decrypt(encrypt(choices)) =
    L_choice at every OT, and point, ciphertext, label, A and AaInv equal the restatement's at 24 OTs, both sides of the
    sweep edge and of a session edge among them."""
    per = 127
    S = -(-(SWEEP + THREADS + 1) // per)
    n, id0 = S * per, (1 << 32) - 7  # the id carries into its high word at OT 7 of every session
    assert n > SWEEP + THREADS and (n - SWEEP) % THREADS != 0 and per % 64 != 0
    rng = np.random.default_rng(20250211)
    a = rng.integers(0, 256, (S, 32), dtype=np.uint8)
    scalars = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    choice = rng.integers(0, 2, n).astype(np.uint8)
    wires = np.zeros(n, WIRE)
    for half in ("l0", "l1"):
        wires[half]["d0"] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        wires[half]["d1"] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    d_a, d_sc, d_ch, d_w = ctx.to_device(a), ctx.to_device(scalars), ctx.to_device(choice), ctx.to_device(wires)
    d_A, d_ainv = ctx.empty((S, 64)).zero(SENTINEL), ctx.empty((S, 64)).zero(SENTINEL)
    d_pts, d_ct, d_lab = ctx.empty((n, 64)).zero(SENTINEL), ctx.empty((n, 32)).zero(SENTINEL), ctx.empty((n, 16)).zero(SENTINEL)
    d_st = [ctx.empty(4, np.uint64).zero(SENTINEL) for _ in range(4)]
    engine.co_multi_sender_setup_dev(ctx, d_a, S, d_A, d_ainv, d_st[0])
    engine.co_multi_receiver_choices_dev(ctx, d_A, d_sc, d_ch, S, per, d_pts, d_st[1])
    engine.co_multi_sender_encrypt_dev(ctx, d_a, d_ainv, d_pts, d_w, S, per, id0, d_ct, d_st[2])
    engine.co_multi_receiver_decrypt_dev(ctx, d_A, d_sc, d_ch, d_ct, S, per, id0, d_lab, d_st[3])
    ctx.sync()
    assert [[int(v) for v in d.numpy()] for d in d_st] == [CLEAN] * 4
    As, ainvs, pts, ct = d_A.numpy(), d_ainv.numpy(), d_pts.numpy(), d_ct.numpy()
    labels = np.frombuffer(d_lab.numpy().tobytes(), LABEL)
    bad = np.flatnonzero(labels != pick(wires, choice))
    assert bad.size == 0, "decrypt(encrypt) != L_choice at %d OTs, the first %d" % (bad.size, bad[0])
    edge = (SWEEP // per) * per  # the first OT of the session that the sweep edge falls into
    assert edge < SWEEP < edge + per
    idx = {0, 1, n - 2, n - 1, edge - 1, edge, edge + per - 1, edge + per} | set(range(SWEEP - 4, SWEEP + 4))
    while len(idx) < 24:
        idx.add(int(rng.integers(0, n)))
    for i in sorted(idx):
        s, j = divmod(i, per)
        av = int.from_bytes(bytes(a[s]), "big")
        A, AaInv = co.sender_setup(av)
        assert bytes(As[s]) == co.point_bytes(A) and bytes(ainvs[s]) == co.point_bytes(AaInv), "setup of session %d" % s
        b, c = int.from_bytes(bytes(scalars[i]), "big"), int(choice[i])
        pair = (label_raw(wires["l0"][i:i + 1])[0], label_raw(wires["l1"][i:i + 1])[0])
        B = co.receiver_choices(A, [b], [c])
        assert bytes(pts[i]) == co.point_bytes(B[0]), "choice point %d" % i
        cts, none_bad = co.sender_encrypt(av, AaInv, B, [pair], id0 + j)
        assert not none_bad and bytes(ct[i]) == cts[0], "ciphertext %d" % i
        assert label_raw(labels[i:i + 1]) == co.receiver_decrypt(A, [b], [c], cts, id0 + j) == [pair[c]], "label %d" % i


def test_setup_past_one_grid_sweep(ctx):
    """more sessions than one trip of the setup kernel's capped grid has lanes, with a full and a ragged workgroup behind it:
    no session is bad, the sampled ones equal the restatement's on both sides of the edge, and a_s = N behind it is found"""
    S = SWEEP + THREADS + 37
    rng = np.random.default_rng(20250212)
    a = rng.integers(0, 256, (S, 32), dtype=np.uint8)
    zero_at = SWEEP + 9
    a[zero_at] = np.frombuffer(co.N.to_bytes(32, "big"), np.uint8)
    d_A, d_ainv = ctx.empty((S, 64)).zero(SENTINEL), ctx.empty((S, 64)).zero(SENTINEL)
    d_st = ctx.empty(4, np.uint64).zero(SENTINEL)
    engine.co_multi_sender_setup_dev(ctx, ctx.to_device(a), S, d_A, d_ainv, d_st)
    ctx.sync()
    assert [int(v) for v in d_st.numpy()] == [0, ONES, 1, zero_at]
    As, ainvs = d_A.numpy(), d_ainv.numpy()
    zero = np.flatnonzero(~As.any(axis=1) | ~ainvs.any(axis=1))
    assert list(zero) == [zero_at]
    assert not (As == SENTINEL).all(axis=1).any() and not (ainvs == SENTINEL).all(axis=1).any()
    for s in (0, SWEEP - 1, SWEEP, SWEEP + THREADS, S - 1):
        A, AaInv = co.sender_setup(int.from_bytes(bytes(a[s]), "big"))
        assert bytes(As[s]) == co.point_bytes(A) and bytes(ainvs[s]) == co.point_bytes(AaInv), s


def test_go_pinned_session_between_two_others(ctx, sha_circ):
    """sha2pc's TestDeterministicTranscript as session 1 of 3, between seeded neighbours of the same length: its choice
    points hash to Go's `expRound2`, its ciphertexts are the bytes under `expRound3`, its labels are the evaluator's"""
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
    S, per = 3, 256
    assert len(bits) == per and len(t["scalars"]) == per
    rng = np.random.default_rng(20250213)
    a = rng.integers(0, 256, (S, 32), dtype=np.uint8)
    a[1] = np.frombuffer(session["a"].to_bytes(32, "big"), np.uint8)
    scalars = rng.integers(0, 256, (S * per, 32), dtype=np.uint8)
    scalars[per:2 * per] = scalars_array(t["scalars"])
    choice = rng.integers(0, 2, S * per).astype(np.uint8)
    choice[per:2 * per] = np.array(bits, np.uint8)
    wires = np.zeros(S * per, WIRE)
    for half in ("l0", "l1"):
        wires[half]["d0"] = rng.integers(0, 1 << 64, S * per, dtype=np.uint64)
        wires[half]["d1"] = rng.integers(0, 1 << 64, S * per, dtype=np.uint64)
    wires[per:2 * per] = np.ascontiguousarray(seen["in"][256:], dtype=WIRE)
    A, AaInv = engine.co_multi_sender_setup(ctx, a)
    assert bytes(A[1]) == co.point_bytes(session["A"]) and bytes(AaInv[1]) == co.point_bytes(session["AaInv"])
    pts = engine.co_multi_receiver_choices(ctx, A, scalars, choice, S, per)
    assert round2_hash(session, [co.point_from_bytes(bytes(p)) for p in pts[per:2 * per]]) == want[1]
    ct = engine.co_multi_sender_encrypt(ctx, a, AaInv, pts, wires, S, per)
    assert ct_bytes(ct[per:2 * per]) == t["ciphertexts"]
    r3 = t["round3_bytes"]
    assert r3[len(r3) - 32 * per:] == b"".join(ct_bytes(ct[per:2 * per]))  # the tail of the payload that `expRound3` hashes
    labels = engine.co_multi_receiver_decrypt(ctx, A, scalars, choice, ct, S, per)
    assert (labels == pick(wires, choice)).all()  # the neighbours' as well


def test_misuse(ctx, sessions):
    L, p, vp = engine.lib(), engine._p, C.c_void_p
    E_ARG, OK = engine.GC_E_ARG, engine.GC_OK
    S, per = 2, 2
    n = S * per
    g = gather(sessions[:S], per)
    pts = points_array([q for s in sessions[:S] for q in s["B"][:per]])
    ct, out_pts, out_lab = np.zeros((n, 32), np.uint8), np.zeros((n, 64), np.uint8), np.zeros(n, LABEL)
    out_A, out_ainv = np.zeros((S, 64), np.uint8), np.zeros((S, 64), np.uint8)
    bad, bad_s = C.c_size_t(99), C.c_size_t(98)
    # host forms: every pointer but bad_index / bad_session, which may be NULL
    calls = [
        (L.gc_co_multi_sender_setup, [ctx.h, p(g["a"]), S, p(out_A), p(out_ainv), C.byref(bad_s)], (0, 1, 3, 4), (5,)),
        (L.gc_co_multi_sender_encrypt, [ctx.h, p(g["a"]), p(g["AaInv"]), p(pts), p(g["wires"]), S, per, 0, p(ct), C.byref(bad),
                                        C.byref(bad_s)], (0, 1, 2, 3, 4, 8), (9, 10)),
        (L.gc_co_multi_receiver_choices, [ctx.h, p(g["A"]), p(g["scalars"]), p(g["choice"]), S, per, p(out_pts), C.byref(bad_s)],
         (0, 1, 2, 3, 6), (7,)),
        (L.gc_co_multi_receiver_decrypt, [ctx.h, p(g["A"]), p(g["scalars"]), p(g["choice"]), p(ct), S, per, 0, p(out_lab),
                                          C.byref(bad_s)], (0, 1, 2, 3, 4, 8), (9,)),
    ]
    for fn, good, needed, optional in calls:
        assert fn(*good) == OK, fn.__name__
        for k in needed:
            args = list(good)
            args[k] = None
            assert fn(*args) == E_ARG, (fn.__name__, k)
        args = list(good)
        for k in optional:
            args[k] = None
        assert fn(*args) == OK, fn.__name__
    assert (bad.value, bad_s.value) == (99, 98)
    # device forms: every pointer, the status block included
    d = ctx.zeros(64 * n)
    q = vp(d.ptr)
    dev_calls = [
        (L.gc_co_multi_sender_setup_dev, [ctx.h, q, S, q, q, q], (0, 1, 3, 4, 5)),
        (L.gc_co_multi_sender_encrypt_dev, [ctx.h, q, q, q, q, S, per, 0, q, q], (0, 1, 2, 3, 4, 8, 9)),
        (L.gc_co_multi_receiver_choices_dev, [ctx.h, q, q, q, S, per, q, q], (0, 1, 2, 3, 6, 7)),
        (L.gc_co_multi_receiver_decrypt_dev, [ctx.h, q, q, q, q, S, per, 0, q, q], (0, 1, 2, 3, 4, 8, 9)),
    ]
    for fn, good, needed in dev_calls:
        for k in needed:
            args = list(good)
            args[k] = None
            assert fn(*args) == E_ARG, (fn.__name__, k)
    # a NULL ctx is refused at zero as well
    assert L.gc_co_multi_sender_setup(None, None, 0, None, None, None) == E_ARG
    assert L.gc_co_multi_receiver_choices_dev(None, None, None, None, 0, 5, None, None) == E_ARG
    # S * per that overflows, and one whose 64 bytes per OT do
    top = C.c_size_t(-1).value
    for big_s, big_per in ((top, 2), (top // 2 + 1, 2), (top // 64 + 1, 1), (1, top // 64 + 1), (1 << 40, 1 << 40)):
        assert L.gc_co_multi_sender_encrypt(ctx.h, p(g["a"]), p(g["AaInv"]), p(pts), p(g["wires"]), big_s, big_per, 0, p(ct),
                                            None, None) == E_ARG
        assert L.gc_co_multi_receiver_choices(ctx.h, p(g["A"]), p(g["scalars"]), p(g["choice"]), big_s, big_per, p(out_pts),
                                              None) == E_ARG
        assert L.gc_co_multi_receiver_decrypt(ctx.h, p(g["A"]), p(g["scalars"]), p(g["choice"]), p(ct), big_s, big_per, 0,
                                              p(out_lab), None) == E_ARG
        assert L.gc_co_multi_sender_encrypt_dev(ctx.h, q, q, q, q, big_s, big_per, 0, q, q) == E_ARG
        assert L.gc_co_multi_receiver_choices_dev(ctx.h, q, q, q, big_s, big_per, q, q) == E_ARG
        assert L.gc_co_multi_receiver_decrypt_dev(ctx.h, q, q, q, q, big_s, big_per, 0, q, q) == E_ARG
    assert L.gc_co_multi_sender_setup(ctx.h, p(g["a"]), top // 64 + 1, p(out_A), p(out_ainv), None) == E_ARG
    assert L.gc_co_multi_sender_setup_dev(ctx.h, q, top // 64 + 1, q, q, q) == E_ARG
    ctx.sync()
    assert (d.numpy() == 0).all()


def test_first_table_call_inside_a_capture_is_refused(sessions):
    """setup and choices read G's window table, which the first such call of a ctx uploads synchronously: not between
    gc_ctx_capture_begin and _end.  The ctx stays usable, and the same call outside a capture uploads the table and runs."""
    c = engine.Context(0)
    S, per = 2, 2
    g = gather(sessions[:S], per)
    d_a, d_A0, d_sc, d_ch = c.to_device(g["a"]), c.to_device(g["A"]), c.to_device(g["scalars"]), c.to_device(g["choice"])
    d_A, d_ainv, d_pts, d_st = c.zeros((S, 64)), c.zeros((S, 64)), c.zeros((S * per, 64)), c.zeros(4, np.uint64)
    for call in (lambda: engine.co_multi_sender_setup_dev(c, d_a, S, d_A, d_ainv, d_st),
                 lambda: engine.co_multi_receiver_choices_dev(c, d_A0, d_sc, d_ch, S, per, d_pts, d_st)):
        with pytest.raises(engine.EngineError) as e:
            c.capture(call)
        assert e.value.code == engine.GC_E_ARG
    c.sync()
    assert not d_A.numpy().any() and not d_pts.numpy().any() and not d_st.numpy().any()
    engine.co_multi_sender_setup_dev(c, d_a, S, d_A, d_ainv, d_st)  # uploads the table
    engine.co_multi_receiver_choices_dev(c, d_A, d_sc, d_ch, S, per, d_pts, d_st)
    c.sync()
    assert [bytes(x) for x in d_A.numpy()] == [co.point_bytes(s["A"]) for s in sessions[:S]]
    assert [bytes(x) for x in d_pts.numpy()] == [co.point_bytes(q) for s in sessions[:S] for q in s["B"][:per]]
    assert engine.lib().gc_abi_version() == 2
    c.close()
