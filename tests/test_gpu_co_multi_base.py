"""The multi-session Chou-Orlandi receiver behind a handle (gc_co_multi_base_*, mpc_amd/csrc/co_multi_base_kernels.hip,
co_multi_table.h): per-session window tables built on the device, and a decrypt that reads them.  The yardsticks are the
restated reference (tests/py_co_reference.py) and the ladder call gc_co_multi_receiver_decrypt_dev on the same inputs:
byte parity over the shapes of tests/test_gpu_co_multi.py in host and device form; every one of the 2 x 960 table entries
through the public call; the chunk edges of the build; more than one sweep of the decrypt kernel's capped grid; bad sessions
inside one wave; reuse and lifetime of handles; Go's pinned session between two others; misuse.

The pool of sessions is that of tests/test_gpu_co_multi.py (computed once for this module)."""
import ctypes as C

import numpy as np
import pytest

from mpc_amd import engine
from mpc_amd.circuit import LABEL, WIRE
from tests import go_transcript as gt
from tests import py_co_reference as co
from tests.test_co_table_host import expected_table
from tests.test_gpu_co import HOSTILE, ID0S, ct_bytes, label_raw, masks_xor, pick, scalars_array
from tests.test_gpu_co_multi import CLEAN, ONES, SENTINEL, SHAPES, expected, gather
from tests.test_gpu_co_multi import sessions  # noqa: F401  (the module-scoped fixture: 65 sessions with the edge scalars)
from tests.test_py_co_reference import go_session
from tests.util import drbg, kernel_constants

pytestmark = pytest.mark.gpu

THREADS, GRID, CHUNK = kernel_constants("kCoMultiTabThreads", "kCoMultiTabGrid", "kCoMultiTabChunk")
SWEEP = THREADS * GRID  # OTs of one trip of the decrypt kernel's capped grid
TOP = 1 << 256


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


def as_labels(d_lab):
    return np.frombuffer(d_lab.numpy().tobytes(), LABEL)


def status_of(d_st):
    return [int(v) for v in d_st.numpy()]


def handle_dev(ctx, h, sc, ch, cts, per, id0):
    """the handle's device form on host arrays -> labels, status"""
    n = h.S * per
    d_lab, d_st = ctx.empty((n, 16)).zero(SENTINEL), ctx.empty(4, np.uint64).zero(SENTINEL)
    h.decrypt_dev(ctx.to_device(sc), ctx.to_device(ch), ctx.to_device(cts), per, id0, d_lab, d_st)
    ctx.sync()
    return as_labels(d_lab), status_of(d_st)


def ladder_dev(ctx, A, sc, ch, cts, S, per, id0):
    """gc_co_multi_receiver_decrypt_dev on host arrays -> labels, status"""
    n = S * per
    d_lab, d_st = ctx.empty((n, 16)).zero(SENTINEL), ctx.empty(4, np.uint64).zero(SENTINEL)
    engine.co_multi_receiver_decrypt_dev(ctx, ctx.to_device(A), ctx.to_device(sc), ctx.to_device(ch), ctx.to_device(cts), S, per,
                                         id0, d_lab, d_st)
    ctx.sync()
    return as_labels(d_lab), status_of(d_st)


def ct_array(cts):
    return np.frombuffer(b"".join(cts), np.uint8).reshape(-1, 32).copy()


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("id0", ID0S)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "%dx%d" % v)
def test_byte_parity(ctx, sessions, shape, id0, form):  # noqa: F811
    S, per = shape
    sess = sessions[:S]
    g = gather(sess, per)
    _, want_ct, want_labels, _ = expected(sess, per, id0)
    cts = ct_array(want_ct)
    ladder, ladder_st = ladder_dev(ctx, g["A"], g["scalars"], g["choice"], cts, S, per, id0)
    assert ladder_st == CLEAN
    if form == "host":
        h = engine.CoMultiBase(ctx, g["A"])
        labels = h.decrypt(g["scalars"], g["choice"], cts, per, id0)
    else:
        h = engine.CoMultiBase(ctx, ctx.to_device(g["A"]), S)
        labels, st = handle_dev(ctx, h, g["scalars"], g["choice"], cts, per, id0)
        assert st == CLEAN
    assert h.info() == (S, 0, None)
    h.close()
    assert label_raw(labels) == want_labels, "decrypted labels differ from the restatement's"
    assert labels.tobytes() == ladder.tobytes(), "decrypted labels differ from the ladder call's"
    if S > 6:  # the receiver's edge scalars 0, 1, N - 1, N, N + 1, 2^256 - 1 are OT 0 of sessions 1 .. 6: one wave
        assert 6 * per < 64
        assert [sess[s]["scalars"][0] for s in range(1, 7)] == [0, 1, co.N - 1, co.N, co.N + 1, TOP - 1]


def test_every_table_entry_through_the_public_call(ctx):
    """S = 2, per = 960: scalar j = 15 i + d - 1 of each session is d * 16^i, whose product is the table entry (i, d) alone, so
    label j = mask(T[i][d - 1], id0 + j) ^ ct with T from Python additions, no scalar multiplication"""
    S, per, id0 = 2, 960, (1 << 32) - 500
    A = [co.mul(co.G, int.from_bytes(drbg("co_multi_base/entries/a%d" % s, 32), "big") % co.N) for s in range(S)]
    ks = [d << (4 * i) for i in range(64) for d in range(1, 16)]
    assert len(ks) == per and len(set(ks)) == per and max(ks) < co.N
    sc = scalars_array(ks * S)
    rng = np.random.default_rng(20250301)
    ch = rng.integers(0, 2, S * per).astype(np.uint8)
    cts = rng.integers(0, 256, (S * per, 32), dtype=np.uint8)
    h = engine.CoMultiBase(ctx, A)
    labels = label_raw(h.decrypt(sc, ch, cts, per, id0))
    h.close()
    for s in range(S):
        windows, digits, table = expected_table(A[s], 4)
        assert (windows, digits, len(table)) == (64, 15, per)
        for j in range(per):
            c = bytes(cts[s * per + j])
            want = masks_xor(table[j], id0 + j, c[16:] if ch[s * per + j] else c[:16])
            assert labels[s * per + j] == want, "session %d, window %d, digit %d" % (s, j // 15, j % 15 + 1)


def test_chunk_edges_of_the_build(ctx):
    """five sessions more than one chunk of the rows kernel, one OT each, A_s = a_s * G from the device setup: device against
    device the ladder call's labels, and the restatement's on both sides of the chunk edge"""
    S, per, id0 = CHUNK + 5, 1, 41
    rng = np.random.default_rng(20250302)
    a = rng.integers(0, 256, (S, 32), dtype=np.uint8)
    sc = rng.integers(0, 256, (S, 32), dtype=np.uint8)
    ch = rng.integers(0, 2, S).astype(np.uint8)
    cts = rng.integers(0, 256, (S, 32), dtype=np.uint8)
    d_A, d_ainv, d_st = ctx.empty((S, 64)).zero(SENTINEL), ctx.empty((S, 64)).zero(SENTINEL), ctx.empty(4, np.uint64)
    engine.co_multi_sender_setup_dev(ctx, ctx.to_device(a), S, d_A, d_ainv, d_st)
    h = engine.CoMultiBase(ctx, d_A, S)  # reads d_A behind the setup kernel, on the ctx stream
    assert status_of(d_st) == CLEAN and h.info() == (S, 0, None)
    d_sc, d_ch, d_ct = ctx.to_device(sc), ctx.to_device(ch), ctx.to_device(cts)
    d_lab, d_lad = ctx.empty((S, 16)).zero(SENTINEL), ctx.empty((S, 16)).zero(SENTINEL)
    d_st2 = ctx.empty(4, np.uint64).zero(SENTINEL)
    h.decrypt_dev(d_sc, d_ch, d_ct, per, id0, d_lab, d_st)
    engine.co_multi_receiver_decrypt_dev(ctx, d_A, d_sc, d_ch, d_ct, S, per, id0, d_lad, d_st2)
    ctx.sync()
    h.close()
    assert status_of(d_st) == CLEAN and status_of(d_st2) == CLEAN
    labels, ladder = as_labels(d_lab), as_labels(d_lad)
    bad = np.flatnonzero(labels != ladder)
    assert bad.size == 0, "%d sessions differ from the ladder call, the first %d" % (bad.size, bad[0])
    for s in (0, CHUNK - 1, CHUNK, CHUNK + 4):
        A = co.sender_setup(int.from_bytes(bytes(a[s]), "big"))[0]
        c = bytes(cts[s])
        want = masks_xor(co.mul(A, int.from_bytes(bytes(sc[s]), "big")), id0, c[16:] if ch[s] else c[:16])
        assert label_raw(labels[s:s + 1]) == [want], s


def test_past_one_grid_sweep(ctx):
    """two sessions so long that S * per exceeds one trip of the decrypt kernel's capped grid by a full workgroup and a ragged
    one: the whole output equals the ladder call's, and 24 OTs on both sides of the sweep edge and of the session edge equal
    the restatement's"""
    S = 2
    per = -(-(SWEEP + THREADS + 1) // S)
    n, id0 = S * per, (1 << 32) - 7
    assert n > SWEEP + THREADS and (n - SWEEP) % THREADS != 0 and per < SWEEP < n
    rng = np.random.default_rng(20250303)
    As = [co.mul(co.G, int.from_bytes(drbg("co_multi_base/sweep/a%d" % s, 32), "big") % co.N) for s in range(S)]
    sc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    ch = rng.integers(0, 2, n).astype(np.uint8)
    cts = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    A = engine._points(As)
    d_sc, d_ch, d_ct = ctx.to_device(sc), ctx.to_device(ch), ctx.to_device(cts)
    d_lab, d_lad = ctx.empty((n, 16)).zero(SENTINEL), ctx.empty((n, 16)).zero(SENTINEL)
    d_st, d_st2 = ctx.empty(4, np.uint64).zero(SENTINEL), ctx.empty(4, np.uint64).zero(SENTINEL)
    h = engine.CoMultiBase(ctx, A)
    h.decrypt_dev(d_sc, d_ch, d_ct, per, id0, d_lab, d_st)
    engine.co_multi_receiver_decrypt_dev(ctx, ctx.to_device(A), d_sc, d_ch, d_ct, S, per, id0, d_lad, d_st2)
    ctx.sync()
    h.close()
    assert status_of(d_st) == CLEAN and status_of(d_st2) == CLEAN
    labels, ladder = as_labels(d_lab), as_labels(d_lad)
    bad = np.flatnonzero(labels != ladder)
    assert bad.size == 0, "%d OTs differ from the ladder call, the first %d" % (bad.size, bad[0])
    idx = {0, n - 1} | set(range(per - 3, per + 3)) | set(range(SWEEP - 4, SWEEP + 4))
    while len(idx) < 24:
        idx.add(int(rng.integers(0, n)))
    for i in sorted(idx):
        s, j = divmod(i, per)
        c = bytes(cts[i])
        want = masks_xor(co.mul(As[s], int.from_bytes(bytes(sc[i]), "big")), id0 + j, c[16:] if ch[i] else c[:16])
        assert label_raw(labels[i:i + 1]) == [want], i


@pytest.mark.parametrize("bad_at,point", [(5, "x_equals_p"), (0, "infinity")])
def test_bad_sessions_inside_one_wave(ctx, sessions, bad_at, point):  # noqa: F811
    """(8, 8), 64 OTs: one wave, one of whose sessions has an A that is not a point of the curve"""
    S, per, id0 = 8, 8, 77
    n = S * per
    sess = sessions[:S]
    g = gather(sess, per)
    _, want_ct, want_labels, _ = expected(sess, per, id0)
    cts = ct_array(want_ct)
    A = g["A"].copy()
    assert not co.valid_point(HOSTILE[point])
    A[bad_at] = np.frombuffer(co.point_bytes(HOSTILE[point]), np.uint8)
    want = [bytes(16) if i // per == bad_at else want_labels[i] for i in range(n)]
    for h in (engine.CoMultiBase(ctx, A), engine.CoMultiBase(ctx, ctx.to_device(A), S)):
        assert h.info() == (S, 1, bad_at)
        labels, st = handle_dev(ctx, h, g["scalars"], g["choice"], cts, per, id0)
        assert st == [0, ONES, 1, bad_at]
        assert label_raw(labels) == want
        ladder, ladder_st = ladder_dev(ctx, A, g["scalars"], g["choice"], cts, S, per, id0)
        assert ladder_st == st and ladder.tobytes() == labels.tobytes()
        with pytest.raises(engine.CoSessionError) as e:
            h.decrypt(g["scalars"], g["choice"], cts, per, id0)
        assert e.value.code == engine.GC_E_POINT and e.value.bad_session == bad_at and "ot: point not on curve" in str(e.value)
        assert label_raw(e.value.out) == want  # every good label all the same
        h.close()


def test_reuse_and_lifetime(ctx, sessions):  # noqa: F811
    """one handle for two calls with different per and id0; two handles with different A arrays on one ctx, used alternately; a
    device call followed at once by free, which waits"""
    def case(sess, per, id0):
        g = gather(sess, per)
        _, want_ct, want_labels, _ = expected(sess, per, id0)
        return g, ct_array(want_ct), want_labels

    s1, s2 = sessions[:4], sessions[4:8]
    h1 = engine.CoMultiBase(ctx, gather(s1, 1)["A"])
    h2 = engine.CoMultiBase(ctx, gather(s2, 1)["A"])
    for h, sess, per, id0 in ((h1, s1, 3, 0), (h2, s2, 8, 9), (h1, s1, 65, (1 << 32) + 5), (h2, s2, 2, 1), (h1, s1, 3, 0)):
        g, cts, want = case(sess, per, id0)
        assert label_raw(h.decrypt(g["scalars"], g["choice"], cts, per, id0)) == want, (per, id0)
        labels, st = handle_dev(ctx, h, g["scalars"], g["choice"], cts, per, id0)
        assert st == CLEAN and label_raw(labels) == want, (per, id0)
    h2.close()
    g, cts, want = case(s1, 64, 7)
    d_lab, d_st = ctx.empty((4 * 64, 16)).zero(SENTINEL), ctx.empty(4, np.uint64).zero(SENTINEL)
    h1.decrypt_dev(ctx.to_device(g["scalars"]), ctx.to_device(g["choice"]), ctx.to_device(cts), 64, 7, d_lab, d_st)
    h1.close()  # no sync in between: the free waits for the stream
    h1.close()  # a second close is a no-op
    assert status_of(d_st) == CLEAN and label_raw(as_labels(d_lab)) == want


def test_go_pinned_session_between_two_others(ctx, sha_circ):
    """sha2pc's TestDeterministicTranscript as session 1 of 3 (tests/test_gpu_co_multi.py has the sender's side): the handle's
    labels are the evaluator's, the neighbours' as well"""
    dc = engine.DeviceCircuit(ctx, sha_circ)
    seen = {}

    def garble(key, rnd):
        g = dc.garble(key, rnd, batch=1)
        io = g["io"][0]
        seen["in"] = io[:512].copy()
        return {"in": io[:512], "out": io[512:]}, g["slab"][0]

    t = gt.transcript(sha_circ, garble, "transcript")
    dc.close()
    assert (t["round1"], t["round2"], t["round3"]) == gt.CASES["transcript"][1]
    session, bits = go_session()
    S, per = 3, 256
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
    assert bytes(A[1]) == co.point_bytes(session["A"])
    pts = engine.co_multi_receiver_choices(ctx, A, scalars, choice, S, per)
    ct = engine.co_multi_sender_encrypt(ctx, a, AaInv, pts, wires, S, per)
    assert ct_bytes(ct[per:2 * per]) == t["ciphertexts"]
    h = engine.CoMultiBase(ctx, A)
    labels = h.decrypt(scalars, choice, ct, per)
    h.close()
    assert (labels == pick(wires, choice)).all()


def test_misuse(ctx, sessions):  # noqa: F811
    L, p, vp = engine.lib(), engine._p, C.c_void_p
    E_ARG, OK = engine.GC_E_ARG, engine.GC_OK
    S, per = 2, 2
    n = S * per
    g = gather(sessions[:S], per)
    ct, out_lab = np.zeros((n, 32), np.uint8), np.zeros(n, LABEL)
    d = ctx.zeros(64 * n)
    q = vp(d.ptr)
    top = C.c_size_t(-1).value
    st = C.c_int(77)
    # create: NULL ctx, NULL array, S = 0, an S whose tables do not fit size_t; status may be NULL
    for fn, arr in ((L.gc_co_multi_base_create, p(g["A"])), (L.gc_co_multi_base_create_dev, q)):
        for args in ((None, arr, S), (ctx.h, None, S), (ctx.h, arr, 0), (ctx.h, arr, top // 61440 + 1), (ctx.h, arr, top)):
            st.value = 77
            assert not fn(*args, C.byref(st)) and st.value == E_ARG, (fn.__name__, args[2])
        assert not fn(None, None, 0, None)
    assert L.gc_co_multi_base_info(None, None, None, None) == E_ARG
    L.gc_co_multi_base_free(None)
    h = engine.CoMultiBase(ctx, g["A"])
    assert L.gc_co_multi_base_info(h.h, None, None, None) == OK  # any pointer may be NULL
    got_S = C.c_size_t(0)
    assert L.gc_co_multi_base_info(h.h, C.byref(got_S), None, None) == OK and got_S.value == S
    # host form: every pointer but bad_session, which may be NULL
    bad_s = C.c_size_t(98)
    good = [h.h, p(g["scalars"]), p(g["choice"]), p(ct), per, 0, p(out_lab), C.byref(bad_s)]
    assert L.gc_co_multi_base_decrypt(*good) == OK
    for k in (0, 1, 2, 3, 6):
        args = list(good)
        args[k] = None
        assert L.gc_co_multi_base_decrypt(*args) == E_ARG, k
    args = list(good)
    args[7] = None
    assert L.gc_co_multi_base_decrypt(*args) == OK and bad_s.value == 98
    # device form: every pointer, the status block included
    good_dev = [h.h, q, q, q, per, 0, q, q]
    for k in (0, 1, 2, 3, 6, 7):
        args = list(good_dev)
        args[k] = None
        assert L.gc_co_multi_base_decrypt_dev(*args) == E_ARG, k
    # S * per that overflows, and one whose 64 bytes per OT do
    for big in (top, top // 2 + 1, top // 128 + 1, 1 << 62):
        assert L.gc_co_multi_base_decrypt(h.h, p(g["scalars"]), p(g["choice"]), p(ct), big, 0, p(out_lab), None) == E_ARG
        assert L.gc_co_multi_base_decrypt_dev(h.h, q, q, q, big, 0, q, q) == E_ARG
    # per = 0: GC_OK with no other pointer; sentinel-filled outputs and status stay as they are; a NULL handle is refused
    d_lab, d_st = ctx.empty((n, 16)).zero(SENTINEL), ctx.empty(4, np.uint64).zero(SENTINEL)
    h_lab = np.full((n, 16), 0x77, np.uint8)
    assert L.gc_co_multi_base_decrypt_dev(h.h, q, q, q, 0, 3, vp(d_lab.ptr), vp(d_st.ptr)) == OK
    assert L.gc_co_multi_base_decrypt_dev(h.h, None, None, None, 0, 3, None, None) == OK
    assert L.gc_co_multi_base_decrypt(h.h, p(g["scalars"]), p(g["choice"]), p(ct), 0, 3, p(h_lab), C.byref(bad_s)) == OK
    assert L.gc_co_multi_base_decrypt(h.h, None, None, None, 0, 3, None, None) == OK
    assert L.gc_co_multi_base_decrypt(None, None, None, None, 0, 3, None, None) == E_ARG
    assert L.gc_co_multi_base_decrypt_dev(None, None, None, None, 0, 3, None, None) == E_ARG
    assert len(h.decrypt([], [], [], 0)) == 0
    ctx.sync()
    assert (d_lab.numpy() == SENTINEL).all() and (d_st.numpy().view(np.uint8) == SENTINEL).all()
    assert (h_lab == 0x77).all() and bad_s.value == 98 and (d.numpy() == 0).all()
    h.close()
    assert L.gc_abi_version() == 2


def test_create_inside_a_capture_is_refused(sessions):  # noqa: F811
    """create allocates and waits for the stream: not between gc_ctx_capture_begin and _end.  The ctx stays usable."""
    c = engine.Context(0)
    S, per, id0 = 2, 2, 5
    g = gather(sessions[:S], per)
    d_A = c.to_device(g["A"])
    for make in (lambda: engine.CoMultiBase(c, g["A"]), lambda: engine.CoMultiBase(c, d_A, S)):
        with pytest.raises(engine.EngineError) as e:
            c.capture(make)
        assert e.value.code == engine.GC_E_ARG
    c.sync()
    _, want_ct, want_labels, _ = expected(sessions[:S], per, id0)
    h = engine.CoMultiBase(c, d_A, S)
    assert label_raw(h.decrypt(g["scalars"], g["choice"], ct_array(want_ct), per, id0)) == want_labels
    h.close()
    c.close()
