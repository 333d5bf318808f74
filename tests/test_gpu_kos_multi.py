"""The KOS check of the malicious IKNP variant for S sessions per call (gc_kos_multi_*; mpc_amd/csrc/kos_multi_kernels.hip,
kos_multi.h) byte for byte against the C oracle run on every session ALONE: oracle.kos_receiver_tags / kos_sender_check.
Sessions have different seeded seed2, delta and labels.  Whole output buffers are compared, and every device output lies
between two sentinel words.

The sizes are the smallest at which the named thing can go wrong, derived from the constants of kernels.h: sessions shorter
than a byte of choice bits and across one; per + 256 at the threshold between a wave per session and a workgroup per session,
one below and one above; more sessions than workgroups, so that a workgroup holds several wave teams; one session more than a
sweep of the grid covers, for both team sizes."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from mpc_amd import engine
from mpc_amd.circuit import LABEL
from tests.test_gpu_iknp_multi import OracleSessions, make_sessions, pack_choice, u_bytes
from tests.test_gpu_ot_sweeps import GUARD, SENTINEL, Guarded, label_u8, rand_labels, tup, xor_where
from tests.util import kernel_constants

pytestmark = pytest.mark.gpu

THREADS, GRID, WAVE_MAX = kernel_constants("kKosMultiThreads", "kKosMultiGrid", "kKosMultiWaveMax")
WAVE_SWEEP = GRID * (THREADS // 64)  # sessions one sweep covers with a wave per session
WG_SWEEP = GRID                      # ... with a workgroup per session
PER_WG = WAVE_MAX - 256 + 1          # the smallest per that takes a workgroup per session
NONE = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


class GuardedBytes:
    """Guarded for an output of any byte length"""

    def __init__(self, ctx, nbytes):
        self.n = nbytes
        self.buf = ctx.empty(nbytes + 2 * GUARD).zero(SENTINEL)
        self.ptr = self.buf + GUARD

    def read(self):
        raw = self.buf.numpy()
        assert (raw[:GUARD] == SENTINEL).all(), "the bytes before the output were written"
        assert (raw[GUARD + self.n:] == SENTINEL).all(), "the bytes behind the output were written"
        return raw[GUARD:GUARD + self.n].copy()


class Case:
    """S honest sessions of per OTs (the receiver's labels are the sender's ^ choice * delta_s) and the oracle's tags"""

    def __init__(self, seed, S, per):
        rng = np.random.default_rng(seed)
        self.S, self.per = S, per
        self.seed2, self.delta = rand_labels(rng, S), rand_labels(rng, S)
        self.b = rng.integers(0, 2, (S, per)).astype(np.uint8)
        self.bcv = rng.integers(0, 2, (S, 256)).astype(np.uint8)
        self.sent, self.cvs = rand_labels(rng, S * per).reshape(S, per), rand_labels(rng, S * 256).reshape(S, 256)
        self.result, self.cv = self.sent.copy(), self.cvs.copy()
        for s in range(S):
            self.result[s] = xor_where(self.sent[s], self.b[s], tup(self.delta[s]))
            self.cv[s] = xor_where(self.cvs[s], self.bcv[s], tup(self.delta[s]))
        self.tags = np.zeros((S, 3), LABEL)
        for s in range(S):
            x, t0, t1 = oracle.kos_receiver_tags(tup(self.seed2[s]), self.result[s], self.b[s], self.cv[s], self.bcv[s])
            for k, v in enumerate((x, t0, t1)):
                self.tags[s, k]["d0"], self.tags[s, k]["d1"] = v

    def oracle_ok(self, sent=None, cvs=None, tags=None):
        sent = self.sent if sent is None else sent
        cvs = self.cvs if cvs is None else cvs
        tags = self.tags if tags is None else tags
        return np.array([oracle.kos_sender_check(tup(self.seed2[s]), sent[s], cvs[s], tup(self.delta[s]), tup(tags[s, 0]),
                                                 tup(tags[s, 1]), tup(tags[s, 2])) for s in range(self.S)], np.uint8)


@functools.lru_cache(maxsize=None)
def case(seed, S, per):
    """computed once and shared; the tests copy what they change"""
    return Case(seed, S, per)


def pack_bcv(bcv, ones=False):
    out = np.full((len(bcv), 64), 0xff if ones else 0, np.uint8)
    out[:, :32] = np.packbits(bcv, axis=1, bitorder="little")
    return out


def pack_b(b, S, per, ones=False):
    out = pack_choice(b, S, per) if per else np.zeros((S, 0), np.uint8)
    if ones and per:
        pad = np.ones((S, out.shape[1] * 8), np.uint8)
        pad[:, :per] = b
        out = np.packbits(pad, axis=1, bitorder="little")
    return out


def tags_dev(ctx, c, result=None, ones=False):
    S, per = c.S, c.per
    d = [ctx.to_device(label_u8(c.seed2)), ctx.to_device(label_u8(c.result if result is None else result)),
         ctx.to_device(pack_b(c.b, S, per, ones).reshape(-1)), ctx.to_device(label_u8(c.cv)),
         ctx.to_device(pack_bcv(c.bcv, ones).reshape(-1))]
    g = Guarded(ctx, 48 * S)
    engine.kos_multi_receiver_tags_dev(ctx, d[0], d[1] if per else None, d[2] if per else None, d[3], d[4], S, per, g.ptr)
    ctx.sync()
    return np.frombuffer(g.read().tobytes(), LABEL).reshape(S, 3)


def check_dev(ctx, c, sent=None, cvs=None, tags=None):
    """-> (ok [S], status [2])"""
    S, per = c.S, c.per
    d = [ctx.to_device(label_u8(c.seed2)), ctx.to_device(label_u8(c.sent if sent is None else sent)),
         ctx.to_device(label_u8(c.cvs if cvs is None else cvs)), ctx.to_device(label_u8(c.delta)),
         ctx.to_device(label_u8(c.tags if tags is None else tags))]
    g_ok, g_st = GuardedBytes(ctx, S), Guarded(ctx, 16)
    engine.kos_multi_sender_check_dev(ctx, d[0], d[1] if per else None, d[2], d[3], d[4], S, per, g_ok.ptr, g_st.ptr)
    ctx.sync()
    return g_ok.read(), [int(v) for v in np.frombuffer(g_st.read().tobytes(), np.uint64)]


def check_both_roles(ctx, c, forms=("host", "dev")):
    S, per = c.S, c.per
    if S <= 17:
        assert c.oracle_ok().all(), "the oracle's sender accepts the oracle's tags of an honest run"
    if "host" in forms:
        got = engine.kos_multi_receiver_tags(ctx, c.seed2, c.result, c.b, c.cv, c.bcv, S, per)
        assert got.tobytes() == c.tags.tobytes()
        ok, bad = engine.kos_multi_sender_check(ctx, c.seed2, c.sent, c.cvs, c.delta, c.tags, S, per)
        assert ok.tolist() == [1] * S and bad is None
    if "dev" in forms:
        assert tags_dev(ctx, c).tobytes() == c.tags.tobytes()
        ok, st = check_dev(ctx, c)
        assert ok.tolist() == [1] * S and st == [0, NONE]


@pytest.mark.parametrize("per", [0, 1, 127, 128, 129])
def test_short_sessions(ctx, per):
    check_both_roles(ctx, case(1, 3, per))


def test_padding_of_the_packed_choice_bits_reaches_no_output(ctx):
    for per in (1, 127, 129):
        c = case(1, 3, per)
        assert tags_dev(ctx, c, ones=True).tobytes() == c.tags.tobytes()


@pytest.mark.parametrize("S", [2, 17, GRID + 1])
@pytest.mark.parametrize("n", [WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1])
def test_team_thresholds(ctx, S, n):
    """a wave per session up to per + 256 = kKosMultiWaveMax, a workgroup above; with S = kKosMultiGrid + 1 workgroup 0 holds
    two wave teams (or takes a second trip as a workgroup team) and every other workgroup one"""
    assert n - 256 > 0 and (n > WAVE_MAX) == (n - 256 >= PER_WG)
    check_both_roles(ctx, case(2, S, n - 256), forms=("dev",) if S > 17 else ("host", "dev"))


def test_past_one_grid_sweep_with_wave_teams(ctx):
    S = WAVE_SWEEP + 1
    assert 1 + 256 <= WAVE_MAX
    check_both_roles(ctx, case(3, S, 1), forms=("dev",))


def test_past_one_grid_sweep_with_workgroup_teams(ctx):
    S = WG_SWEEP + 1
    assert PER_WG + 256 > WAVE_MAX
    check_both_roles(ctx, case(3, S, PER_WG), forms=("dev",))


def flip(a, s, k=0, bit=1, field="d0"):
    out = a.copy()
    out[field][s, k] ^= np.uint64(bit)
    return out


FLIPS = {
    "t0": lambda c, s: dict(tags=flip(c.tags, s, 1, 1 << 7)),
    "t1": lambda c, s: dict(tags=flip(c.tags, s, 2, 1 << 63, "d1")),
    "x": lambda c, s: dict(tags=flip(c.tags, s, 0, 2)),
    "result": lambda c, s: dict(sent=flip(c.sent, s, 77, 1 << 40)),
    "choice_vec": lambda c, s: dict(cvs=flip(c.cvs, s, 255, 1, "d1")),
}


def merged(c, sessions, what):
    kw = {}
    for s in sessions:
        for k, v in FLIPS[what](c, s).items():
            base = kw.get(k, getattr(c, k))
            base = base.copy()
            base[s] = v[s]
            kw[k] = base
    return kw


@pytest.mark.parametrize("what", sorted(FLIPS))
def test_a_failing_session_is_named(ctx, what):
    c = case(4, 5, 129)
    ok, st = check_dev(ctx, c)
    assert ok.tolist() == [1] * 5 and st == [0, NONE]
    ok, bad = engine.kos_multi_sender_check(ctx, c.seed2, c.sent, c.cvs, c.delta, c.tags, 5, 129)
    assert ok.tolist() == [1] * 5 and bad is None
    for sessions, want_ok, want_st in (((3,), [1, 1, 1, 0, 1], [1, 3]), ((1, 4), [1, 0, 1, 1, 0], [2, 1])):
        kw = merged(c, sessions, what)
        assert c.oracle_ok(**kw).tolist() == want_ok
        ok, st = check_dev(ctx, c, **kw)
        assert ok.tolist() == want_ok and st == want_st
        ok, bad = engine.kos_multi_sender_check(ctx, c.seed2, kw.get("sent", c.sent), kw.get("cvs", c.cvs), c.delta,
                                                kw.get("tags", c.tags), 5, 129)
        assert ok.tolist() == want_ok and bad == want_st[1]
        # either output of the host form may be left out
        L, p = engine.lib(), lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
        arrs = [np.ascontiguousarray(a) for a in (c.seed2, kw.get("sent", c.sent), kw.get("cvs", c.cvs), c.delta,
                                                  kw.get("tags", c.tags))]
        only_ok, only_bad = np.zeros(5, np.uint8), C.c_size_t(0)
        assert L.gc_kos_multi_sender_check(ctx.h, *[p(a) for a in arrs], 5, 129, p(only_ok), None) == engine.GC_OK
        assert L.gc_kos_multi_sender_check(ctx.h, *[p(a) for a in arrs], 5, 129, None, C.byref(only_bad)) == engine.GC_OK
        assert only_ok.tolist() == want_ok and only_bad.value == want_st[1]


def test_end_to_end_on_the_device(ctx):
    """the malicious flow of both roles on buffers that never leave the device: extend at per, extend the random choice vector
    at 256, tags, check.  Then one byte of session 2's u is changed on its way to the sender."""
    S, per = 4, 130
    rng, base, deltas, k0 = make_sessions(11, S)
    b = rng.integers(0, 2, (S, per)).astype(np.uint8)
    bcv = rng.integers(0, 2, (S, 256)).astype(np.uint8)
    seed2 = rand_labels(rng, S)
    orc = OracleSessions(base, deltas, k0)
    _, got, _ = orc.call(b, per)
    _, cv, _ = orc.call(bcv, 256)
    want = np.zeros((S, 3), LABEL)
    for s in range(S):
        tags = oracle.kos_receiver_tags(tup(seed2[s]), got[s * per:(s + 1) * per], b[s], cv[s * 256:(s + 1) * 256], bcv[s])
        for k, v in enumerate(tags):
            want[s, k]["d0"], want[s, k]["d1"] = v

    d_seed2, d_delta = ctx.to_device(label_u8(seed2)), ctx.to_device(label_u8(deltas))
    d_choice, d_bcv = ctx.to_device(pack_choice(b, S, per)), ctx.to_device(pack_choice(bcv, S, 256))
    rcv = engine.IKNPMultiReceiver(ctx, base)
    d_u, d_u2 = ctx.empty(S * u_bytes(per)), ctx.empty(S * u_bytes(256))
    d_res, d_cv = ctx.empty(16 * S * per), ctx.empty(16 * S * 256)
    g_tags = Guarded(ctx, 48 * S)
    rcv.receive_dev(d_choice, per, d_u, d_res)
    rcv.receive_dev(d_bcv, 256, d_u2, d_cv)
    engine.kos_multi_receiver_tags_dev(ctx, d_seed2, d_res, d_choice, d_cv, d_bcv, S, per, g_tags.ptr)
    ctx.sync()
    assert g_tags.read().tobytes() == want.tobytes()
    rcv.close()

    col = next(i for i in range(64) if (int(deltas[2]["d0"]) >> i) & 1)
    u = d_u.numpy().copy()
    u_bad = u.copy()
    u_bad[2 * u_bytes(per) + col * ((per + 7) // 8)] ^= 0x10
    for u_in, want_ok, want_st in ((u, [1, 1, 1, 1], [0, NONE]), (u_bad, [1, 1, 0, 1], [1, 2])):
        snd = engine.IKNPMultiSender(ctx, deltas, k0)
        d_u.upload(u_in)
        d_q, d_qcv = ctx.empty(16 * S * per), ctx.empty(16 * S * 256)
        g_ok, g_st = GuardedBytes(ctx, S), Guarded(ctx, 16)
        snd.send_dev(d_u, per, d_q)
        snd.send_dev(d_u2, 256, d_qcv)
        engine.kos_multi_sender_check_dev(ctx, d_seed2, d_q, d_qcv, d_delta, g_tags.ptr, S, per, g_ok.ptr, g_st.ptr)
        ctx.sync()
        assert g_ok.read().tolist() == want_ok
        assert [int(v) for v in np.frombuffer(g_st.read().tobytes(), np.uint64)] == want_st
        snd.close()


def test_both_dev_calls_are_captured_and_replayed(ctx):
    S, per = 3, 129
    a, b = case(1, S, per), case(5, S, per)
    b_bad = merged(b, (1,), "result")["sent"]
    d_seed2, d_res, d_choice = ctx.empty(16 * S), ctx.empty(16 * S * per), ctx.empty(S * 64)
    d_cv, d_bcv, d_sent, d_cvs, d_delta = ctx.empty(16 * S * 256), ctx.empty(S * 64), ctx.empty(16 * S * per), \
        ctx.empty(16 * S * 256), ctx.empty(16 * S)
    g_tags, g_ok, g_st = Guarded(ctx, 48 * S), GuardedBytes(ctx, S), Guarded(ctx, 16)

    def load(c, sent):
        for d, v in ((d_seed2, c.seed2), (d_res, c.result), (d_choice, pack_b(c.b, S, per)), (d_cv, c.cv),
                     (d_bcv, pack_bcv(c.bcv)), (d_sent, sent), (d_cvs, c.cvs), (d_delta, c.delta)):
            d.upload(label_u8(v))

    def calls():
        engine.kos_multi_receiver_tags_dev(ctx, d_seed2, d_res, d_choice, d_cv, d_bcv, S, per, g_tags.ptr)
        engine.kos_multi_sender_check_dev(ctx, d_seed2, d_sent, d_cvs, d_delta, g_tags.ptr, S, per, g_ok.ptr, g_st.ptr)

    load(a, a.sent)
    graph = ctx.capture(calls)
    try:
        for c, sent, want_ok, want_st in ((b, b_bad, [1, 0, 1], [1, 1]), (a, a.sent, [1, 1, 1], [0, NONE])):
            load(c, sent)
            graph.launch()
            ctx.sync()
            assert g_tags.read().tobytes() == c.tags.tobytes()
            assert g_ok.read().tolist() == want_ok
            assert [int(v) for v in np.frombuffer(g_st.read().tobytes(), np.uint64)] == want_st
    finally:
        graph.close()


def test_argument_errors(ctx):
    S, per = 3, 8
    c = case(6, S, per)
    L, E = engine.lib(), engine.GC_E_ARG
    d = ctx.empty(16 * S * 256 + 64).zero()
    P = d.ptr
    g_tags, g_ok, g_st = Guarded(ctx, 48 * S), GuardedBytes(ctx, S), Guarded(ctx, 16)
    tags_args = [P, P, P, P, P]
    check_args = [P, P, P, P, P]
    # a NULL ctx; a NULL array that is needed
    assert L.gc_kos_multi_receiver_tags_dev(None, *tags_args, S, per, g_tags.ptr) == E
    assert L.gc_kos_multi_sender_check_dev(None, *check_args, S, per, g_ok.ptr, g_st.ptr) == E
    for k in range(5):
        a = list(tags_args)
        a[k] = None
        assert L.gc_kos_multi_receiver_tags_dev(ctx.h, *a, S, per, g_tags.ptr) == E, k
        a = list(check_args)
        a[k] = None
        assert L.gc_kos_multi_sender_check_dev(ctx.h, *a, S, per, g_ok.ptr, g_st.ptr) == E, k
    assert L.gc_kos_multi_receiver_tags_dev(ctx.h, *tags_args, S, per, None) == E
    assert L.gc_kos_multi_sender_check_dev(ctx.h, *check_args, S, per, None, g_st.ptr) == E
    assert L.gc_kos_multi_sender_check_dev(ctx.h, *check_args, S, per, g_ok.ptr, None) == E
    # a label pointer that is not 16-byte aligned (the packed choice bits are read byte by byte and may lie anywhere)
    for k in (0, 1, 3):
        a = list(tags_args)
        a[k] = P + 8
        assert L.gc_kos_multi_receiver_tags_dev(ctx.h, *a, S, per, g_tags.ptr) == E, k
    assert L.gc_kos_multi_receiver_tags_dev(ctx.h, *tags_args, S, per, g_tags.ptr + 8) == E
    for k in range(5):
        a = list(check_args)
        a[k] = P + 8
        assert L.gc_kos_multi_sender_check_dev(ctx.h, *a, S, per, g_ok.ptr, g_st.ptr) == E, k
    assert L.gc_kos_multi_sender_check_dev(ctx.h, *check_args, S, per, g_ok.ptr, g_st.ptr + 4) == E
    # a size that does not fit size_t
    for big_S, big_per in ((1 << 62, 8), (3, 1 << 62), (1 << 33, 1 << 33), (1 << 60, 0)):
        assert L.gc_kos_multi_receiver_tags_dev(ctx.h, *tags_args, big_S, big_per, g_tags.ptr) == E
        assert L.gc_kos_multi_sender_check_dev(ctx.h, *check_args, big_S, big_per, g_ok.ptr, g_st.ptr) == E
    # the host forms: NULL arrays, both outputs of the check left out
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    host = [p(c.seed2), p(c.sent), p(c.cvs), p(c.delta), p(c.tags)]
    assert L.gc_kos_multi_sender_check(ctx.h, *host, S, per, None, None) == E
    for k in range(5):
        a = list(host)
        a[k] = None
        assert L.gc_kos_multi_sender_check(ctx.h, *a, S, per, p(np.zeros(S, np.uint8)), None) == E, k
    rhost = [p(c.seed2), p(c.result), p(c.b), p(c.cv), p(c.bcv)]
    out = np.zeros((S, 3), LABEL)
    for k in range(5):
        a = list(rhost)
        a[k] = None
        assert L.gc_kos_multi_receiver_tags(ctx.h, *a, S, per, p(out)) == E, k
    assert L.gc_kos_multi_receiver_tags(ctx.h, *rhost, S, per, None) == E
    # S = 0 is GC_OK and writes nothing; nothing above wrote anything either
    assert L.gc_kos_multi_receiver_tags_dev(ctx.h, None, None, None, None, None, 0, per, None) == engine.GC_OK
    assert L.gc_kos_multi_sender_check_dev(ctx.h, None, None, None, None, None, 0, per, None, None) == engine.GC_OK
    assert L.gc_kos_multi_receiver_tags(ctx.h, None, None, None, None, None, 0, per, None) == engine.GC_OK
    assert L.gc_kos_multi_sender_check(ctx.h, None, None, None, None, None, 0, per, None, None) == engine.GC_OK
    ctx.sync()
    assert (g_tags.read() == SENTINEL).all() and (g_ok.read() == SENTINEL).all() and (g_st.read() == SENTINEL).all()
    # per = 0 with the per-OT arrays NULL is valid (test_short_sessions compares its values)
    z = case(1, 3, 0)
    got = engine.kos_multi_receiver_tags(ctx, z.seed2, z.result, z.b, z.cv, z.bcv, 3, 0)
    assert got.tobytes() == z.tags.tobytes()
