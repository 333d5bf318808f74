"""Bit-COT for S sessions per call (gc_iknp_multi_*_bits*; mpc_amd/csrc/iknp_multi_bits_kernels.hip, iknp_multi_bits.h) and
the triple folds over S peers (gc_gmw_triples_multi_*) byte for byte against the C oracle run on every session ALONE
(oracle.iknp_receive_bits / iknp_send_bits on one oracle.IKNPReceiver / IKNPSender pair per session).  Whole buffers are
compared; every device output lies between sentinel words and starts out filled with non-zero bytes, so a result word the
kernel did not write shows.  Every sender case holds sessions with Delta.Bit(0) = 0 and = 1.

The sizes are the smallest at which the named thing can go wrong: sessions shorter than a chunk, a word, a byte; a trailing
partial choice word that must not enter u; a ragged chunk of exactly one word; stream positions off a block boundary in
every arm of the shift; label calls between bit calls; every form of the choice stride; a second, ragged step of workgroup 0
of each capped grid (derived from kernels.h); a whole triple batch for 2, 3 and 5 parties."""
import ctypes as C

import numpy as np
import pytest

import oracle
from mpc_amd import engine
from tests.test_gpu_iknp_multi import OracleSessions, chunks, make_sessions, receive_dev, send_dev, tup, u_bytes
from tests.test_gpu_ot_sweeps import Guarded, SENTINEL
from tests.util import kernel_constants

pytestmark = pytest.mark.gpu

MULTI_GRID, RECV_ITEMS = kernel_constants("kIknpMultiGrid", "kIknpRecvChunks")
SEND_THREADS, SEND_GRID = kernel_constants("kIknpBitsSendThreads", "kIknpBitsSendGrid")
FOLD_THREADS, FOLD_GRID = kernel_constants("kGmwMultiFoldThreads", "kGmwMultiFoldGrid")
CHUNK = 512


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


def W(per):
    return -(-per // 64)


def advance(per):
    return (per // CHUNK) * 64 + (per % CHUNK + 7) // 8


def rand_words(rng, shape):
    return rng.integers(0, 0xFFFFFFFFFFFFFFFF, shape, dtype=np.uint64, endpoint=True)


class GuardedWords:
    """`words` u64 of device output in a Guarded buffer; the bytes that pad it to Guarded's 16 are sentinels too"""

    def __init__(self, ctx, words, data=None):
        self.n = 8 * words
        full = -(-self.n // 16) * 16
        if data is not None:
            data = np.concatenate([np.ascontiguousarray(data, np.uint64).view(np.uint8), np.full(full - self.n, SENTINEL, np.uint8)])
        self.g = Guarded(ctx, full, data)
        self.ptr = self.g.ptr

    def read(self):
        raw = self.g.read()
        assert (raw[self.n:] == SENTINEL).all(), "the word behind the output was written"
        return raw[:self.n].view(np.uint64)


def force_delta_bit0(deltas, base):
    """sessions 0 and 1 get Delta.Bit(0) = 0 and 1 (three random deltas can share the bit); k0 follows"""
    from tests.test_gpu_iknp_multi import delta_bits
    deltas = deltas.copy()
    deltas["d0"][0] &= np.uint64(0xFFFFFFFFFFFFFFFE)
    if len(deltas) > 1:
        deltas["d0"][1] |= np.uint64(1)
    return deltas, np.where(delta_bits(deltas), base["l1"], base["l0"])


def sessions(seed, S):
    rng, base, deltas, _ = make_sessions(seed, S)
    deltas, k0 = force_delta_bit0(deltas, base)
    assert S == 1 or (int(deltas["d0"][0]) & 1, int(deltas["d0"][1]) & 1) == (0, 1)
    return rng, base, deltas, k0


def oracle_bits(orc, ch, per):
    """one bits call on every session of an OracleSessions alone: ch [S, W] -> (u of all sessions, r [S, W], s [S, W])"""
    us, rs, ss = [], [], []
    for s in range(orc.S):
        u, r = oracle.iknp_receive_bits(orc.rcv[s], ch[s], per)
        assert len(u) == u_bytes(per)
        us.append(u)
        rs.append(r.copy())
        ss.append(oracle.iknp_send_bits(orc.snd[s], u, per).copy())
    return b"".join(us), np.stack(rs), np.stack(ss)


def receive_bits_dev(ctx, rcv, flat, stride, S, per):
    """flat: the choice words as the call reads them; exactly as many as it may read, so a read past them leaves the buffer"""
    d_ch = ctx.to_device(np.ascontiguousarray(flat, np.uint64))
    g_u, g_r = Guarded(ctx, S * u_bytes(per)), GuardedWords(ctx, S * W(per))
    rcv.receive_bits_dev(d_ch, stride, per, g_u.ptr, g_r.ptr)
    ctx.sync()
    return g_u.read().tobytes(), g_r.read().reshape(S, W(per)).copy()


def send_bits_dev(ctx, snd, u, S, per):
    d_u = ctx.to_device(np.frombuffer(u, np.uint8))
    g_s = GuardedWords(ctx, S * W(per))
    snd.send_bits_dev(d_u, per, g_s.ptr)
    ctx.sync()
    return g_s.read().reshape(S, W(per)).copy()


def check_bit_calls(ctx, seed, S, pers, forms=("host", "dev")):
    """one pair of handles per form, the bit calls of `pers` one after the other, against one oracle pair per session"""
    rng, base, deltas, k0 = sessions(seed, S)
    orc, want = OracleSessions(base, deltas, k0), []
    for per in pers:
        ch = rand_words(rng, (S, W(per)))
        want.append((per, ch) + oracle_bits(orc, ch, per) + (orc.pos(),))
    for form in forms:
        rcv, snd = engine.IKNPMultiReceiver(ctx, base), engine.IKNPMultiSender(ctx, deltas, k0)
        for per, ch, u, r, s, pos in want:
            what = "%s form, S = %d, per = %d" % (form, S, per)
            if form == "host":
                have_u, have_r = rcv.receive_bits(ch, per)
                have_s = snd.send_bits(u, per)  # the sender is fed the ORACLE's u
            else:
                have_u, have_r = receive_bits_dev(ctx, rcv, ch, W(per), S, per)
                have_s = send_bits_dev(ctx, snd, u, S, per)
            assert have_u == u, "u differs from the oracle's (%s)" % what
            assert have_r.tobytes() == r.tobytes(), "the receiver's bits differ from the oracle's (%s)" % what
            assert have_s.tobytes() == s.tobytes(), "the sender's bits differ from the oracle's (%s)" % what
            assert rcv.pos == pos and snd.pos == pos, what
        rcv.close()
        snd.close()


# ---- 1, 2: short sessions, several chunks ------------------------------------------------------------------------------


@pytest.mark.parametrize("per", [128, 127, 100, 64, 37, 1])
def test_short_sessions(ctx, per):
    """two whole words; 127: one bit of tail; 100: 13 byte rows, so one choice word enters u and 36 choice bits must not; one
    word exactly; 37: no choice word enters u at all; one OT"""
    check_bit_calls(ctx, 20250101 + per, 3, [per])


@pytest.mark.parametrize("per", [549, 576, 1024])
def test_several_chunks(ctx, per):
    """a full chunk plus 37 rows; plus a ragged chunk of exactly one word; two full chunks"""
    check_bit_calls(ctx, 20250102 + per, 3, [per])


# ---- 3: the stream position ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("variant", ["default", "generic"])
def test_stream_position_across_calls(ctx, monkeypatch, variant):
    """40 OTs leave column 0 five bytes into a block: the sender's lanes of the next calls take two blocks each.  generic:
    the general counter form (GC_IKNP_GENERIC=1), which both new kernels honour"""
    if variant == "generic":
        monkeypatch.setenv("GC_IKNP_GENERIC", "1")
    check_bit_calls(ctx, 20250103, 3, [40, 128, 549])


def test_every_arm_of_the_misaligned_shift(ctx):
    """the calls start at byte 0, 12, 19, 24 and 93 of every column stream: every dword selection of the byte shift, with and
    without a byte part (tests/test_gpu_iknp_multi.py: test_every_arm_of_the_misaligned_shift)"""
    pers = [96, 56, 40, 549, 128]
    starts = [0]
    for per in pers:
        starts.append(starts[-1] + advance(per))
    assert [p % 16 for p in starts[:5]] == [0, 12, 3, 8, 13]
    check_bit_calls(ctx, 20250104, 3, pers)


def test_bit_calls_and_label_calls_mixed_on_one_handle(ctx):
    """bits(96), labels(56) through gc_iknp_multi_receive_dev / _send_dev, bits(549): the oracle sessions do the same, and the
    position is checked after every call"""
    S = 3
    rng, base, deltas, k0 = sessions(20250105, S)
    orc = OracleSessions(base, deltas, k0)
    rcv, snd = engine.IKNPMultiReceiver(ctx, base), engine.IKNPMultiSender(ctx, deltas, k0)
    pos = 0
    for kind, per in (("bits", 96), ("labels", 56), ("bits", 549)):
        if kind == "bits":
            ch = rand_words(rng, (S, W(per)))
            u, r, s = oracle_bits(orc, ch, per)
            have_u, have_r = receive_bits_dev(ctx, rcv, ch, W(per), S, per)
            have_s = send_bits_dev(ctx, snd, u, S, per)
            assert have_u == u and have_r.tobytes() == r.tobytes() and have_s.tobytes() == s.tobytes(), (kind, per)
        else:
            b = rng.integers(0, 2, (S, per)).astype(np.uint8)
            u, got, sent = orc.call(b, per)
            have_u, have_got = receive_dev(ctx, rcv, b, S, per)
            assert have_u == u and have_got == got.tobytes() and send_dev(ctx, snd, u, S, per) == sent.tobytes(), (kind, per)
        pos += advance(per)
        assert rcv.pos == snd.pos == orc.pos() == pos, (kind, per)
    rcv.close()
    snd.close()


# ---- 4: the choice stride ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("per", [100, 549])
def test_choice_stride(ctx, per):
    """stride 0 = stride W with the row replicated; stride W + 3 with random words in the gaps = the per-session result.  The
    device buffer ends with the last word the call may read"""
    S, Wd = 3, W(per)
    rng, base, deltas, k0 = sessions(20250106 + per, S)
    shared, rows, gaps = rand_words(rng, Wd), rand_words(rng, (S, Wd)), rand_words(rng, (S, Wd + 3))
    gaps[:, :Wd] = rows
    flat = gaps.reshape(-1)[:(S - 1) * (Wd + 3) + Wd]

    def fresh():
        return OracleSessions(base, deltas, k0)

    u0, r0, _ = oracle_bits(fresh(), np.tile(shared, (S, 1)), per)
    u1, r1, _ = oracle_bits(fresh(), rows, per)
    for form in ("host", "dev"):
        for what, words, stride, u, r in (("shared", shared, 0, u0, r0), ("replicated", np.tile(shared, (S, 1)), Wd, u0, r0),
                                          ("gaps", flat, Wd + 3, u1, r1)):
            rcv = engine.IKNPMultiReceiver(ctx, base)
            if form == "host":
                have_u, have_r = rcv.receive_bits(words, per, stride=stride)
            else:
                have_u, have_r = receive_bits_dev(ctx, rcv, words.reshape(-1), stride, S, per)
            assert have_u == u and have_r.tobytes() == r.tobytes(), (form, what)
            assert rcv.pos == advance(per)
            rcv.close()


# ---- 5: past one trip of each capped grid ----------------------------------------------------------------------------------


def test_receiver_past_one_trip(ctx):
    """per = 549 is a full chunk and one of 37 rows per session and a step takes RECV_ITEMS: the smallest S at which workgroup
    0 has a second step, and that step is ragged.  The second step also uses the second set of hand-over buffers"""
    per, S = 549, MULTI_GRID * RECV_ITEMS // 2 + 1
    items = S * chunks(per)
    steps = -(-items // RECV_ITEMS)
    assert chunks(per) == 2 and steps == MULTI_GRID + 1 and items % RECV_ITEMS == 2
    assert (S - 1) * chunks(per) <= MULTI_GRID * RECV_ITEMS
    rng, base, deltas, k0 = sessions(20250107, S)
    ch = rand_words(rng, (S, W(per)))
    us, rs = [], []
    for s in range(S):  # the oracle receiver of a session dropped as soon as it has run (oracle_once)
        u, r = oracle.iknp_receive_bits(oracle.IKNPReceiver(base[s]), ch[s], per)
        us.append(u), rs.append(r.copy())
    rcv = engine.IKNPMultiReceiver(ctx, base)
    have_u, have_r = receive_bits_dev(ctx, rcv, ch, W(per), S, per)
    assert have_u == b"".join(us), "u differs from the oracle's"
    assert have_r.tobytes() == np.stack(rs).tobytes(), "the receiver's bits differ from the oracle's"
    rcv.close()


def test_sender_past_one_trip(ctx):
    """per = 549 is five lanes per session (W = 9) and a trip of the grid is SEND_GRID * SEND_THREADS lanes: the smallest S at
    which workgroup 0 has a second trip, and that trip is ragged.  The sender takes any bytes for u, so u is random here and
    the oracle SENDER of every session alone gives the expected words: no oracle receiver has to run for each of the
    sessions (per = 37, one lane per session, would need five times as many)"""
    per = 549
    lanes_per = (W(per) + 1) // 2
    sweep = SEND_GRID * SEND_THREADS
    S = sweep // lanes_per + 1
    assert lanes_per == 5 and S * lanes_per > sweep >= (S - 1) * lanes_per and (S * lanes_per - sweep) < SEND_THREADS
    rng, base, deltas, k0 = sessions(20250108, S)
    ub = u_bytes(per)
    u = rng.integers(0, 256, S * ub, dtype=np.uint8)
    want = np.stack([oracle.iknp_send_bits(oracle.IKNPSender(tup(deltas[s]), k0[s]), u[s * ub:(s + 1) * ub], per).copy()
                     for s in range(S)])
    snd = engine.IKNPMultiSender(ctx, deltas, k0)
    have = send_bits_dev(ctx, snd, u.tobytes(), S, per)
    assert have.tobytes() == want.tobytes(), "the sender's bits differ from the oracle's"
    snd.close()


# ---- 6: a triple batch end to end ------------------------------------------------------------------------------------------


def pair_setup(seed, s, r):
    """the base labels tests/test_gpu_gmw.py: _device_triples gives the ordered pair (sender s, receiver r)"""
    from tests.test_gpu_ot import base_setup
    return base_setup("gmw-%d-%d-%d" % (seed, s, r))


def multi_triples(ctx, P, words, seed, a, b):
    """tripleBatch of every party with its P - 1 peer sessions in one multi handle per role: one receive-bits with the shared
    b (stride 0), one send-bits, three folds.  The u-matrices cross between the parties as device buffers."""
    n = 64 * words
    ub = u_bytes(n)
    S = P - 1
    peers = [[q for q in range(P) if q != p] for p in range(P)]
    rcvs, snds = [], []
    for p in range(P):
        base = np.stack([pair_setup(seed, q, p)[0] for q in peers[p]])  # p receives from sender q
        pairs = [pair_setup(seed, p, q) for q in peers[p]]              # p sends to receiver q
        deltas = np.zeros(S, engine.LABEL)
        for k, (_, delta, _) in enumerate(pairs):
            deltas[k] = delta
        rcvs.append(engine.IKNPMultiReceiver(ctx, base))
        snds.append(engine.IKNPMultiSender(ctx, deltas, np.stack([k0 for _, _, k0 in pairs])))
    d_a = [ctx.to_device(x) for x in a]
    d_b = [ctx.to_device(x) for x in b]
    g_c = [GuardedWords(ctx, words) for _ in range(P)]
    d_umine = [Guarded(ctx, S * ub) for _ in range(P)]
    g_r = [GuardedWords(ctx, S * words) for _ in range(P)]
    for p in range(P):
        engine.gmw_triples_local_dev(ctx, d_a[p], d_b[p], g_c[p].ptr, words)
        rcvs[p].receive_bits_dev(d_b[p], 0, n, d_umine[p].ptr, g_r[p].ptr)
    for p in range(P):
        # what the peers sent p: session k of p's sender is peer q, whose receiver holds p as its session peers[q].index(p)
        d_utheirs, d_v = ctx.empty(S * ub), ctx.empty(S * words * 8)
        for k, q in enumerate(peers[p]):
            d_utheirs.copy_from(d_umine[q].ptr + peers[q].index(p) * ub, ub, k * ub)
            d_v.copy_from(d_b[q], words * 8, k * words * 8)  # v = b of the peer (triples.go:356-359)
        g_s, g_u = GuardedWords(ctx, S * words), GuardedWords(ctx, S * words)
        snds[p].send_bits_dev(d_utheirs, n, g_s.ptr)
        engine.gmw_triples_multi_sender_u_dev(snds[p], d_a[p], g_u.ptr, words)
        engine.gmw_triples_multi_sender_fold_dev(ctx, g_s.ptr, g_u.ptr, d_v, g_c[p].ptr, S, words)
        engine.gmw_triples_multi_receiver_fold_dev(ctx, g_r[p].ptr, g_c[p].ptr, S, words)
        ctx.sync()
        g_s.read(), g_u.read()
        d_utheirs.close(), d_v.close()
    c = [g.read().copy() for g in g_c]
    for g in d_umine + g_r:
        g.read()
    for h in rcvs + snds:
        h.close()
    return c


@pytest.mark.parametrize("P", [2, 3, 5])
@pytest.mark.parametrize("words", [1, 9, 128])
def test_triple_batch_end_to_end(ctx, P, words):
    """XOR over the parties of c is (XOR a) & (XOR b) on every word, and every party's c is what the per-pair one-session
    sequence gives on the same base labels, a and b"""
    from tests.test_gpu_gmw import _device_triples
    seed = 1000 * P + words
    a, b, c_pairs, _ = _device_triples(ctx, P, words, seed)
    c = multi_triples(ctx, P, words, seed, a, b)
    xa = np.bitwise_xor.reduce(np.stack(a), axis=0)
    xb = np.bitwise_xor.reduce(np.stack(b), axis=0)
    assert (np.bitwise_xor.reduce(np.stack(c), axis=0) == (xa & xb)).all(), "the shares do not multiply"
    for p in range(P):
        assert (c[p] == c_pairs[p]).all(), "party %d differs from the one-session sequence" % p


# ---- 7: the three fold calls -----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("S,words", [(1, 37), (4, 37), (1, FOLD_GRID * FOLD_THREADS + FOLD_THREADS + 5), (4, 1)])
def test_the_fold_calls_whole_buffers(ctx, S, words):
    """against numpy; words past one sweep of the folds' grid: the loop goes round for a full workgroup and a ragged one"""
    rng, base, deltas, k0 = sessions(20250109 + S, S)
    snd = engine.IKNPMultiSender(ctx, deltas, k0)
    dmask = np.where(deltas["d0"] & np.uint64(1), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0))
    a, c0 = rand_words(rng, words), rand_words(rng, words)
    x, y, z = rand_words(rng, (S, words)), rand_words(rng, (S, words)), rand_words(rng, (S, words))
    d_a, d_x, d_y, d_z = (ctx.to_device(v) for v in (a, x, y, z))
    g_u = GuardedWords(ctx, S * words)
    engine.gmw_triples_multi_sender_u_dev(snd, d_a, g_u.ptr, words)
    ctx.sync()
    assert np.array_equal(g_u.read().reshape(S, words), a[None, :] ^ dmask[:, None])
    g_c = GuardedWords(ctx, words, c0)
    engine.gmw_triples_multi_sender_fold_dev(ctx, d_x, d_y, d_z, g_c.ptr, S, words)
    ctx.sync()
    c1 = c0 ^ np.bitwise_xor.reduce(x ^ (y & z), axis=0)
    assert np.array_equal(g_c.read(), c1)
    engine.gmw_triples_multi_receiver_fold_dev(ctx, d_x, g_c.ptr, S, words)
    ctx.sync()
    assert np.array_equal(g_c.read(), c1 ^ np.bitwise_xor.reduce(x, axis=0))
    snd.close()
    for d in (d_a, d_x, d_y, d_z):
        d.close()


# ---- 8: misuse -------------------------------------------------------------------------------------------------------------


def test_misuse(ctx):
    L, E_ARG, OK = engine.lib(), engine.GC_E_ARG, engine.GC_OK
    S, per = 3, 549
    Wd = W(per)
    rng, base, deltas, k0 = sessions(20250110, S)
    rcv, snd = engine.IKNPMultiReceiver(ctx, base), engine.IKNPMultiSender(ctx, deltas, k0)
    out = ctx.empty(S * u_bytes(per) + 64).zero(SENTINEL)
    q = C.c_void_p(out.ptr)
    host = np.zeros(S * u_bytes(per) + 64, np.uint8)
    hp = host.ctypes.data_as(C.c_void_p)
    ul = S * u_bytes(per)
    # the wrong role
    assert L.gc_iknp_multi_receive_bits_dev(snd.h, q, 0, per, q, q) == E_ARG
    assert L.gc_iknp_multi_receive_bits(snd.h, hp, 0, per, hp, hp) == E_ARG
    assert L.gc_iknp_multi_send_bits_dev(rcv.h, q, per, q) == E_ARG
    assert L.gc_iknp_multi_send_bits(rcv.h, hp, ul, per, hp) == E_ARG
    assert L.gc_gmw_triples_multi_sender_u_dev(rcv.h, q, q, 4) == E_ARG
    # NULL arrays
    for args in ((None, 0, per, q, q), (q, 0, per, None, q), (q, 0, per, q, None)):
        assert L.gc_iknp_multi_receive_bits_dev(rcv.h, *args) == E_ARG
        assert L.gc_iknp_multi_receive_bits(rcv.h, *[hp if a is q else a for a in args]) == E_ARG
    assert L.gc_iknp_multi_send_bits_dev(snd.h, None, per, q) == E_ARG and L.gc_iknp_multi_send_bits_dev(snd.h, q, per, None) == E_ARG
    assert L.gc_iknp_multi_send_bits(snd.h, None, ul, per, hp) == E_ARG and L.gc_iknp_multi_send_bits(snd.h, hp, ul, per, None) == E_ARG
    # a stride in (0, W)
    for stride in (1, Wd - 1):
        assert L.gc_iknp_multi_receive_bits_dev(rcv.h, q, stride, per, q, q) == E_ARG
        assert L.gc_iknp_multi_receive_bits(rcv.h, hp, stride, per, hp, hp) == E_ARG
    # u_len is S * gc_iknp_u_bytes(per)
    for bad in (u_bytes(per), ul + 1, ul - 1, 0):
        assert L.gc_iknp_multi_send_bits(snd.h, hp, bad, per, hp) == E_ARG
    # sizes that do not fit size_t
    top = C.c_size_t(-1).value
    for big in (top // 2, top // S, top // 64):
        assert L.gc_iknp_multi_receive_bits_dev(rcv.h, q, 0, big, q, q) == E_ARG
        assert L.gc_iknp_multi_send_bits_dev(snd.h, q, big, q) == E_ARG
    assert L.gc_iknp_multi_receive_bits_dev(rcv.h, q, top // 8, per, q, q) == E_ARG
    assert L.gc_gmw_triples_multi_sender_fold_dev(ctx.h, q, q, q, q, S, top // 8) == E_ARG
    assert L.gc_gmw_triples_multi_receiver_fold_dev(ctx.h, q, q, 0, 4) == E_ARG
    # inside a capture: the position is a kernel argument
    for call in (lambda: rcv.receive_bits_dev(out, 0, per, out, out), lambda: snd.send_bits_dev(out, per, out)):
        with pytest.raises(engine.EngineError) as e:
            ctx.capture(call)
        assert e.value.code == E_ARG
    # per = 0: GC_OK, nothing written, the position stays — with or without arrays
    assert L.gc_iknp_multi_receive_bits_dev(rcv.h, None, 0, 0, None, None) == OK and L.gc_iknp_multi_receive_bits(rcv.h, None, 0, 0, None, None) == OK
    assert L.gc_iknp_multi_send_bits_dev(snd.h, None, 0, None) == OK and L.gc_iknp_multi_send_bits(snd.h, None, 0, 0, None) == OK
    ctx.sync()
    assert (out.numpy() == SENTINEL).all() and not host.any(), "a refused or empty call wrote something"
    assert rcv.info() == (S, True, 0) and snd.info() == (S, False, 0), "a refused or empty call moved the position"
    # and the handles still serve: the bytes of a fresh oracle pair
    ch = rand_words(rng, (S, Wd))
    u, r, s = oracle_bits(OracleSessions(base, deltas, k0), ch, per)
    have_u, have_r = rcv.receive_bits(ch, per)
    assert have_u == u and have_r.tobytes() == r.tobytes() and snd.send_bits(u, per).tobytes() == s.tobytes()
    rcv.close()
    snd.close()
