"""The per-session cursors of the device random streams (gc_rand_*_cur*; mpc_amd/csrc/rand_cursor_kernels.hip, rand_int.h)
byte for byte against the Python restatement of the Go reader (tests/py_rand_reference.py, held against SP 800-38A and OpenSSL
by the CPU suite) and of crypto/rand.Int (tests/go_transcript.py::crand_int, pinned by Go's own transcript hashes).  Every
device output is filled with a canary and lies between two sentinel words (Guarded), so a byte written behind a slot, into a
bad session's part, before the array or past its end fails the case.

Expected scalars are crand_int(reader, max) on a reader positioned at the session's cursor, the expected new cursor that
reader's position.  The reader here takes its bytes from rr.Streams (the array form of rr.Reader, which the CPU suite holds
against it) because the cases draw megabytes.

The sizes are the smallest at which the named thing can go wrong: ragged blocks, cursors in mid-block and apart by more than
2^32 blocks, a wave's chunk of 64 candidates and one more, candidates that straddle blocks at every offset, more blocks and
more streams than one sweep of the capped grid.  No case provokes a fault: a bad session is an ordinary data path."""
import ctypes as C

import numpy as np
import pytest

import oracle
from mpc_amd import engine
from tests import py_rand_reference as rr
from tests.go_transcript import crand_int
from tests.test_gpu_ot_sweeps import Guarded, SENTINEL

pytestmark = pytest.mark.gpu

GRID, THREADS, RUN = engine.rand_kernel_shape()
FF64 = (1 << 64) - 1
N = engine.P256_N
FAR = ((1 << 32) + 5) * 16 + 3
BEHIND_GARBLER = 32 + 16 * (1 + 128)

# max -> (k, mask)
MODULI = {N: (32, 0xff), (1 << 255) - 19: (32, 0x7f), (1 << 255) + 1: (32, 0xff), 1 << 128: (16, 0xff),
          (1 << 64) + 1: (9, 0x01), 257: (2, 0x01), 3: (1, 0x03), 2: (1, 0x01)}
REJECTING = ((1 << 255) + 1, (1 << 64) + 1, 257, 3)


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


def seeded(tag, S, keylen=32):
    rng = np.random.default_rng([S, keylen] + list(tag.encode()))
    return rng.integers(0, 256, (S, keylen), dtype=np.uint8), rng.integers(0, 256, (S, 16), dtype=np.uint8)


def cap(count):
    return 4 * count + 256


class StreamReader:
    """rr.Reader of one session, positioned at `pos`, its bytes fetched from rr.Streams a stretch at a time"""

    def __init__(self, seed, iv, pos=0, stretch=4096):
        self.st, self.pos, self.lo, self.buf, self.stretch = rr.Streams([seed], [iv]), pos, pos, b"", stretch

    def read(self, n):
        off = self.pos - self.lo
        if off + n > len(self.buf):
            self.lo, off = self.pos, 0
            self.buf = self.st.at(self.pos, max(n, self.stretch))[0].tobytes()
        self.pos += n
        return self.buf[off: off + n]


class Cursors:
    """d_cur and d_status of a handle's calls"""

    def __init__(self, ctx, cur):
        self.ctx = ctx
        self.d_cur = ctx.to_device(np.array(cur, np.uint64))
        self.status = Guarded(ctx, 16)

    def read(self):
        self.ctx.sync()
        return [int(v) for v in self.d_cur.numpy()]

    def read_status(self):
        self.ctx.sync()
        return [int(v) for v in self.status.read().view(np.uint64)]


def slot_stride(n):
    return (n + 15) // 16 * 16 + 32


def fill_cur(ctx, h, cs, n, stride=None):
    """one gc_rand_fill_cur_dev into canary-filled slots -> u8 [S, stride]"""
    stride = slot_stride(n) if stride is None else stride
    g = Guarded(ctx, (h.S * stride + 15) // 16 * 16)
    h.fill_cur(cs.d_cur, n, g.ptr, cs.status.ptr, stride)
    ctx.sync()
    raw = g.read()
    assert (raw[h.S * stride:] == SENTINEL).all()
    return raw[:h.S * stride].reshape(h.S, stride)


def check_slots(got, want, n):
    assert (got[:, :n] == want).all(), "session %d differs" % int(np.argmax((got[:, :n] != want).any(axis=1)))
    assert (got[:, n:] == SENTINEL).all(), "bytes behind nbytes were written"


def each_stream(seeds, ivs, cur, n):
    return np.stack([np.frombuffer(rr.Streams([seeds[s]], [ivs[s]]).at(cur[s], n)[0].tobytes(), np.uint8)
                     for s in range(len(seeds))])


# ---- 1. equal cursors are the handle ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("pos", [0, 5])
def test_equal_cursors_are_the_handle(ctx, pos):
    S = 3
    seeds, ivs = seeded("equal", S)
    h, ref = engine.RandStreams(ctx, seeds, ivs), rr.Streams(seeds, ivs)
    for n in (1, 15, 16, 17, 4112):
        cs = Cursors(ctx, [123] * S)
        h.cur_set(cs.d_cur, pos)
        check_slots(fill_cur(ctx, h, cs, n), ref.at(pos, n), n)
        assert cs.read() == [pos + n] * S and cs.read_status() == [0, FF64]
        assert h.info() == (S, 32, 0)  # the handle's own position is not the cursors'
    h.close()


# ---- 2. divergent cursors ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,stride", [(37, 41), (4112, 4144)], ids=["bytewise", "aligned"])
def test_divergent_cursors(ctx, n, stride):
    S = 5
    cur = [0, 5, 16, 33, FAR]
    seeds, ivs = seeded("divergent", S)
    h = engine.RandStreams(ctx, seeds, ivs)
    cs = Cursors(ctx, cur)
    for _ in range(2):  # the second fill continues each stream from its own place
        got = fill_cur(ctx, h, cs, n, stride)
        if n < 100:  # block by block on the AES class as well
            for s in range(S):
                assert got[s, :n].tobytes() == rr.keystream(seeds[s], ivs[s], cur[s], n), s
        check_slots(got, each_stream(seeds, ivs, cur, n), n)
        cur = [c + n for c in cur]
        assert cs.read() == cur and cs.read_status() == [0, FF64]
    h.close()


# ---- 3. past one sweep of the grid --------------------------------------------------------------------------------------------


def test_one_stream_longer_than_a_sweep(ctx):
    n = (GRID * THREADS + 2 * THREADS + RUN + 3) * 16 + 5
    seeds, ivs = seeded("sweep", 1)
    h = engine.RandStreams(ctx, seeds, ivs)
    cs = Cursors(ctx, [7])
    check_slots(fill_cur(ctx, h, cs, n), rr.Streams(seeds, ivs).at(7, n), n)
    assert cs.read() == [7 + n] and cs.read_status() == [0, FF64]
    h.close()


def test_more_streams_than_a_sweep_of_waves(ctx):
    S = 70000
    assert S > GRID * THREADS // 64
    seeds, ivs = seeded("many", S)
    h = engine.RandStreams(ctx, seeds, ivs)
    cur = [s % 3 for s in range(S)]
    cs = Cursors(ctx, cur)
    got = fill_cur(ctx, h, cs, 16, stride=16)
    wide = rr.Streams(seeds, ivs).at(0, 18)  # bytes [0, 18) of every stream hold its 16 from 0, 1 or 2
    want = np.stack([wide[s, cur[s]: cur[s] + 16] for s in range(S)])
    check_slots(got, want, 16)
    assert cs.read() == [c + 16 for c in cur] and cs.read_status() == [0, FF64]
    h.close()


# ---- 4. counter carries under a cursor ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("iv", [(1 << 128) - 1, (0x0123456789abcdef << 64) | (FF64 - 1)], ids=["wrap", "into-high-half"])
def test_counter_carries_under_a_cursor(ctx, iv):
    seeds, _ = seeded("carry", 2)
    ivs = np.array([list(iv.to_bytes(16, "big"))] * 2, np.uint8)
    h = engine.RandStreams(ctx, seeds, ivs)
    cur = [0, 16]
    cs = Cursors(ctx, cur)
    got = fill_cur(ctx, h, cs, 64)
    for s in range(2):
        assert got[s, :64].tobytes() == rr.keystream(seeds[s], ivs[s], cur[s], 64), s
    check_slots(got, each_stream(seeds, ivs, cur, 64), 64)
    assert cs.read() == [64, 80]
    h.close()


# ---- 5. a bad session in a fill ---------------------------------------------------------------------------------------------


def test_bad_session_in_a_fill(ctx):
    S, n = 3, 16
    seeds, ivs = seeded("badfill", S)
    h = engine.RandStreams(ctx, seeds, ivs)
    cur = [3, (1 << 64) - 8, 32]
    cs = Cursors(ctx, cur)
    got = fill_cur(ctx, h, cs, n)
    assert cs.read_status() == [1, 1]
    assert (got[1] == SENTINEL).all(), "the bad session's slot was written"
    for s in (0, 2):
        assert got[s, :n].tobytes() == rr.keystream(seeds[s], ivs[s], cur[s], n) and (got[s, n:] == SENTINEL).all()
    assert cs.read() == [3 + n, cur[1], 32 + n]
    # the last position that fits is served: 2^64 - 1 - n
    cs = Cursors(ctx, [FF64 - n] * S)
    got = fill_cur(ctx, h, cs, n)
    assert cs.read_status() == [0, FF64] and cs.read() == [FF64] * S
    check_slots(got, each_stream(seeds, ivs, [FF64 - n] * S, n), n)
    # the host form: GC_E_ARG, the lowest bad session, the same outputs
    out = np.full((S, 48), SENTINEL, np.uint8)
    with pytest.raises(engine.RandSessionError) as e:
        h.fill_cur_host(cur, n, out, 48)
    assert e.value.code == engine.GC_E_ARG and e.value.bad_session == 1
    assert (out == got_host_want(seeds, ivs, cur, n, 48)).all()
    assert [int(v) for v in e.value.cur] == [3 + n, cur[1], 32 + n]
    # ... and without a bad session
    out, new = h.fill_cur_host([0, 5, FAR], 37)
    assert (out == each_stream(seeds, ivs, [0, 5, FAR], 37)).all() and [int(v) for v in new] == [37, 42, FAR + 37]
    assert h.pos == 0
    h.close()


def got_host_want(seeds, ivs, cur, n, stride):
    want = np.full((len(seeds), stride), SENTINEL, np.uint8)
    for s in range(len(seeds)):
        if cur[s] <= FF64 - n:
            want[s, :n] = np.frombuffer(rr.keystream(seeds[s], ivs[s], cur[s], n), np.uint8)
    return want


# ---- 6. scalars -------------------------------------------------------------------------------------------------------------

COUNTS = (1, 5, 64, 65, 200)
STARTS = (0, 7, BEHIND_GARBLER)


def reference_scalars(seeds, ivs, cur, mx, count):
    """-> (scalars u8 [S, count, 32], new cursors, candidates looked at per draw [S][count])"""
    S = len(seeds)
    out, new, looked = np.zeros((S, count, 32), np.uint8), [], []
    k = MODULI[mx][0] if mx in MODULI else ((mx - 1).bit_length() + 7) // 8
    for s in range(S):
        r = StreamReader(seeds[s], ivs[s], cur[s], stretch=max(4096, 2 * k * count))
        per = []
        for i in range(count):
            before = r.pos
            out[s, i] = np.frombuffer(crand_int(r, mx).to_bytes(32, "big"), np.uint8)
            per.append((r.pos - before) // k)
        new.append(r.pos)
        looked.append(per)
    return out, new, looked


def first_rejected(per):
    """the index of a session's first rejected candidate, from the candidates each of its draws looked at"""
    for i, n in enumerate(per):
        if n > 1:
            return sum(per[:i])
    return sum(per)


def scalars_dev(ctx, h, cs, mx, count):
    g = Guarded(ctx, h.S * count * 32)
    h.scalars_cur(cs.d_cur, mx, count, g.ptr, cs.status.ptr)
    ctx.sync()
    return g.read().reshape(h.S, count, 32)


def scalar_cases(S, keylen):
    """every modulus with every count, the start cursors going round the sessions -> (seeds, ivs, [(max, count, cursors,
    scalars, new cursors, candidates per draw)]); asserts on the reference alone, before any device is looked at, that the
    cases do what they are there for"""
    seeds, ivs = seeded("scalars", S, keylen)
    cases = []
    for ci, (mx, count) in enumerate((m, c) for m in MODULI for c in COUNTS):
        cur = [STARTS[(ci + s) % 3] for s in range(S)]
        cases.append((mx, count, cur) + reference_scalars(seeds, ivs, cur, mx, count))
    for mx in REJECTING:
        assert any(new[s] > cur[s] + count * MODULI[mx][0] for m, count, cur, _, new, _ in cases if m == mx for s in range(S)), \
            "no rejection with max = %#x" % mx
    assert any(first_rejected(per) < 64 for _, count, _, _, _, looked in cases if count == 65 for per in looked), \
        "at count = 65 no session rejects inside its first chunk of 64 candidates"
    assert all(sum(per) <= cap(count) for _, count, _, _, _, looked in cases for per in looked)
    return seeds, ivs, cases


@pytest.mark.parametrize("S,keylen", [(1, 32), (3, 32), (65, 32), (3, 16), (3, 24)])
def test_scalars(ctx, S, keylen):
    seeds, ivs, cases = scalar_cases(S, keylen)
    h = engine.RandStreams(ctx, seeds, ivs)
    for mx, count, cur, want, new, _ in cases:
        cs = Cursors(ctx, cur)
        got = scalars_dev(ctx, h, cs, mx, count)
        bad = (got != want).any(axis=2)
        assert not bad.any(), "max = %#x count = %d: session %d draw %d" % ((mx, count) + tuple(int(v[0]) for v in np.nonzero(bad)))
        assert cs.read() == new, (hex(mx), count)
        assert cs.read_status() == [0, FF64]
    # the host form is the device form
    for mx, count, cur, want, new, _ in cases[1::7]:
        out, got_cur = h.scalars_cur_host(cur, mx, count)
        assert (out == want).all() and [int(v) for v in got_cur] == new
    assert h.pos == 0
    h.close()


def test_scalars_into_unaligned_and_successive_outputs(ctx):
    """an output array off 16-byte boundaries goes out bytewise, and two draws in a row are one draw of the sum"""
    S = 3
    seeds, ivs = seeded("unaligned", S)
    h = engine.RandStreams(ctx, seeds, ivs)
    cur = [0, 7, 100]
    want, new, _ = reference_scalars(seeds, ivs, cur, (1 << 255) + 1, 70)
    cs = Cursors(ctx, cur)
    g = Guarded(ctx, S * 70 * 32 + 16)
    h.scalars_cur(cs.d_cur, (1 << 255) + 1, 70, g.ptr + 4, cs.status.ptr)
    ctx.sync()
    raw = g.read()
    assert (raw[:4] == SENTINEL).all() and (raw[4 + S * 70 * 32:] == SENTINEL).all()
    assert (raw[4: 4 + S * 70 * 32].reshape(S, 70, 32) == want).all() and cs.read() == new
    cs = Cursors(ctx, cur)
    first, second = scalars_dev(ctx, h, cs, (1 << 255) + 1, 30), scalars_dev(ctx, h, cs, (1 << 255) + 1, 40)
    assert (np.concatenate([first, second], axis=1) == want).all() and cs.read() == new
    h.close()


# ---- 7. a bad session in a scalar draw --------------------------------------------------------------------------------------


def test_bad_session_in_a_scalar_draw(ctx):
    S, count = 3, 5
    seeds, ivs = seeded("badscalar", S)
    h = engine.RandStreams(ctx, seeds, ivs)
    cur = [0, 7, (1 << 64) - 100]
    want, new, _ = reference_scalars(seeds[:2], ivs[:2], cur[:2], N, count)
    cs = Cursors(ctx, cur)
    got = scalars_dev(ctx, h, cs, N, count)
    assert cs.read_status() == [1, 2]
    assert (got[2] == SENTINEL).all(), "the bad session's scalars were written"
    assert (got[:2] == want).all() and cs.read() == new + [cur[2]]
    # the range test is the header's: the last cursor that leaves room for every candidate of the bound is served
    edge = FF64 - 32 * cap(count)
    cs = Cursors(ctx, [edge, edge + 1, 0])
    got = scalars_dev(ctx, h, cs, N, count)
    assert cs.read_status() == [1, 1] and (got[1] == SENTINEL).all()
    w0, n0, _ = reference_scalars(seeds[:1], ivs[:1], [edge], N, count)
    assert (got[0] == w0[0]).all() and cs.read()[:2] == [n0[0], edge + 1]
    out = np.full((S, count, 32), SENTINEL, np.uint8)
    with pytest.raises(engine.RandSessionError) as e:
        h.scalars_cur_host(cur, N, count, out)
    assert e.value.bad_session == 2 and (out[:2] == want).all() and (out[2] == SENTINEL).all()
    assert [int(v) for v in e.value.cur] == new + [cur[2]]
    h.close()


# ---- 8. into Chou-Orlandi -----------------------------------------------------------------------------------------------------


def test_the_draws_feed_chou_orlandi(ctx):
    S, per = 3, 5
    seeds, ivs = seeded("co", S)
    h = engine.RandStreams(ctx, seeds, ivs)
    readers = [StreamReader(seeds[s], ivs[s]) for s in range(S)]
    a = [crand_int(r, N) for r in readers]
    scalars = [crand_int(r, N) for r in readers for _ in range(per)]
    choice = np.random.default_rng(8).integers(0, 2, S * per, dtype=np.uint8)
    A, AaInv = engine.co_multi_sender_setup(ctx, a)  # (the first CO call of the ctx: uploads G's table)
    points = engine.co_multi_receiver_choices(ctx, A, scalars, choice, S, per)
    cs = Cursors(ctx, [0] * S)
    d_a, d_sc = Guarded(ctx, S * 32), Guarded(ctx, S * per * 32)
    d_A, d_AaInv, d_pts = Guarded(ctx, S * 64), Guarded(ctx, S * 64), Guarded(ctx, S * per * 64)
    d_co = ctx.zeros(4, np.uint64)
    h.draw_co_sender(cs.d_cur, d_a.ptr, cs.status.ptr)
    engine.co_multi_sender_setup_dev(ctx, d_a.ptr, S, d_A.ptr, d_AaInv.ptr, d_co)
    h.draw_co_receiver(per, cs.d_cur, d_sc.ptr, cs.status.ptr)
    d_choice = ctx.to_device(choice)
    engine.co_multi_receiver_choices_dev(ctx, d_A.ptr, d_sc.ptr, d_choice, S, per, d_pts.ptr, d_co)
    ctx.sync()
    assert (d_a.read().reshape(S, 32) == engine._scalars(a)).all()
    assert (d_A.read().reshape(S, 64) == A).all() and (d_AaInv.read().reshape(S, 64) == AaInv).all()
    assert (d_pts.read().reshape(S * per, 64) == points).all()
    assert cs.read() == [r.pos for r in readers] and cs.read_status() == [0, FF64]
    h.close()


# ---- 9. capture -------------------------------------------------------------------------------------------------------------


def test_a_captured_step_draws_fresh_keys_on_every_replay(ctx, add64_circ):
    c, batch = add64_circ, 3
    seeds, ivs = seeded("capture", batch)
    h = engine.RandStreams(ctx, seeds, ivs)
    dc = engine.DeviceCircuit(ctx, c)
    gb = engine.Batch(dc, batch)
    assert gb.keyed_supported()
    gb.set_graph(True)
    nrnd = 16 * (1 + c.num_inputs)
    d_keys, d_rnd, d_a = ctx.empty((batch, 32)), ctx.empty((batch, nrnd)), Guarded(ctx, batch * 32)
    cs = Cursors(ctx, [99] * batch)
    h.cur_set(cs.d_cur, 0)

    def step():
        h.fill_cur(cs.d_cur, 32, d_keys, cs.status.ptr)
        h.fill_cur(cs.d_cur, nrnd, d_rnd, cs.status.ptr)
        h.draw_co_sender(cs.d_cur, d_a.ptr, cs.status.ptr)
        gb.garble_keyed(d_keys, 32, d_rnd)

    def check(readers):
        ctx.sync()
        R, slab, a = gb.read_r(), gb.read_slab(), d_a.read().reshape(batch, 32)
        for i, r in enumerate(readers):
            key, rnd = r.read(32), r.read(nrnd)
            ref = oracle.garble(c.Gates, c.NumWires, c.num_inputs, key, rnd)
            assert R[i] == ref["R"], "R of instance %d" % i
            assert (slab[i] == ref["slab"]).all(), "tables of instance %d" % i
            assert a[i].tobytes() == crand_int(r, N).to_bytes(32, "big"), "a of instance %d" % i
        assert cs.read() == [r.pos for r in readers] and cs.read_status() == [0, FF64]

    step()  # uncaptured once
    check([StreamReader(seeds[i], ivs[i]) for i in range(batch)])
    h.cur_set(cs.d_cur, 0)
    g = ctx.capture(step)
    assert cs.read() == [0] * batch  # recording runs nothing
    readers = [StreamReader(seeds[i], ivs[i]) for i in range(batch)]
    for _ in range(3):
        g.launch()
        check(readers)  # round r of every reader: the streams go on where the array stands
    g.close()
    # a cur_set at the head of the graph: every replay is the first round again
    g = ctx.capture(lambda: (h.cur_set(cs.d_cur, 0), step()))
    for _ in range(2):
        g.launch()
        check([StreamReader(seeds[i], ivs[i]) for i in range(batch)])
    g.close()
    assert h.pos == 0
    gb.close()
    dc.close()
    h.close()


# ---- 10. errors with a device -------------------------------------------------------------------------------------------------


def test_error_contract(ctx):
    L = engine.lib()
    S = 3
    seeds, ivs = seeded("errors", S)
    h = engine.RandStreams(ctx, seeds, ivs)
    cur = [1, 2, 3]
    cs = Cursors(ctx, cur)
    d = Guarded(ctx, S * 64)
    host = np.full((S, 64), SENTINEL, np.uint8)
    hcur = np.array(cur, np.uint64)
    dp = lambda v: C.c_void_p(v)
    mx = lambda v: np.frombuffer(int(v).to_bytes(32, "big"), np.uint8).ctypes.data_as(C.c_void_p)
    n32, none = mx(N), None
    refused = [
        lambda: L.gc_rand_fill_cur_dev(h.h, dp(cs.d_cur.ptr), 33, dp(d.ptr), 32, dp(cs.status.ptr)),         # stride < nbytes
        lambda: L.gc_rand_fill_cur(h.h, hcur.ctypes.data_as(C.c_void_p), 33, host.ctypes.data_as(C.c_void_p), 32, none),
        lambda: L.gc_rand_fill_cur_dev(h.h, dp(cs.d_cur.ptr), 16, dp(d.ptr), 64, none),                      # NULL d_status
        lambda: L.gc_rand_scalars_cur_dev(h.h, dp(cs.d_cur.ptr), n32, 1, dp(d.ptr), none),
        lambda: L.gc_rand_fill_cur_dev(h.h, none, 16, dp(d.ptr), 64, dp(cs.status.ptr)),                     # NULL arrays
        lambda: L.gc_rand_fill_cur_dev(h.h, dp(cs.d_cur.ptr), 16, none, 64, dp(cs.status.ptr)),
        lambda: L.gc_rand_scalars_cur_dev(h.h, dp(cs.d_cur.ptr), none, 1, dp(d.ptr), dp(cs.status.ptr)),
        lambda: L.gc_rand_scalars_cur_dev(h.h, dp(cs.d_cur.ptr), n32, 1, none, dp(cs.status.ptr)),
        lambda: L.gc_rand_cur_set_dev(h.h, none, 0),
        lambda: L.gc_rand_fill_cur_dev(h.h, dp(cs.d_cur.ptr + 4), 16, dp(d.ptr), 64, dp(cs.status.ptr)),    # misaligned d_cur
        lambda: L.gc_rand_scalars_cur_dev(h.h, dp(cs.d_cur.ptr + 4), n32, 1, dp(d.ptr), dp(cs.status.ptr)),
        lambda: L.gc_rand_cur_set_dev(h.h, dp(cs.d_cur.ptr + 4), 0),
        lambda: L.gc_rand_fill_cur_dev(h.h, dp(cs.d_cur.ptr), 16, dp(d.ptr), 1 << 63, dp(cs.status.ptr)),    # past size_t
        lambda: L.gc_rand_scalars_cur_dev(h.h, dp(cs.d_cur.ptr), n32, 1 << 59, dp(d.ptr), dp(cs.status.ptr)),
        lambda: L.gc_rand_scalars_cur_dev(h.h, dp(cs.d_cur.ptr), mx(0), 1, dp(d.ptr), dp(cs.status.ptr)),    # a bad max
        lambda: L.gc_rand_scalars_cur_dev(h.h, dp(cs.d_cur.ptr), mx(1), 1, dp(d.ptr), dp(cs.status.ptr)),
        lambda: L.gc_rand_scalars_cur(h.h, hcur.ctypes.data_as(C.c_void_p), mx(1), 1, host.ctypes.data_as(C.c_void_p), none),
    ]
    for i, call in enumerate(refused):
        assert call() == engine.GC_E_ARG, i
    # nothing to do is no error and touches nothing, the status included
    h.fill_cur(cs.d_cur, 0, d.ptr, cs.status.ptr, 0)
    h.scalars_cur(cs.d_cur, N, 0, d.ptr, cs.status.ptr)
    assert L.gc_rand_fill_cur_dev(h.h, none, 0, none, 0, none) == engine.GC_OK
    assert L.gc_rand_scalars_cur_dev(h.h, none, none, 0, none, none) == engine.GC_OK
    assert L.gc_rand_fill_cur(h.h, none, 0, none, 0, none) == engine.GC_OK
    assert L.gc_rand_scalars_cur(h.h, none, n32, 0, none, none) == engine.GC_OK
    ctx.sync()
    assert cs.read() == cur and hcur.tolist() == cur and (host == SENTINEL).all() and (d.read() == SENTINEL).all()
    assert (cs.status.read() == SENTINEL).all(), "a refused or empty call wrote the status block"
    # the host forms wait and allocate: not inside a capture
    for call in (lambda: h.fill_cur_host(cur, 16), lambda: h.scalars_cur_host(cur, N, 1)):
        with pytest.raises(engine.EngineError) as e:
            ctx.capture(call)
        assert e.value.code == engine.GC_E_ARG
    # after cursor draws on this handle the calls on its own position are what they were: refused inside a capture ...
    h.fill_cur(cs.d_cur, 16, d.ptr, cs.status.ptr, 64)
    h.seek(16)
    with pytest.raises(engine.EngineError) as e:
        ctx.capture(lambda: h.fill(16, d.ptr, 64))
    assert e.value.code == engine.GC_E_ARG and h.pos == 16
    # ... and filling from h.pos, whatever the cursors say
    g = Guarded(ctx, S * 64)
    h.fill(48, g.ptr, 64)
    ctx.sync()
    check_slots(g.read().reshape(S, 64), rr.Streams(seeds, ivs).at(16, 48), 48)
    assert h.pos == 64 and cs.read() == [c + 16 for c in cur]
    h.close()
