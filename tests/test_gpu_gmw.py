"""GMW party engine on the GPU (gc_gmw_*, mpc_amd/csrc/gmw_engine.cpp + gmw_kernels.hip) against the plain-Python
restatement of the reference (tests/py_gmw_reference.py): every step's message (padding bits included), the output shares,
the plaintext result, the launch count, for every instance of the batch; the circuits of tests/gmw_cases.py (the ones the
host walk of tests/test_gmw_plan_walk.py runs on the CPU); several passes on one handle, abandoned ones and misuse between
them; 2^20 instances of aes_128; the Beaver-triple folds on real bit-COT outputs and past one sweep of their grid; an
end-to-end AES pass on device-made triples; misuse."""
import numpy as np
import pytest

import oracle
from mpc_amd import engine
from tests import gmw_cases as G
from tests import py_gmw_reference as R
from tests.test_gpu_ot import base_setup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


def _fuzz3():
    rng = np.random.default_rng(3030)
    return R.fuzz_circuit(rng, 96, 900, 0.15, nargs=3, p_and=0.3)


def _circuit(name, aes_circ, add64_circ):
    return {"aes": aes_circ, "add64": add64_circ, "fuzz3": None}[name] or _fuzz3()


def _sample(batch, rng):
    if batch <= 64:
        return np.arange(batch)
    return np.unique(np.concatenate([np.arange(16), [batch - 1], rng.choice(batch, 47, replace=False)]))


def _round_words(c):
    _, _, _, wl = engine.gmw_plan_describe(c.Gates, c.NumWires, c.num_inputs, c.num_outputs)
    return [int(w) for w in wl if w]


def _host_steps(parties, msgs, cur, limit=None):
    """host-form steps of every party, round by round, until the pass ends (True) or `limit` rounds were made (False);
    msgs[p] grows by (level, [2][w][batch]) per round, cur holds the last round's messages"""
    P = len(parties)
    done = 0
    while limit is None or done < limit:
        new = []
        for p, g in enumerate(parties):
            peers = None if cur[0] is None else np.stack([cur[q] for q in range(P) if q != p])
            new.append(g.step(peers))
        if new[0][1].shape[1] == 0:
            assert all(m.shape[1] == 0 for _, m in new)
            return True
        for p in range(P):
            msgs[p].append(new[p])
        cur[:] = [m for _, m in new]
        done += 1
    return False


def _run_host(parties, inputs, triples, limit=None):
    """one pass of every party through the host forms; returns (msgs[p] = [(level, [2][w][batch])], outs[p]).  With `limit`
    the pass is left after that many rounds: (msgs, None)."""
    P = len(parties)
    for g, x, t in zip(parties, inputs, triples):
        g.set_inputs(x)
        g.set_triples(*t)
    msgs = [[] for _ in range(P)]
    cur = [None] * P
    if limit is not None:
        assert not _host_steps(parties, msgs, cur, limit)
        return msgs, None
    assert _host_steps(parties, msgs, cur)
    return msgs, [g.get_outputs() for g in parties]


def _run_dev(ctx, c, parties, inputs, triples, limit=None):
    """the same through the _dev forms, messages passed device-side through a double-buffered exchange area: party p writes
    slot p, slots 0 .. P-2 are copied behind slot P-1, so party p's peers are the P-1 slots after its own"""
    P, batch = len(parties), parties[0].batch
    ws = _round_words(c)
    maxw = max(ws + [1])
    d_in = [ctx.to_device(np.ascontiguousarray(x, np.uint64)) for x in inputs]
    d_t = [[ctx.to_device(np.ascontiguousarray(a, np.uint64)) for a in t] for t in triples]
    xch = [ctx.zeros((2 * P - 1) * 2 * maxw * batch * 8) for _ in range(2)]
    outw = (c.num_outputs + 63) // 64
    d_out = [ctx.zeros(max(outw * batch * 8, 16)) for _ in range(P)]
    for g, x, t in zip(parties, d_in, d_t):
        g.set_inputs_dev(x)
        g.set_triples_dev(*t)
    msgs = [[] for _ in range(P)]
    r = 0
    while limit is None or r < limit:
        w_prev = ws[r - 1] if r else 0
        w = ws[r] if r < len(ws) else 0
        src, dst = xch[(r + 1) & 1], xch[r & 1]
        res = []
        for p, g in enumerate(parties):
            peers = (src + (p + 1) * 2 * w_prev * batch * 8) if w_prev else None
            res.append(g.step_dev(peers, (dst + p * 2 * w * batch * 8) if w else None))
        assert all(x == res[0] for x in res)
        level, words = res[0]
        assert words == w
        if not words:
            break
        slot = 2 * w * batch * 8
        for k in range(P - 1):
            dst.copy_from(dst + k * slot, slot, offset=(P + k) * slot)
        host = dst.download(np.uint64, None, 0, P * slot).reshape(P, 2, w, batch)
        for p in range(P):
            msgs[p].append((level, host[p]))
        r += 1
    outs = [] if limit is None else None
    for p, g in enumerate(parties):
        if limit is not None:  # the pass is left here; the handle's triple pointers die with the buffers below
            assert r == limit
            break
        g.get_outputs_dev(d_out[p])
        outs.append(d_out[p].download(np.uint64, None, 0, outw * batch * 8).reshape(outw, batch))
    for b in d_in + [x for t in d_t for x in t] + xch + d_out:
        b.close()
    return msgs, outs


def _check_pass(c, P, batch, seed, msgs, outs, bits, shares, trip, launches):
    """every instance of the batch: the messages of every level (whole words, padding bits included) and the output shares
    against R.run_parties (vectorised over the batch), the XOR of the output shares against the plaintext in the bucketed
    order, (level, words) of every round, and the launch count"""
    ref_msgs, ref_outs = R.run_parties(c, shares, trip)
    w_of = R.triple_words(c)[0]
    for p in range(P):
        assert [lv for lv, _ in msgs[p]] == [lv for lv, _ in ref_msgs[p]]
        for (lv, m), (_, rm) in zip(msgs[p], ref_msgs[p]):
            assert m.shape == rm.shape == (2, w_of[lv], batch)
            assert (m == rm).all(), "party %d level %d: message differs from the reference's" % (p, lv)
        assert outs[p].shape == ref_outs[p].shape and (outs[p] == ref_outs[p]).all()
    x = np.bitwise_xor.reduce(np.stack(outs), axis=0)
    ob = R.unpack(x, c.num_outputs)
    assert (ob == G.plain_bucketed_batch(c, bits)).all()
    rng = np.random.default_rng(seed + 1)
    for i in _sample(batch, rng)[:24]:  # the batched plaintext above against the restatement's own, instance by instance
        assert (ob[:, i] == R.plain_bucketed(c, bits[i])).all()
    ands, _ = R.buckets(c)
    n_and_levels = sum(1 for a in ands if a)
    assert launches <= n_and_levels + 2
    return n_and_levels


@pytest.mark.parametrize("batch", [1, 63, 64, 65, 1000, 4096])
@pytest.mark.parametrize("name,P", [("aes", 2), ("add64", 2), ("fuzz3", 3)])
def test_online_phase_bit_for_bit(ctx, aes_circ, add64_circ, name, P, batch):
    c = _circuit(name, aes_circ, add64_circ)
    seed = batch * 7 + P
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, (batch, c.num_inputs)).astype(np.uint8)
    shares = R.share_inputs(rng, c, bits, P)
    _, _, tw = R.triple_words(c)
    trip = R.beaver_triples(rng, P, tw, batch)
    parties = [engine.Gmw(ctx, c, P, p, batch) for p in range(P)]
    assert parties[0].info.triple_words == tw
    if batch in (65, 1000, 4096):  # the device-resident forms
        msgs, outs = _run_dev(ctx, c, parties, shares, trip)
    else:
        msgs, outs = _run_host(parties, shares, trip)
    _check_pass(c, P, batch, seed, msgs, outs, bits, shares, trip, parties[0].last_launches)
    assert all(g.last_launches == parties[0].last_launches for g in parties)
    for g in parties:
        g.close()


def _make(ctx, c, P, batch):
    parties = [engine.Gmw(ctx, c, P, p, batch) for p in range(P)]
    assert parties[0].info.triple_words == R.triple_words(c)[2]
    return parties


def _one_pass(ctx, c, parties, batch, seed, dev):
    """a full pass on the given handles with the inputs and triples of `seed`, every instance checked; returns the number of
    AND levels"""
    P = len(parties)
    bits, shares, trip = G.pass_data(c, P, batch, seed)
    msgs, outs = _run_dev(ctx, c, parties, shares, trip) if dev else _run_host(parties, shares, trip)
    n_and_levels = _check_pass(c, P, batch, seed, msgs, outs, bits, shares, trip, parties[0].last_launches)
    assert all(g.last_launches == parties[0].last_launches for g in parties)
    return n_and_levels


DIRECTED = G.directed()


@pytest.mark.parametrize("batch", [1, 65, 130])
@pytest.mark.parametrize("k", range(len(DIRECTED)), ids=[c.name for c, _ in DIRECTED])
def test_directed_circuits_through_the_engine(ctx, k, batch):
    """the directed circuits of tests/gmw_cases.py (what each pins is written there), 2 .. 5 parties in turn; every circuit
    runs in the host form at one batch and in the _dev form at another"""
    c, status = DIRECTED[k]
    P = G.directed_parties(k)
    if status:
        with pytest.raises(engine.EngineError) as e:
            engine.Gmw(ctx, c, P, 0, batch)
        assert e.value.code == status == engine.GC_E_WIRE
        return
    parties = _make(ctx, c, P, batch)
    _one_pass(ctx, c, parties, batch, 1000 * batch + k, dev=(k + batch) % 2 == 1)
    for g in parties:
        g.close()


@pytest.mark.parametrize("seed,batch,dev", G.GPU_FUZZ)
def test_fuzz_circuits_through_the_engine(ctx, seed, batch, dev):
    """seeded circuits of the host walk's set: 2 .. 5 parties (P = 5 in both forms: four peers behind `peers`), reuse up to
    0.6, p_and 0 .. 0.9"""
    c, P = G.fuzz_case(seed)
    assert P == 2 + seed % 4
    parties = _make(ctx, c, P, batch)
    _one_pass(ctx, c, parties, batch, 50000 + seed, dev)
    for g in parties:
        g.close()


def test_fuzz_set_covers_parties_batches_and_forms():
    cases = [(2 + seed % 4, batch, dev) for seed, batch, dev in G.GPU_FUZZ]
    assert len(cases) >= 24
    assert {P for P, _, _ in cases} == {2, 3, 4, 5} and {b for _, b, _ in cases} == {1, 63, 64, 65, 257, 1000}
    assert {dev for P, _, dev in cases if P == 5} == {False, True}
    assert 8 <= sum(1 for _, _, dev in cases if dev) <= len(cases) - 8


def _arg_error(fn, *args):
    with pytest.raises(engine.EngineError) as e:
        fn(*args)
    assert e.value.code == engine.GC_E_ARG


@pytest.mark.parametrize("name,P,batch", [("aes", 2, 130), ("fuzz3", 3, 257)])
def test_handles_are_reused_over_passes(ctx, aes_circ, add64_circ, name, P, batch):
    """One set of handles, pass after pass with new inputs and triples, each checked for every instance and with the launch
    count of that pass: host form, _dev form, host form; a host pass left after two rounds, then a full _dev pass; a _dev pass
    left after two rounds, then a host pass with misuse in it (outputs and a step between the restart and the triples,
    triples after the first step, outputs in mid-pass: GC_E_ARG each, and the pass goes on); a last _dev pass."""
    c = _circuit(name, aes_circ, add64_circ)
    parties = _make(ctx, c, P, batch)
    g0 = parties[0]
    seed = 31000 + batch
    for k, dev in enumerate((False, True, False)):
        n = _one_pass(ctx, c, parties, batch, seed + k, dev)
        assert g0.last_launches == n + 2  # the input load and R + 1 steps: the count starts again with every pass
    assert n >= 3
    # a host pass left after two rounds; the next set_inputs starts over
    _, shares, trip = G.pass_data(c, P, batch, seed + 10)
    msgs, outs = _run_host(parties, shares, trip, limit=2)
    assert outs is None and len(msgs[0]) == 2
    assert _one_pass(ctx, c, parties, batch, seed + 11, True) == n and g0.last_launches == n + 2
    # a _dev pass left after two rounds, then a host pass with misuse in it
    _, shares, trip = G.pass_data(c, P, batch, seed + 12)
    msgs, outs = _run_dev(ctx, c, parties, shares, trip, limit=2)
    assert outs is None and len(msgs[0]) == 2
    bits, shares, trip = G.pass_data(c, P, batch, seed + 13)
    for g, x in zip(parties, shares):
        g.set_inputs(x)
    d_buf = ctx.zeros(max(2 * g0.info.max_level_words, g0.out_words, 1) * batch * 8)
    _arg_error(g0.get_outputs)                 # between the restart and the end of the pass
    _arg_error(g0.get_outputs_dev, d_buf)
    _arg_error(g0.step)                        # a step straight after the restart: the triples must be set again
    _arg_error(g0.step_dev, None, d_buf)
    for g, t in zip(parties, trip):
        g.set_triples(*t)
    msgs, cur = [[] for _ in range(P)], [None] * P
    assert not _host_steps(parties, msgs, cur, 1)
    _arg_error(g0.set_triples, *trip[0])       # after the first step
    _arg_error(g0.set_triples_dev, d_buf, d_buf, d_buf)
    _arg_error(g0.get_outputs)                 # in mid-pass
    assert _host_steps(parties, msgs, cur)
    outs = [g.get_outputs() for g in parties]
    assert _check_pass(c, P, batch, seed + 13, msgs, outs, bits, shares, trip, g0.last_launches) == n
    assert all(g.last_launches == n + 2 for g in parties)
    _arg_error(g0.step, np.stack(cur[1:]))  # a step after the end
    assert _one_pass(ctx, c, parties, batch, seed + 14, True) == n and g0.last_launches == n + 2
    d_buf.close()
    for g in parties:
        g.close()


def test_2_20_instances_of_aes_on_real_triples(ctx, aes_circ):
    """aes_128, 2 parties, 2^20 instances through the _dev forms with valid random triples: the slot store is 36 919 x 16 384
    words per party, so byte offsets pass 2^32.  300 distinct (key, plaintext) pairs are tiled over the batch, instance 0 the
    FIPS-197 C.1 vector: the XOR of the two output buffers is compared for all 2^20 instances with the tiled plaintext
    results; every message and the output shares are compared with R.run_parties on 256 sampled instances (the first and
    last 64 and both sides of three instance-word boundaries).  Device memory ~17.6 GB (arithmetic, not measured): slots
    2 x 36 919 x 16 384 x 8 B = 9.68 GB, triples 6 x 130 x 2^20 x 8 B = 6.54 GB, four message buffers of
    2 x max_level_words x 2^20 x 8 B, inputs and outputs 0.1 GB.  Host memory: three triple arrays of 1.09 GB at a time."""
    c, P, batch, K = aes_circ, 2, 1 << 20, 300
    tw = R.triple_words(c)[2]
    ws = _round_words(c)
    rng = np.random.default_rng(2020)

    def rand(rows):
        return rng.integers(0, 0xFFFFFFFFFFFFFFFF, (rows, batch), dtype=np.uint64, endpoint=True)

    small = rng.integers(0, 2, (K, c.num_inputs)).astype(np.uint8)
    key = int.from_bytes(bytes(range(16)), "big")
    pt = int.from_bytes(bytes.fromhex("00112233445566778899aabbccddeeff"), "big")
    small[0] = [(key >> i) & 1 for i in range(128)] + [(pt >> i) & 1 for i in range(128)]
    plain = G.plain_bucketed_batch(c, small)  # [128][K]
    ct = sum(int(v) << i for i, v in enumerate(plain[:, 0]))
    assert ct.to_bytes(16, "big").hex() == "69c4e0d86a7b0430d8cdb78070b4c55a"
    assert (plain[:, 1] == c.compute_bits(small[1])[c.NumWires - c.num_outputs:]).all()
    reps = -(-batch // K)
    want = np.tile(R.pack(plain), (1, reps))[:, :batch]
    ranges = [(0, 64), (333 * 64 - 16, 333 * 64 + 16), ((1 << 19) - 32, (1 << 19) + 32),
              (batch - (1 << 16) - 16, batch - (1 << 16) + 16), (batch - 64, batch)]
    idx = np.concatenate([np.arange(lo, hi) for lo, hi in ranges])
    assert len(idx) == 256

    s0 = rand((c.num_inputs + 63) // 64)
    shares = [s0, s0 ^ np.tile(R.pack(small.T), (1, reps))[:, :batch]]
    d_in = [ctx.to_device(x) for x in shares]
    s_in = [x[:, idx].copy() for x in shares]
    del s0, shares
    # triples, one array at a time: upload, keep the sampled columns, fold into c1 = (a0 ^ a1) & (b0 ^ b1) ^ c0
    d_t = [[None] * 3 for _ in range(P)]
    s_t = [[None] * 3 for _ in range(P)]

    def put(p, k, arr):
        d_t[p][k] = ctx.to_device(arr)
        s_t[p][k] = arr[:, idx].copy()

    acc = rand(tw)
    put(0, 0, acc)
    x = rand(tw)
    put(1, 0, x)
    acc ^= x  # a0 ^ a1
    xb = rand(tw)
    put(0, 1, xb)
    x = rand(tw)
    put(1, 1, x)
    xb ^= x  # b0 ^ b1
    acc &= xb
    del xb
    x = rand(tw)
    put(0, 2, x)
    acc ^= x
    put(1, 2, acc)
    del x, acc

    parties = _make(ctx, c, P, batch)
    assert parties[0].info.ninputs + parties[0].info.ngates == 36919
    assert 36919 * ((batch + 63) // 64) * 8 > 1 << 32
    maxw = max(ws)
    mb = [[ctx.empty(2 * maxw * batch * 8) for _ in range(P)] for _ in range(2)]
    d_out = [ctx.empty(2 * batch * 8) for _ in range(P)]
    for g, d, t in zip(parties, d_in, d_t):
        g.set_inputs_dev(d)
        g.set_triples_dev(*t)
    msgs = [[] for _ in range(P)]
    r = 0
    while True:
        w_prev = ws[r - 1] if r else 0
        w = ws[r] if r < len(ws) else 0
        res = [g.step_dev(mb[(r - 1) & 1][1 - p] if w_prev else None, mb[r & 1][p] if w else None) for p, g in enumerate(parties)]
        assert res[0] == res[1] and res[0][1] == w
        if not w:
            assert res[0][0] == len(R.buckets(c)[0])
            break
        for p in range(P):
            rows = [np.concatenate([mb[r & 1][p].download(np.uint64, None, (row * batch + lo) * 8, (hi - lo) * 8) for lo, hi in ranges])
                    for row in range(2 * w)]
            msgs[p].append((res[0][0], np.stack(rows).reshape(2, w, len(idx))))
        r += 1
    outs = []
    for p, g in enumerate(parties):
        g.get_outputs_dev(d_out[p])
        outs.append(d_out[p].download(np.uint64, (2, batch)))
    assert all(g.last_launches == len(ws) + 2 == 62 for g in parties)
    assert np.array_equal(outs[0] ^ outs[1], want)  # all 2^20 instances
    ref_msgs, ref_outs = R.run_parties(c, s_in, [tuple(t) for t in s_t])
    for p in range(P):
        assert [lv for lv, _ in msgs[p]] == [lv for lv, _ in ref_msgs[p]] and len(msgs[p]) == 60
        for (lv, m), (_, rm) in zip(msgs[p], ref_msgs[p]):
            assert m.shape == rm.shape and (m == rm).all(), "party %d level %d: message differs from the reference's" % (p, lv)
        assert (outs[p][:, idx] == ref_outs[p]).all()
    for g in parties:
        g.close()
    for b in d_in + [x for t in d_t for x in t] + mb[0] + mb[1] + d_out:
        b.close()
    ctx.sync()


@pytest.mark.parametrize("words", [1, 255, 256, 257, (1 << 24) + 3])
def test_triple_folds_whole_buffers(ctx, words):
    """each of the four folds against numpy over the whole buffer, and the word after the end of the written buffer
    untouched.  One sweep of k_gmw_fold's grid is 65 536 blocks x 256 threads = 2^24 words: at 2^24 + 3 the grid-stride
    loop goes round for three threads.  Device memory at that size: 4 x 134 MB = 0.54 GB."""
    rng = np.random.default_rng(words)
    x, y, z, c0 = (rng.integers(0, 0xFFFFFFFFFFFFFFFF, words + 1, dtype=np.uint64, endpoint=True) for _ in range(4))
    d_x, d_y, d_z, d_c = (ctx.to_device(v) for v in (x, y, z, c0))

    def check(want):
        got = d_c.download(np.uint64)
        assert got[words] == c0[words], "the word after the end was written"
        assert np.array_equal(got[:words], want[:words])
        d_c.upload(c0)

    engine.gmw_triples_local_dev(ctx, d_x, d_y, d_c, words)
    check(x & y)
    engine.gmw_triples_sender_u_dev(ctx, 0, d_x, d_c, words)
    check(x)
    engine.gmw_triples_sender_u_dev(ctx, 1, d_x, d_c, words)
    check(~x)
    engine.gmw_triples_sender_fold_dev(ctx, d_x, d_y, d_z, d_c, words)
    check(c0 ^ x ^ (y & z))
    engine.gmw_triples_receiver_fold_dev(ctx, d_x, d_c, words)
    check(c0 ^ x)
    for b in (d_x, d_y, d_z, d_c):
        b.close()


def _device_triples(ctx, P, words, seed):
    """tripleBatch on the device: real bit-COT (gc_iknp_*_bits_dev) for every ordered pair, then the four folds"""
    rng = np.random.default_rng(seed)
    n = 64 * words  # whole words: the reference folds whole choice words only (iknp.go:583-597)
    a = [rng.integers(0, 2 ** 63, words, dtype=np.int64).astype(np.uint64) ^ (rng.integers(0, 2, words).astype(np.uint64) << np.uint64(63))
         for _ in range(P)]
    b = [rng.integers(0, 2 ** 63, words, dtype=np.int64).astype(np.uint64) ^ (rng.integers(0, 2, words).astype(np.uint64) << np.uint64(63))
         for _ in range(P)]
    d_a = [ctx.to_device(x) for x in a]
    d_b = [ctx.to_device(x) for x in b]
    d_c = [ctx.zeros(words * 8) for _ in range(P)]
    for p in range(P):
        engine.gmw_triples_local_dev(ctx, d_a[p], d_b[p], d_c[p], words)
    cot, bufs, handles = {}, [], []
    d_u = ctx.zeros(((n + 511) // 512) * 8192)
    d_uv = ctx.zeros(words * 8)
    for s in range(P):
        for r in range(P):
            if s == r:
                continue
            base, delta, k0 = base_setup("gmw-%d-%d-%d" % (seed, s, r))
            rcv, snd = engine.IKNPReceiver(ctx, base), engine.IKNPSender(ctx, delta, k0)
            handles += [rcv, snd]
            d_s, d_r = ctx.zeros(words * 8), ctx.zeros(words * 8)
            bufs += [d_s, d_r]
            rcv.receive_bits_dev(d_b[r], n, d_u, d_r)  # choices = b of the receiver (triples.go:375, :402)
            snd.send_bits_dev(d_u, n, d_s)
            dbit = oracle.label_bit(delta, 0)
            engine.gmw_triples_sender_u_dev(ctx, dbit, d_a[s], d_uv, words)     # u = a ^ Delta   (:340-349)
            engine.gmw_triples_sender_fold_dev(ctx, d_s, d_uv, d_b[r], d_c[s], words)  # v = b of r (:362-364)
            engine.gmw_triples_receiver_fold_dev(ctx, d_r, d_c[r], words)        # (:387-389)
            cot[(s, r)] = (dbit, d_s, d_r)
    ctx.sync()
    cot = {k: (v[0], v[1].download(np.uint64), v[2].download(np.uint64)) for k, v in cot.items()}
    c = [x.download(np.uint64) for x in d_c]
    for h in handles:
        h.close()
    for x in bufs + d_a + d_b + d_c + [d_u, d_uv]:
        x.close()
    return a, b, c, cot


@pytest.mark.parametrize("P", [2, 3])
def test_triple_folds_on_real_bitcot(ctx, P):
    words = 96
    a, b, c, cot = _device_triples(ctx, P, words, 11 + P)
    want, _ = R.triple_batch(a, b, cot)
    for p in range(P):
        assert (c[p] == want[p]).all()
    xa = np.bitwise_xor.reduce(np.stack(a), axis=0)
    xb = np.bitwise_xor.reduce(np.stack(b), axis=0)
    assert (np.bitwise_xor.reduce(np.stack(c), axis=0) == (xa & xb)).all()
    # the u the sender would send (triples.go:340-352), from the fold kernel alone
    d_a, d_u = ctx.to_device(a[0]), ctx.zeros(words * 8)
    engine.gmw_triples_sender_u_dev(ctx, 1, d_a, d_u, words)
    assert (d_u.download(np.uint64) == ~a[0]).all()
    engine.gmw_triples_sender_u_dev(ctx, 0, d_a, d_u, 0)  # zero words: nothing launched
    d_a.close(); d_u.close()


def test_end_to_end_aes_on_device_triples(ctx, aes_circ):
    """device-made triples feed the online phase of aes_128, batch 4096, 2 parties; instance 0 is FIPS-197 C.1 (key then
    plaintext, LSB-first: the wire order of tests/test_oracle_circuits.py)"""
    c, P, batch = aes_circ, 2, 4096
    tw = R.triple_words(c)[2]
    a, b, cc, _ = _device_triples(ctx, P, tw * batch, 77)
    trip = [tuple(x.reshape(tw, batch) for x in (a[p], b[p], cc[p])) for p in range(P)]
    rng = np.random.default_rng(78)
    bits = rng.integers(0, 2, (batch, c.num_inputs)).astype(np.uint8)
    key = int.from_bytes(bytes(range(16)), "big")
    pt = int.from_bytes(bytes.fromhex("00112233445566778899aabbccddeeff"), "big")
    bits[0] = [(key >> i) & 1 for i in range(128)] + [(pt >> i) & 1 for i in range(128)]
    shares = R.share_inputs(rng, c, bits, P)
    parties = [engine.Gmw(ctx, c, P, p, batch) for p in range(P)]
    msgs, outs = _run_dev(ctx, c, parties, shares, trip)
    assert len(msgs[0]) == 60 and parties[0].last_launches <= 62
    ob = R.unpack(outs[0] ^ outs[1], c.num_outputs)
    ct = sum(int(v) << i for i, v in enumerate(ob[:, 0]))
    assert ct.to_bytes(16, "big").hex() == "69c4e0d86a7b0430d8cdb78070b4c55a"
    for i in (1, 2, batch - 1):
        assert (ob[:, i] == c.compute_bits(bits[i])[c.NumWires - c.num_outputs:]).all()
    for g in parties:
        g.close()


def test_misuse_is_rejected(ctx, add64_circ):
    c = add64_circ
    L = engine.lib()
    for P, p, batch in ((2, 2, 8), (2, 5, 8), (1, 0, 8), (2, 0, 0)):
        with pytest.raises(engine.EngineError) as e:
            engine.Gmw(ctx, c, P, p, batch)
        assert e.value.code == engine.GC_E_ARG
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2, (8, c.num_inputs)).astype(np.uint8)
    shares = R.share_inputs(rng, c, bits, 2)
    trip = R.beaver_triples(rng, 2, R.triple_words(c)[2], 8)
    g = engine.Gmw(ctx, c, 2, 0, 8)
    with pytest.raises(engine.EngineError) as e:  # a step before inputs
        g.step()
    assert e.value.code == engine.GC_E_ARG
    g.set_inputs(shares[0])
    with pytest.raises(engine.EngineError) as e:  # a step before the triples
        g.step()
    assert e.value.code == engine.GC_E_ARG
    g.set_triples(*trip[0])
    d_msg = ctx.zeros(2 * 8 * 8)
    with pytest.raises(engine.EngineError) as e:  # wrong npeers
        g.step_dev(None, d_msg, npeers=2)
    assert e.value.code == engine.GC_E_ARG
    with pytest.raises(engine.EngineError) as e:  # outputs before the pass ended
        g.get_outputs()
    assert e.value.code == engine.GC_E_ARG
    g.close()
    # a whole pass, then a step after its end
    parties = [engine.Gmw(ctx, c, 2, p, 8) for p in range(2)]
    _run_host(parties, shares, trip)
    with pytest.raises(engine.EngineError) as e:
        parties[0].step(np.zeros((1, 2, 0, 8), np.uint64))
    assert e.value.code == engine.GC_E_ARG
    for x in parties:
        x.close()
    d_msg.close()
    assert L.gc_gmw_last_launches(None) == 0


def test_two_handles_on_one_ctx_do_not_interfere(ctx, add64_circ, aes_circ):
    """two 2-party sessions (different circuits, batches and inputs) on one ctx, stepped round by round in turn"""
    sessions = []
    for k, (c, batch) in enumerate(((add64_circ, 70), (aes_circ, 5))):
        rng = np.random.default_rng(900 + k)
        bits = rng.integers(0, 2, (batch, c.num_inputs)).astype(np.uint8)
        shares = R.share_inputs(rng, c, bits, 2)
        trip = R.beaver_triples(rng, 2, R.triple_words(c)[2], batch)
        parties = [engine.Gmw(ctx, c, 2, p, batch) for p in range(2)]
        for g, x, t in zip(parties, shares, trip):
            g.set_inputs(x)
            g.set_triples(*t)
        sessions.append(dict(c=c, bits=bits, parties=parties, cur=[None, None], done=False))
    while not all(s["done"] for s in sessions):
        for s in sessions:
            if s["done"]:
                continue
            cur = s["cur"]
            new = [g.step(None if cur[0] is None else cur[1 - p][None]) for p, g in enumerate(s["parties"])]
            s["cur"] = [m for _, m in new]
            s["done"] = new[0][1].shape[1] == 0
    for s in sessions:
        c = s["c"]
        x = s["parties"][0].get_outputs() ^ s["parties"][1].get_outputs()
        ob = R.unpack(x, c.num_outputs)
        for i in range(s["bits"].shape[0]):
            assert (ob[:, i] == c.compute_bits(s["bits"][i])[c.NumWires - c.num_outputs:]).all()
        for g in s["parties"]:
            g.close()
