"""GMW party engine on the GPU (gc_gmw_*, mpc_amd/csrc/gmw_engine.cpp + gmw_kernels.hip) against the plain-Python
restatement of the reference (tests/py_gmw_reference.py): every step's message (padding bits included), the output shares,
the plaintext result, the launch count; the Beaver-triple folds on real bit-COT outputs; an end-to-end AES pass on
device-made triples; misuse."""
import numpy as np
import pytest

import oracle
from mpc_amd import engine
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


def _run_host(parties, inputs, triples):
    """one pass of every party through the host forms; returns (msgs[p] = [(level, [2][w][batch])], outs[p])"""
    P = len(parties)
    for g, x, t in zip(parties, inputs, triples):
        g.set_inputs(x)
        g.set_triples(*t)
    msgs = [[] for _ in range(P)]
    cur = [None] * P
    while True:
        new = []
        for p, g in enumerate(parties):
            peers = None if cur[0] is None else np.stack([cur[q] for q in range(P) if q != p])
            new.append(g.step(peers))
        if new[0][1].shape[1] == 0:
            assert all(m.shape[1] == 0 for _, m in new)
            break
        for p in range(P):
            msgs[p].append(new[p])
        cur = [m for _, m in new]
    return msgs, [g.get_outputs() for g in parties]


def _run_dev(ctx, c, parties, inputs, triples):
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
    while True:
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
    outs = []
    for p, g in enumerate(parties):
        g.get_outputs_dev(d_out[p])
        outs.append(d_out[p].download(np.uint64, None, 0, outw * batch * 8).reshape(outw, batch))
    for b in d_in + [x for t in d_t for x in t] + xch + d_out:
        b.close()
    return msgs, outs


def _check_pass(c, P, batch, seed, msgs, outs, bits, shares, trip, launches):
    rng = np.random.default_rng(seed + 1)
    idx = _sample(batch, rng)
    ref_msgs, ref_outs = R.run_parties(c, [s[:, idx] for s in shares], [tuple(x[:, idx] for x in t) for t in trip])
    for p in range(P):
        assert [lv for lv, _ in msgs[p]] == [lv for lv, _ in ref_msgs[p]]
        for (lv, m), (_, rm) in zip(msgs[p], ref_msgs[p]):
            assert (m[:, :, idx] == rm).all(), "party %d level %d: message differs from the reference's" % (p, lv)
        assert (outs[p][:, idx] == ref_outs[p]).all()
    x = np.bitwise_xor.reduce(np.stack(outs), axis=0)
    ob = R.unpack(x[:, idx], c.num_outputs)
    for k, i in enumerate(idx[:24]):
        assert (ob[:, k] == R.plain_bucketed(c, bits[i])).all()
    ands, _ = R.buckets(c)
    n_and_levels = sum(1 for a in ands if a)
    assert launches <= n_and_levels + 2


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
