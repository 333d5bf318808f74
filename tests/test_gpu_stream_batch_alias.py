"""In-place steps of the session-batched stream (rewrite_aliased and last_wins of stream_batch.cpp) beyond the one fixed
four-gate circuit of test_in_place_step_twice: NSTEPS seeded steps of 8 to 40 gates over all five gate types, chained on one
handle for S = 3 sessions, every step applied twice in a row.  out[] shares one to all of its ids with in[]; an id is repeated
inside out[] (the later output is Set later: it is the one the store keeps) or inside in[]; gates read an input-mapped wire
both before and after the gate that sets the output mapped to the same global id.

After every application: each session's bytes equal the oracle's Streaming.Garble and the one-session gc_stream_garble (the
original rewrite_aliased) for that session's key and random stream, the whole store equals the oracle's, and the evaluator
handle fed the device bytes holds the oracle StreamEvaluator's label on every wire.

What the generated steps leave out, because the one-session stream they are also compared with resolves it by index where the
reference resolves it by time: an id repeated inside out[] is never one of in[]'s, its outputs are Set in the order of their
indices, and no gate reads them back.  test_an_id_repeated_in_out_is_resolved_in_gate_order runs exactly that on the batched
handles alone: the store keeps what the last GATE Set, and every read sees the latest Set."""
import numpy as np
import pytest

import oracle
from mpc_amd import engine
from mpc_amd.circuit import GATE, INV, LABEL
from tests import keyed_geometry as kg
from tests.test_gpu_stream_batch import FILL, rnd_streams, stride_for

pytestmark = pytest.mark.gpu

S, KEYLEN = 3, 32
NSTEPS = 24
PRIM = list(range(10, 22))  # the program's primary inputs; outputs that alias nothing get ids from 40 up


_steps = []


def step(k):
    """(gates, nwires, in_, out_, {which of the shapes it has}) of step k; in_ draws on PRIM and on the outputs of the steps
    before it"""
    while len(_steps) <= k:
        _steps.append(_step(len(_steps), PRIM + sorted({w for st in _steps for w in st[3]} - set(PRIM))))
    return _steps[k]


def _step(k, pool):
    rng = np.random.default_rng([7, k])
    ngates = (8, 40)[k] if k < 2 else int(rng.integers(8, 41))
    nin, nout = int(rng.integers(3, 7)), int(rng.integers(2, 6))
    what = set()
    in_ = [int(w) for w in rng.choice(pool, nin, replace=False)]
    if k % 3 == 1:
        in_[-1] = in_[0]
        what.add("in repeats an id")
    distinct = list(dict.fromkeys(in_))
    repeat = k % 4 == 2  # the last two outputs share a fresh id
    free = nout - 2 if repeat else nout  # outputs that may alias an input
    share = min(len(distinct), free, 1 + k % free) if free else 0
    if not repeat and k % 5 == 0:
        share = min(len(distinct), nout)
    shared = [int(w) for w in rng.choice(distinct, share, replace=False)]
    out_ = shared + [40 + 8 * k + i for i in range(free - share)]
    out_ = [out_[i] for i in rng.permutation(len(out_))]
    if repeat:
        out_ += [40 + 8 * k + 7] * 2
        what.add("out repeats an id")
    if not shared:  # (nout == 2 and both repeat): alias through a third output
        out_.insert(0, distinct[0])
        shared, nout = [distinct[0]], nout + 1
    if set(out_) <= set(in_):
        what.add("all of out in in")
    nwires = nin + (ngates - nout) + nout
    first_out = nwires - nout
    # which gate Sets which output: in the order of the indices, none first and none last
    at = sorted(int(p) for p in rng.choice(np.arange(1, ngates - 1), nout, replace=False))
    setter = dict(zip(at, range(nout)))
    readable_out = [j for j in range(nout) if out_.count(out_[j]) == 1]
    gates = np.zeros(ngates, GATE)
    written, tmp = [], nin
    for g in range(ngates):
        op = int(rng.integers(0, 5)) if g >= 5 else g  # (every type in every step)
        srcs = list(range(nin)) + written
        a, b = (int(w) for w in rng.choice(srcs, 2))
        if g in setter:
            o = first_out + setter[g]
        else:
            o, tmp = tmp, tmp + 1
        gates[g] = (a, 0 if op == INV else b, o, op, 0)
        if o < first_out or setter[g] in readable_out:
            written.append(o)
    # an input-mapped wire read before AND after the gate that Sets the output of the same global id
    j = next(j for j in range(nout) if out_[j] in shared)
    i, p = in_.index(out_[j]), at[j]
    gates[p - 1]["in0"] = i
    gates[p + 1]["in0"] = i
    what.add("read before and after the set")
    assert tmp == first_out
    return gates, nwires, in_, out_, what


def test_generated_in_place_steps_twice_each():
    ctx = engine.Context(0)
    keys = kg.edge_keys("stream-batch/alias-gen", S, KEYLEN)
    rnd = rnd_streams("alias-gen", S, len(PRIM))
    bits = np.random.default_rng(11).integers(0, 2, (S, len(PRIM)), dtype=np.uint8)
    og = [oracle.Stream(keys[s].tobytes(), rnd[s].tobytes(), PRIM) for s in range(S)]
    oe = [oracle.StreamEval(keys[s].tobytes()) for s in range(S)]
    one = [engine.Stream(ctx, keys[s].tobytes(), rnd[s].tobytes(), PRIM) for s in range(S)]
    d_keys, d_rnd = engine.DeviceBuffer(ctx, data=keys), engine.DeviceBuffer(ctx, data=rnd)
    sb = engine.StreamBatch(ctx, S, d_keys, KEYLEN, d_rnd, PRIM)
    se = engine.StreamEvalBatch(ctx, S, d_keys, KEYLEN)
    active = np.zeros((S, len(PRIM)), LABEL)
    for s in range(S):
        for j, w in enumerate(PRIM):
            wire = og[s].get(w)
            active[s, j] = wire["l1"] if bits[s, j] else wire["l0"]
            oe[s].set(w, active[s, j])
    se.set_wires(PRIM, engine.DeviceBuffer(ctx, data=active))
    d_bad = engine.DeviceBuffer(ctx, shape=S, dtype=np.uint32)
    touched = list(PRIM)
    for k in range(NSTEPS):
        gates, nwires, in_, out_, _ = step(k)
        n = engine.stream_batch_step_bytes(gates, nwires, in_, out_)
        assert n > 0
        stride, lead = stride_for(n), 1 + k % 3
        d_out = engine.DeviceBuffer(ctx, shape=lead + S * stride + 16)
        touched += [w for w in out_ if w not in touched]
        for rep in range(2):
            tag = "step %d, application %d" % (k, rep)
            d_out.zero(FILL)
            assert sb.garble(gates, nwires, in_, out_, d_out + lead, stride) == n, tag
            buf = d_out.numpy()
            body = buf[lead: lead + S * stride].reshape(S, stride)
            assert (buf[:lead] == FILL).all() and (buf[lead + S * stride:] == FILL).all() and (body[:, n:] == FILL).all(), tag
            for s in range(S):
                want = og[s].garble(gates, nwires, in_, out_)
                assert body[s, :n].tobytes() == want, "%s, session %d against the oracle" % (tag, s)
                assert one[s].garble(gates, nwires, in_, out_) == want, "%s, session %d: gc_stream_garble against the oracle" % (tag, s)
            for w in touched:
                got = sb.get(w)
                for s in range(S):
                    assert got[s] == og[s].get(w), "%s: wire %d of session %d" % (tag, w, s)
            d_bad.zero(0xFF)
            nw = max(max(in_), max(out_)) + 1
            assert se.circuit(len(gates), nwires, nw, body[0, :n].tobytes(), d_out + lead, stride, d_bad) == n, tag
            assert (d_bad.numpy() == 0).all(), tag
            for s in range(S):
                assert oe[s].circuit(len(gates), nwires, nw, body[s, :n].tobytes()) == n
            for w in touched:
                got = se.get(w)
                for s in range(S):
                    assert (int(got[s]["d0"]), int(got[s]["d1"])) == oe[s].get(w), "%s: the evaluator's wire %d of session %d" % (tag, w, s)
        d_out.close()
    for x in one + [sb, se]:
        x.close()
    ctx.close()


def reordered_step():
    """out = [30, 30, 31] over in = [10, 11, 30]: global 30 is read through the wire of out[1] before any gate Set it, Set first
    through out[1], then through out[0] — the LATER gate, of the lower index — and read in between and afterwards through the
    input-mapped wire and through the wire of out[1]"""
    gates = np.zeros(7, GATE)
    gates[0] = (8, 0, 3, 4, 0)  # INV reads 30 through the wire of out[1]: the label the step began with
    gates[1] = (0, 3, 8, 2, 0)  # AND -> out[1]: 30 is Set
    gates[2] = (2, 0, 4, 0, 0)  # XOR reads 30 through in[2]: gate 1's label
    gates[3] = (4, 1, 7, 3, 0)  # OR  -> out[0]: 30 is Set again
    gates[4] = (2, 1, 5, 2, 0)  # AND reads 30 through in[2]: gate 3's label
    gates[5] = (8, 0, 6, 3, 0)  # OR  reads 30 through the wire of out[1]: gate 3's label too
    gates[6] = (5, 6, 9, 0, 0)  # XOR -> out[2]
    return gates, 10, [10, 11, 30], [30, 30, 31]


def test_an_id_repeated_in_out_is_resolved_in_gate_order():
    """the reference resolves every read and every Set through the global id at the time of the gate (stream_garble.go:131-157):
    the store keeps what the LAST GATE Set, whatever its index in out[], and a read sees the latest Set"""
    gates, nwires, in_, out_ = reordered_step()
    prim = [10, 11, 30]
    ctx = engine.Context(0)
    keys = kg.edge_keys("stream-batch/alias-order", S, KEYLEN)
    rnd = rnd_streams("alias-order", S, len(prim))
    og = [oracle.Stream(keys[s].tobytes(), rnd[s].tobytes(), prim) for s in range(S)]
    oe = [oracle.StreamEval(keys[s].tobytes()) for s in range(S)]
    d_keys, d_rnd = engine.DeviceBuffer(ctx, data=keys), engine.DeviceBuffer(ctx, data=rnd)
    sb = engine.StreamBatch(ctx, S, d_keys, KEYLEN, d_rnd, prim)
    se = engine.StreamEvalBatch(ctx, S, d_keys, KEYLEN)
    active = np.zeros((S, len(prim)), LABEL)
    for s in range(S):
        for j, w in enumerate(prim):
            active[s, j] = og[s].get(w)["l1" if (s + j) % 2 else "l0"]
            oe[s].set(w, active[s, j])
    se.set_wires(prim, engine.DeviceBuffer(ctx, data=active))
    n = engine.stream_batch_step_bytes(gates, nwires, in_, out_)
    stride = stride_for(n)
    d_out = engine.DeviceBuffer(ctx, shape=S * stride + 16)
    d_bad = engine.DeviceBuffer(ctx, shape=S, dtype=np.uint32)
    for rep in range(2):
        d_out.zero(FILL)
        assert sb.garble(gates, nwires, in_, out_, d_out, stride) == n
        body = d_out.numpy()[: S * stride].reshape(S, stride)
        for s in range(S):
            assert body[s, :n].tobytes() == og[s].garble(gates, nwires, in_, out_), (rep, s)
        for w in (10, 11, 30, 31):
            got = sb.get(w)
            for s in range(S):
                assert got[s] == og[s].get(w), (rep, w, s)
        d_bad.zero(0xFF)
        assert se.circuit(len(gates), nwires, 32, body[0, :n].tobytes(), d_out, stride, d_bad) == n
        assert (d_bad.numpy() == 0).all()
        for s in range(S):
            assert oe[s].circuit(len(gates), nwires, 32, body[s, :n].tobytes()) == n
        for w in (10, 11, 30, 31):
            got = se.get(w)
            for s in range(S):
                assert (int(got[s]["d0"]), int(got[s]["d1"])) == oe[s].get(w), (rep, w, s)
    sb.close(), se.close()
    ctx.close()
