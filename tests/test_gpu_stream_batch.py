"""S sessions of one streamed program per call (gc_stream_batch_* / gc_stream_eval_batch_*) against the oracle's Streaming.Garble
and StreamEvaluator run per session with that session's key and random stream: every byte of every session's stream, the
wire stores, the evaluator's labels and plaintext bits, tampered blocks, and the steps that are refused."""
import hashlib

import numpy as np
import pytest

import oracle
from mpc_amd import engine
from mpc_amd.circuit import LABEL, WIRE
from tests import hostile_fuzz as hf
from tests import keyed_geometry as kg
from tests.test_oracle_stream import make_program, plain_program
from tests.test_stream_batch_host import STEP_BYTES, alias_gates

pytestmark = pytest.mark.gpu

FILL = 0xA5  # what the output buffer holds where no step may write


def rnd_streams(tag, S, n):
    seed = int.from_bytes(("stream-batch/" + tag).encode(), "big") % (1 << 63)
    r = np.random.default_rng(seed).integers(0, 256, (S, 1 + n, 16), dtype=np.uint8)
    assert len({x.tobytes() for x in r}) == S
    return r


def stride_for(total):
    """a multiple of 4 that is no multiple of 16: the sessions' streams start at every 4-byte alignment"""
    st = (total + 3) & ~3
    return st + 4 if st % 16 == 0 else st


_refs = {}


def reference(S, base, keylen):
    """the oracle, once per shape: keys, random streams, per session the step bytes and every program wire, the evaluator's
    input bits, its output labels and the plaintext values"""
    if (S, base, keylen) in _refs:
        return _refs[(S, base, keylen)]
    steps, prim = make_program(base)
    keys = kg.edge_keys("stream-batch", S, keylen)
    rnd = rnd_streams("%d/%d" % (S, base), S, len(prim))
    outs = [o for _, _, out_ in steps for o in out_]
    bits = np.random.default_rng(S + base + keylen).integers(0, 2, (S, len(prim)), dtype=np.uint8)
    streams, wires, ev = [], {w: np.zeros(S, WIRE) for w in prim + outs}, {o: [] for o in outs}
    vals = []
    for s in range(S):
        g = oracle.Stream(keys[s].tobytes(), rnd[s].tobytes(), prim)
        e = oracle.StreamEval(keys[s].tobytes())
        for w, b in zip(prim, bits[s]):
            wire = g.get(w)
            e.set(w, wire["l1"] if b else wire["l0"])
        mine = []
        for c, in_, out_ in steps:
            data = g.garble(c.Gates, c.NumWires, in_, out_)
            assert e.circuit(c.NumGates, c.NumWires, max(max(in_), max(out_)) + 1, data) == len(data)
            mine.append(data)
        streams.append(mine)
        for w in prim + outs:
            wires[w][s] = g.get(w)
        for o in outs:
            ev[o].append(e.get(o))
        vals.append(plain_program(steps, prim, bits[s]))
    assert tuple(len(x) for x in streams[0]) == STEP_BYTES[base]
    _refs[(S, base, keylen)] = dict(steps=steps, prim=prim, keys=keys, rnd=rnd, streams=streams, wires=wires, outs=outs, bits=bits,
                                    ev=ev, vals=vals)
    return _refs[(S, base, keylen)]


class Run:
    """the garbler's side of the program on the device: the steps appended per session at running offsets"""

    def __init__(self, ctx, ref, S, keylen, keys=None, lead=0):
        self.ref, self.S = ref, S
        self.total = sum(len(x) for x in ref["streams"][0])
        self.stride, self.lead = stride_for(self.total), lead
        self.d_keys = engine.DeviceBuffer(ctx, data=ref["keys"] if keys is None else keys)
        self.d_rnd = engine.DeviceBuffer(ctx, data=ref["rnd"])
        self.d_out = engine.DeviceBuffer(ctx, data=np.full(lead + S * self.stride + 16, FILL, np.uint8))
        self.sb = engine.StreamBatch(ctx, S, self.d_keys, keylen, self.d_rnd, ref["prim"])
        self.offs, off = [], 0
        for c, in_, out_ in ref["steps"]:
            n = self.sb.garble(c.Gates, c.NumWires, in_, out_, self.d_out + (lead + off), self.stride)
            assert n == engine.stream_batch_step_bytes(c.Gates, c.NumWires, in_, out_)
            self.offs.append(off)
            off += n
        assert off == self.total
        self.buf = self.d_out.numpy()

    def session(self, s):
        at = self.lead + s * self.stride
        return self.buf[at: at + self.total].tobytes()

    def untouched(self):
        """nothing was written in front of the first stream, between two streams or behind the last"""
        b = self.buf
        ok = (b[: self.lead] == FILL).all() and (b[self.lead + self.S * self.stride:] == FILL).all()
        gaps = b[self.lead: self.lead + self.S * self.stride].reshape(self.S, self.stride)[:, self.total:]
        return ok and (gaps == FILL).all()

    def close(self):
        self.sb.close()
        for d in (self.d_keys, self.d_rnd, self.d_out):
            d.close()


def check_store(sb, ref, sessions=None):
    for w, want in ref["wires"].items():
        got = sb.get(w)
        idx = slice(None) if sessions is None else sessions
        assert (got[idx] == want[idx]).all(), "wire %d" % w


@pytest.mark.parametrize("base,keylen,lead", [(0, 32, 0), (0x20000, 16, 3), (0x20000, 24, 9)])
def test_five_sessions_bytes_and_store_equal_the_oracle(base, keylen, lead):
    S = 5
    ctx = engine.Context(0)
    ref = reference(S, base, keylen)
    run = Run(ctx, ref, S, keylen, lead=lead)
    assert run.stride % 16 != 0
    for s in range(S):
        assert run.session(s) == b"".join(ref["streams"][s]), "session %d" % s
    assert run.untouched()
    check_store(run.sb, ref)
    run.close()
    ctx.close()


@pytest.mark.parametrize("S,ti", [(67, 1), (1027, 4)])
def test_many_sessions_ragged_wave_and_ragged_tile(S, ti):
    ctx = engine.Context(0)
    ref = reference(S, 0, 32)
    run = Run(ctx, ref, S, 32, lead=5)
    want = [hashlib.sha256(b"".join(x)).digest() for x in ref["streams"]]
    got = [hashlib.sha256(run.session(s)).digest() for s in range(S)]
    assert [s for s in range(S) if got[s] != want[s]] == []
    sample = kg.sample(S, ti) if S > 100 else range(S)
    assert len(sample) >= 40
    for s in sample:
        assert run.session(s) == b"".join(ref["streams"][s]), "session %d" % s
    assert run.untouched()
    check_store(run.sb, ref)
    run.close()
    ctx.close()


def test_in_place_step_twice():
    """in = [0, 1], out = [0, 2]: a gate that reads global 0 after the gate that set it sees the new label — bytes and store
    equal the oracle's both times"""
    S, prim, gates = 5, [0, 1, 2], alias_gates()
    ctx = engine.Context(0)
    keys = kg.edge_keys("stream-batch/alias", S, 32)
    rnd = rnd_streams("alias", S, len(prim))
    ogs = [oracle.Stream(keys[s].tobytes(), rnd[s].tobytes(), prim) for s in range(S)]
    d_keys, d_rnd = engine.DeviceBuffer(ctx, data=keys), engine.DeviceBuffer(ctx, data=rnd)
    sb = engine.StreamBatch(ctx, S, d_keys, 32, d_rnd, prim)
    n = engine.stream_batch_step_bytes(gates, 5, [0, 1], [0, 2])
    stride = stride_for(n)
    d_out = engine.DeviceBuffer(ctx, shape=S * stride + 16)
    for rep in range(2):
        d_out.zero(FILL)
        assert sb.garble(gates, 5, [0, 1], [0, 2], d_out + 1, stride) == n
        buf = d_out.numpy()
        for s in range(S):
            want = ogs[s].garble(gates, 5, [0, 1], [0, 2])
            assert buf[1 + s * stride: 1 + s * stride + n].tobytes() == want, (rep, s)
        for w in prim:
            got = sb.get(w)
            for s in range(S):
                assert got[s] == ogs[s].get(w), (rep, w, s)
    sb.close()
    ctx.close()


def test_two_sessions_with_swapped_keys_change_alone():
    S = 5
    ctx = engine.Context(0)
    ref = reference(S, 0, 32)
    keys = ref["keys"].copy()
    keys[[1, 3]] = keys[[3, 1]]
    a, b = Run(ctx, ref, S, 32), Run(ctx, ref, S, 32, keys=keys)
    changed = [s for s in range(S) if a.session(s) != b.session(s)]
    assert changed == [1, 3]
    for s in (0, 2, 4):
        assert b.session(s) == b"".join(ref["streams"][s])
    a.close(), b.close()
    ctx.close()


def active_labels(ref, S):
    """gc_label [S][prim]: L0 ^ bit * R of every primary input, from the oracle's wires"""
    lab = np.zeros((S, len(ref["prim"])), LABEL)
    for j, w in enumerate(ref["prim"]):
        wire = ref["wires"][w]
        lab[:, j] = np.where(ref["bits"][:, j] == 1, wire["l1"], wire["l0"])
    return lab


def evaluator_for(ctx, ref, run, S, keylen):
    se = engine.StreamEvalBatch(ctx, S, run.d_keys, keylen)
    se.set_wires(ref["prim"], engine.DeviceBuffer(ctx, data=active_labels(ref, S)))
    return se


def eval_step(se, ref, k, ref_block, d_blocks, stride, d_bad):
    c, in_, out_ = ref["steps"][k]
    return se.circuit(c.NumGates, c.NumWires, max(max(in_), max(out_)) + 1, ref_block, d_blocks, stride, d_bad)


@pytest.mark.parametrize("S", [5, 1027])
def test_evaluator_reads_the_garblers_device_buffer(S):
    ctx = engine.Context(0)
    ref = reference(S, 0, 32)
    run = Run(ctx, ref, S, 32, lead=2)
    se = evaluator_for(ctx, ref, run, S, 32)
    d_bad = engine.DeviceBuffer(ctx, shape=S, dtype=np.uint32)
    for k in range(3):
        block = ref["streams"][S // 2][k]  # any one session's bytes
        used = eval_step(se, ref, k, block, run.d_out + (run.lead + run.offs[k]), run.stride, d_bad)
        assert used == len(block)
        assert (d_bad.numpy() == 0).all()
    for o in ref["outs"]:
        got, wire = se.get(o), ref["wires"][o]
        for s in range(S):
            assert (int(got[s]["d0"]), int(got[s]["d1"])) == ref["ev"][o][s], (o, s)
        val = np.array([ref["vals"][s][o] for s in range(S)])
        assert (got == np.where(val == 1, wire["l1"], wire["l0"])).all(), o
    se.close(), run.close()
    ctx.close()


def test_evaluator_with_tampered_blocks():
    """the faults are in the DATA: a session whose structure bytes differ is counted, a changed row byte is evaluated as it is,
    and nobody else's labels move"""
    S = 6
    ctx = engine.Context(0)
    ref = reference(S, 0, 32)
    run = Run(ctx, ref, S, 32)
    c, in_, out_ = ref["steps"][0]
    n = len(ref["streams"][0][0])
    gates, err = hf.parse(ref["streams"][0][0], c.NumGates)
    assert err is None
    xor = [q for q in gates if q[1] == 0][1]
    rowed = [q for q in gates if q[7]][2]
    blocks = run.buf[: S * run.stride].reshape(S, run.stride).copy()
    blocks[2, xor[0]] ^= 0x01              # XOR -> XNOR: one op-nibble bit
    blocks[3, gates[5][5][0] + 1] ^= 0x04  # a wire id byte
    blocks[4, rowed[6] + 7] ^= 0x40        # a ROW byte
    d_blocks = engine.DeviceBuffer(ctx, data=blocks)
    se = evaluator_for(ctx, ref, run, S, 32)
    d_bad = engine.DeviceBuffer(ctx, shape=S, dtype=np.uint32)
    assert eval_step(se, ref, 0, ref["streams"][0][0], d_blocks, run.stride, d_bad) == n
    bad = d_bad.numpy()
    assert bad[2] != 0 and bad[3] != 0 and (bad[[0, 1, 4, 5]] == 0).all(), bad
    # session 4: what StreamEvaluator computes from the tampered bytes
    oe = oracle.StreamEval(ref["keys"][4].tobytes())
    lab = active_labels(ref, S)
    for j, w in enumerate(ref["prim"]):
        oe.set(w, lab[4, j])
    oe.circuit(c.NumGates, c.NumWires, max(max(in_), max(out_)) + 1, blocks[4, :n].tobytes())
    for o in out_:
        got = se.get(o)
        assert (int(got[4]["d0"]), int(got[4]["d1"])) == oe.get(o), o
        for s in (0, 1, 5):
            assert (int(got[s]["d0"]), int(got[s]["d1"])) == ref["ev"][o][s], (o, s)
    # a truncated len: what the one-session evaluator answers
    one = engine.StreamEval(ctx, ref["keys"][0].tobytes())
    with pytest.raises(engine.EngineError) as want:
        one.circuit(c.NumGates, c.NumWires, max(max(in_), max(out_)) + 1, ref["streams"][0][0][: n - 1])
    with pytest.raises(engine.EngineError) as got:
        eval_step(se, ref, 0, ref["streams"][0][0][: n - 1], d_blocks, run.stride, d_bad)
    assert got.value.code == want.value.code == engine.GC_E_ROWS
    one.close(), se.close(), run.close()
    ctx.close()


def test_gather_wires_to_set_wires_round_trip():
    S = 67
    ctx = engine.Context(0)
    ref = reference(S, 0, 32)
    run = Run(ctx, ref, S, 32)
    prim = ref["prim"]
    d_w = engine.DeviceBuffer(ctx, shape=(S, len(prim)), dtype=WIRE)
    run.sb.gather_wires(prim, d_w)
    pairs = d_w.numpy()
    for j, w in enumerate(prim):
        assert (pairs[:, j] == run.sb.get(w)).all(), w
    se = engine.StreamEvalBatch(ctx, S, run.d_keys, 32)
    se.set_wires(prim, engine.DeviceBuffer(ctx, data=np.ascontiguousarray(pairs["l1"])))
    for j, w in enumerate(prim):
        assert (se.get(w) == ref["wires"][w]["l1"]).all(), w
    se.close(), run.close()
    ctx.close()


def test_step_outside_the_keyed_scope_is_refused_and_the_store_stays():
    S = 3
    ctx = engine.Context(0)
    c = kg.build("edge_over")
    dc = engine.DeviceCircuit(ctx, c)
    b = engine.Batch(dc, S)
    assert not kg.predict("edge_over", S).keyed and not b.keyed_supported()
    b.close(), dc.close()
    prim = list(range(8))
    in_ = [i % 8 for i in range(c.num_inputs)]
    keys, rnd = kg.edge_keys("stream-batch/edge", S, 32), rnd_streams("edge", S, len(prim))
    sb = engine.StreamBatch(ctx, S, engine.DeviceBuffer(ctx, data=keys), 32, engine.DeviceBuffer(ctx, data=rnd), prim)
    before = [sb.get(w).copy() for w in prim + [9]]
    n = engine.stream_batch_step_bytes(c.Gates, c.NumWires, in_, [9])
    d_out = engine.DeviceBuffer(ctx, shape=S * ((n + 3) & ~3))
    with pytest.raises(engine.EngineError) as err:
        sb.garble(c.Gates, c.NumWires, in_, [9], d_out, (n + 3) & ~3)
    assert err.value.code == engine.GC_E_ARG
    assert "gc_batch_keyed_supported" in engine.lib().gc_last_error().decode()
    for w, want in zip(prim + [9], before):
        assert (sb.get(w) == want).all(), w
    sb.close()
    ctx.close()
