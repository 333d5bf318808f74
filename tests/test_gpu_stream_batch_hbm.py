"""A streamed program with a step whose circuit keeps its wires in HBM, for S sessions per call (gc_stream_batch_* /
gc_stream_eval_batch_*): the step takes path 2 of gc_batch_keyed_path (k_garble_hbm_keyed / k_eval_hbm_keyed) between the same
gather, scatter, serialiser and ingester as every other step.  Four steps on one handle: an 8-bit adder, kg.lds_edge(N_FIT + 16)
— no LDS plan fits its live set; before path 2 existed the handle refused it — with its inputs mapped onto eight store wires,
an in-place update, the adder again over the updated wires.

Every session's bytes equal what the one-session stream (gc_stream_*) and the oracle give for that session alone, the store
equals the oracle's in every touched wire, the evaluator handle over the S blocks gives the oracle's active labels with
d_bad == 0, and one session's block with a flipped skeleton byte is counted for that session only."""
import types

import numpy as np
import pytest

import oracle
from mpc_amd import circuit, engine
from mpc_amd.circuit import WIRE
from tests import hostile_fuzz as hf
from tests import keyed_geometry as kg
from tests.test_gpu_stream_batch import Run, active_labels, check_store, eval_step, rnd_streams
from tests.test_stream_batch_host import alias_gates

pytestmark = pytest.mark.gpu

KEYLEN = 32


def program():
    add = circuit.adder(8)
    edge = kg.lds_edge(kg.N_FIT + 16)
    ag = alias_gates()
    alias = types.SimpleNamespace(Gates=ag, NumGates=len(ag), NumWires=5, num_inputs=2, num_outputs=2)
    prim = list(range(add.num_inputs))
    out1 = [100 + j for j in range(add.num_outputs)]
    out4 = [300 + j for j in range(add.num_outputs)]
    steps = [(add, prim, out1), (edge, [i % 8 for i in range(edge.num_inputs)], [200]), (alias, [0, 1], [0, 2]), (add, prim, out4)]
    return steps, prim


_refs = {}


def reference(S):
    """the oracle once per S, in the form of tests/test_gpu_stream_batch.reference; `wires` holds the FINAL store, `ev` the
    evaluator's label of every output when its step was done"""
    if S in _refs:
        return _refs[S]
    steps, prim = program()
    keys = kg.edge_keys("stream-batch/hbm", S, KEYLEN)
    rnd = rnd_streams("hbm/%d" % S, S, len(prim))
    bits = np.random.default_rng(S).integers(0, 2, (S, len(prim)), dtype=np.uint8)
    touched = sorted(set(prim) | {o for _, _, out_ in steps for o in out_})
    streams, wires, first = [], {w: np.zeros(S, WIRE) for w in touched}, {w: np.zeros(S, WIRE) for w in prim}
    ev = {w: [] for w in touched}
    for s in range(S):
        g = oracle.Stream(keys[s].tobytes(), rnd[s].tobytes(), prim)
        e = oracle.StreamEval(keys[s].tobytes())
        for w, b in zip(prim, bits[s]):
            wire = g.get(w)
            first[w][s] = wire
            e.set(w, wire["l1"] if b else wire["l0"])
        mine = []
        for c, in_, out_ in steps:
            data = g.garble(c.Gates, c.NumWires, in_, out_)
            assert e.circuit(c.NumGates, c.NumWires, max(max(in_), max(out_)) + 1, data) == len(data)
            mine.append(data)
        streams.append(mine)
        for w in touched:
            wires[w][s] = g.get(w)
            ev[w].append(e.get(w))
    _refs[S] = dict(steps=steps, prim=prim, keys=keys, rnd=rnd, streams=streams, wires=wires, first=first, bits=bits, ev=ev,
                    touched=touched)
    return _refs[S]


def initial_labels(ref, S):
    """active_labels over the primary inputs as they were BEFORE the in-place step"""
    return active_labels(dict(ref, wires=ref["first"]), S)


@pytest.mark.parametrize("S", [3, 70])
def test_program_with_an_hbm_wire_step(S):
    ctx = engine.Context(0)
    ref = reference(S)
    c_edge = ref["steps"][1][0]
    dc = engine.DeviceCircuit(ctx, c_edge)
    b = engine.Batch(dc, S)
    assert not b.lds_wires and b.keyed_path == 2
    b.close(), dc.close()
    run = Run(ctx, ref, S, KEYLEN, lead=3)
    # every session's bytes: the oracle's, and what the one-session stream gives for that session alone
    for s in range(S):
        assert run.session(s) == b"".join(ref["streams"][s]), "session %d against the oracle" % s
        one = engine.Stream(ctx, ref["keys"][s].tobytes(), ref["rnd"][s].tobytes(), ref["prim"])
        alone = b"".join(one.garble(c.Gates, c.NumWires, in_, out_) for c, in_, out_ in ref["steps"])
        one.close()
        assert run.session(s) == alone, "session %d against gc_stream_*" % s
    assert run.untouched()
    check_store(run.sb, ref)
    # the evaluator handle over the S blocks
    se = engine.StreamEvalBatch(ctx, S, run.d_keys, KEYLEN)
    se.set_wires(ref["prim"], engine.DeviceBuffer(ctx, data=initial_labels(ref, S)))
    d_bad = engine.DeviceBuffer(ctx, shape=S, dtype=np.uint32)
    for k in range(len(ref["steps"])):
        block = ref["streams"][S // 2][k]
        assert eval_step(se, ref, k, block, run.d_out + (run.lead + run.offs[k]), run.stride, d_bad) == len(block)
        assert (d_bad.numpy() == 0).all(), k
    for w in ref["touched"]:
        got = se.get(w)
        for s in range(S):
            assert (int(got[s]["d0"]), int(got[s]["d1"])) == ref["ev"][w][s], (w, s)
    se.close(), run.close()
    ctx.close()


def test_a_flipped_skeleton_byte_in_the_hbm_wire_step_is_counted_for_its_session_only():
    S = 3
    ctx = engine.Context(0)
    ref = reference(S)
    run = Run(ctx, ref, S, KEYLEN)
    se = engine.StreamEvalBatch(ctx, S, run.d_keys, KEYLEN)
    se.set_wires(ref["prim"], engine.DeviceBuffer(ctx, data=initial_labels(ref, S)))
    d_bad = engine.DeviceBuffer(ctx, shape=S, dtype=np.uint32)
    assert eval_step(se, ref, 0, ref["streams"][0][0], run.d_out + run.offs[0], run.stride, d_bad) == len(ref["streams"][0][0])
    c, in_, out_ = ref["steps"][1]
    block = ref["streams"][0][1]
    gates, err = hf.parse(block, c.NumGates)
    assert err is None
    n = len(block)
    blocks = run.buf[: S * run.stride].reshape(S, run.stride)[:, run.offs[1]: run.offs[1] + n].copy()
    blocks[1, gates[100][5][0] + 1] ^= 0x04  # a wire id byte of session 1
    stride = (n + 3) & ~3
    padded = np.zeros((S, stride), np.uint8)
    padded[:, :n] = blocks
    d_blocks = engine.DeviceBuffer(ctx, data=padded)
    assert eval_step(se, ref, 1, block, d_blocks, stride, d_bad) == n
    bad = d_bad.numpy()
    assert bad[1] != 0 and bad[0] == 0 and bad[2] == 0, bad
    got = se.get(out_[0])
    for s in (0, 2):
        step_label = oracle_label_after(ref, s, 2, out_[0])
        assert (int(got[s]["d0"]), int(got[s]["d1"])) == step_label, s
    se.close(), run.close()
    ctx.close()


def oracle_label_after(ref, s, nsteps, w):
    """the oracle evaluator's label of wire w in session s after the first nsteps steps"""
    e = oracle.StreamEval(ref["keys"][s].tobytes())
    lab = initial_labels(ref, len(ref["keys"]))
    for j, p in enumerate(ref["prim"]):
        e.set(p, lab[s, j])
    for k in range(nsteps):
        c, in_, out_ = ref["steps"][k]
        e.circuit(c.NumGates, c.NumWires, max(max(in_), max(out_)) + 1, ref["streams"][s][k])
    return e.get(w)
