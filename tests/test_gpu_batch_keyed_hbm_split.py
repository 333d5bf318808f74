"""The split form of the keyed HBM-wire kernels (path 2 of gc_batch_keyed_path under gc_batch_set_keyed_hbm_form:
k_garble_hbm_keyed_split / k_eval_hbm_keyed_split, mpc_amd/csrc/fused_hbm_keyed_split_kernels.hip): on a level wider than
1 024 column lanes the first H waves of the workgroup hash and the others stream the free gates.

Every case compares R, slab, output L0s, active outputs, decoded bits and every wire of both batches with the oracle under the
instance's key, and form 2 with form 1 on the same batch, byte for byte in every instance."""
import numpy as np
import pytest

from mpc_amd import circuit, engine
from tests import keyed_geometry as kg
from tests import keyed_split_cases as sc
from tests.test_gpu_batch_keyed import Pair
from tests.test_gpu_batch_keyed import ctx  # noqa: F401  (the module-scoped fixture)
from tests.test_gpu_batch_keyed_hbm import NATURAL, HbmPair, layered
from tests.util import drbg

pytestmark = pytest.mark.gpu


def set_form(p, form, want):
    for b in (p.gb, p.ev):
        b.set_keyed_hbm_form(form)
        assert b.keyed_path == 2 and b.keyed_hbm_form == want


def forced_pair(ctx, c, batch, tag, ti):
    p = HbmPair(ctx, c, batch, tag)
    p.force()
    assert p.gb.tile_instances == p.ev.tile_instances == ti
    return p


def both_forms(p, d_keys, keylen, keys, smp, what=""):
    """form 2 against the oracle on smp, then form 1 on the same batch: every instance, every field, byte for byte"""
    set_form(p, 2, 2)
    p.keyed(d_keys, keylen)
    assert p.gb.last_launches == 1 and p.ev.last_launches == 1
    split = p.results()
    for i in smp:
        p.check(split, i, keys[i], what + " split form:")
    set_form(p, 1, 1)
    p.keyed(d_keys, keylen)
    plain = p.results()
    p.check_same(split, plain, np.arange(p.batch), what + " split against plain:")
    return split


# ---- 1. all twelve instantiations ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("batch", [5, 1027])
@pytest.mark.parametrize("name", ["adder8", "mixed", "wide"])
@pytest.mark.parametrize("keylen", [16, 24, 32])
def test_all_twelve_instantiations(ctx, keylen, name, batch):
    """mixed: 320 gates a level of every kind, both roles busy; wide: no free gate, H = 16; adder8: never wide, the single-pass
    branch throughout"""
    tag = "split/len/%s/%d/%d" % (name, batch, keylen)
    p = forced_pair(ctx, kg.build(name), batch, tag, 1 if batch == 5 else 4)
    keys = kg.edge_keys(tag, batch, keylen)
    both_forms(p, ctx.to_device(keys), keylen, keys, list(range(batch)) if batch == 5 else kg.sample(batch, 4))
    p.close()


# ---- 2. the shapes where the split can go wrong -----------------------------------------------------------------------------


@pytest.mark.parametrize("batch,ti", [(5, 1), (1027, 4)])
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_split_edges(ctx, name, batch, ti):
    tag = "split/edge/%s/%d" % (name, batch)
    p = forced_pair(ctx, sc.build(name, ti), batch, tag, ti)
    keys = kg.edge_keys(tag, batch, 24)
    both_forms(p, ctx.to_device(keys), 24, keys, list(range(batch)) if batch == 5 else kg.sample(batch, ti)[:24])
    p.close()


# ---- 3. wide tiles ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,batch,ti,keylen", [("mixed_small", 16389, 64, 24), ("adder8", 2051, 8, 32)])
def test_wide_tiles(ctx, name, batch, ti, keylen):
    p = forced_pair(ctx, kg.build(name), batch, "split/ti/%s/%d" % (name, batch), ti)
    assert batch % ti != 0
    set_form(p, 2, 2)
    layered(p, name, batch, keylen)  # the oracle on kg.sample, every instance against three one-key passes
    _, keys = kg.pool_keys("split/ti/%s/%d" % (name, batch), batch, keylen)
    d_keys = ctx.to_device(keys)
    p.keyed(d_keys, keylen)
    split = p.results()
    set_form(p, 1, 1)
    p.keyed(d_keys, keylen)
    p.check_same(split, p.results(), np.arange(batch), "split against plain:")
    p.close()


# ---- 4. fixed hash waves ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("h", [1, 8, 15])
def test_fixed_hash_waves(ctx, h):
    batch, keylen, tag = 1027, 16, "split/h/%d" % h
    p = forced_pair(ctx, kg.build("mixed"), batch, tag, 4)
    for b in (p.gb, p.ev):
        b.debug_keyed_hbm_hash_waves(h, h)
    keys = kg.edge_keys(tag, batch, keylen)
    both_forms(p, ctx.to_device(keys), keylen, keys, kg.sample(batch, 4)[:24], "H = %d" % h)
    for b in (p.gb, p.ev):
        with pytest.raises(engine.EngineError) as e:
            b.debug_keyed_hbm_hash_waves(16, 0)
        assert e.value.code == engine.GC_E_ARG
        b.debug_keyed_hbm_hash_waves(0, 0)
    p.close()


# ---- 5. the rule ------------------------------------------------------------------------------------------------------------


def test_the_rule(ctx):
    p = HbmPair(ctx, kg.lds_edge(NATURAL), 3, "split/rule/natural")
    for b in (p.gb, p.ev):  # natural path 2, one gate per level: the plain form
        assert not b.lds_wires and b.keyed_path == 2 and b.keyed_hbm_form == 1
    p.close()
    batch, keylen = 5, 32
    p = HbmPair(ctx, kg.build("mixed"), batch, "split/rule/mixed")
    for b in (p.gb, p.ev):  # a path-1 batch
        assert b.keyed_path == 1 and b.keyed_hbm_form == 0
        b.set_keyed_hbm_form(2)
        assert b.keyed_hbm_form == 0
        b.set_keyed_hbm_form(0)
    p.force()
    for b in (p.gb, p.ev):
        assert b.keyed_hbm_form == 2
        b.set_keyed_hbm_form(1)
        assert b.keyed_hbm_form == 1
        b.set_keyed_hbm_form(0)
        assert b.keyed_hbm_form == 2
        for bad in (3, -1, 7):
            with pytest.raises(engine.EngineError) as e:
                b.set_keyed_hbm_form(bad)
            assert e.value.code == engine.GC_E_ARG
        assert b.keyed_hbm_form == 2
    keys = kg.edge_keys("split/rule/mixed", batch, keylen)
    d_keys = ctx.to_device(keys)
    p.keyed(d_keys, keylen)  # under the rule
    got = p.results()
    for i in range(batch):
        p.check(got, i, keys[i], "the rule:")
    set_form(p, 1, 1)
    p.keyed(d_keys, keylen)
    p.check_same(got, p.results(), np.arange(batch), "the rule against plain:")
    for b in (p.gb, p.ev):
        b.set_keyed_path(0)
        assert b.keyed_path == 1 and b.keyed_hbm_form == 0
    p.close()


# ---- 6. key semantics -------------------------------------------------------------------------------------------------------


def test_key_semantics_under_the_split_form(ctx):
    batch, name = 1027, "mixed"
    p = forced_pair(ctx, kg.build(name), batch, "split/sem", 4)
    set_form(p, 2, 2)
    key0 = drbg("keyed/split/sem/key0", 32)
    p.one_key(key0)
    one = Pair.results(p)
    d_keys = ctx.to_device(np.tile(np.frombuffer(key0, np.uint8), (batch, 1)))
    p.keyed(d_keys, 32)  # all keys equal: the bytes of the one-key call on the same batch
    p.check_same(p.results(), one, np.arange(batch), "equal keys against the one-key pass:")
    keys = kg.edge_keys("split/sem", batch, 32)
    d_keys.upload(keys)
    p.keyed(d_keys, 32)
    a = p.results()
    for i in range(6):
        p.check(a, i, keys[i], "edge keys:")
    for i, j in ((513, 514), (2, 1026)):  # the same tile; different tiles
        swapped = keys.copy()
        swapped[[i, j]] = keys[[j, i]]
        d_keys.upload(swapped)
        p.keyed(d_keys, 32)
        b = p.results()
        others = np.array([k for k in range(batch) if k not in (i, j)])
        p.check_same(b, a, others, "after the swap:")
        assert (a["slab"][i] != b["slab"][i]).any() and (a["slab"][j] != b["slab"][j]).any()
        for k in (i, j):
            p.check(b, k, swapped[k], "after the swap:")
    p.close()


# ---- 7. a replayed graph ----------------------------------------------------------------------------------------------------


def test_a_replayed_graph_under_the_split_form(ctx):
    name, batch, keylen = "mixed", 1027, 16
    p = forced_pair(ctx, kg.build(name), batch, "split/graph", 4)
    set_form(p, 2, 2)
    p.gb.set_graph(True)
    p.ev.set_graph(True)
    smp = kg.sample(batch, 4)[:24]
    keys_a, keys_b = kg.edge_keys("split/graph/a", batch, keylen), kg.edge_keys("split/graph/b", batch, keylen)[::-1].copy()
    d_keys = ctx.to_device(keys_a)
    p.keyed(d_keys, keylen)  # direct
    got = p.results()
    g = ctx.capture(lambda: p.keyed(d_keys, keylen))
    set_form(p, 1, 1)  # a graph captured before stays valid for what it captured
    for keys in (keys_b, keys_a):
        d_keys.upload(keys)
        g.launch()
        again = p.results()
        for i in smp:
            p.check(again, i, keys[i], "replay:")
        if keys is keys_a:
            p.check_same(again, got, np.arange(batch), "replay against the direct pass:")
    g.close()
    p.close()


# ---- 8. one wide step of a batched stream -----------------------------------------------------------------------------------


def wide_hbm_circuit():
    """kg.lds_edge(NATURAL) — no LDS plan fits its live set — behind one level of 300 ANDs and 900 XORs over its inputs"""
    n = NATURAL
    b = kg._Gates(n)
    front = [b.gate(i, i + 300, circuit.AND) for i in range(300)] + [b.gate(i, i + 901, circuit.XOR) for i in range(900)]
    acc = b.gate(front[0], front[300], circuit.OR)
    acc = b.gate(acc, front[1], circuit.INV)
    for i in range(n):
        acc = b.gate(acc, i, circuit.AND)
    for w in front[2:300]:
        acc = b.gate(acc, w, circuit.XOR)
    return b.circuit(n, 1, "wide_hbm")


def test_a_wide_step_of_a_batched_stream_takes_the_split_form():
    import oracle
    from mpc_amd.circuit import WIRE
    from tests.test_gpu_stream_batch import Run, active_labels, eval_step, rnd_streams
    S, keylen = 5, 32
    ctx = engine.Context(0)
    c = wide_hbm_circuit()
    dc = engine.DeviceCircuit(ctx, c)
    b = engine.Batch(dc, S)
    assert not b.lds_wires and b.keyed_path == 2 and b.keyed_hbm_form == 2 and b.tile_instances == 1
    b.close(), dc.close()
    prim = list(range(16))
    steps = [(c, [i % 16 for i in range(c.num_inputs)], [40])]
    keys = kg.edge_keys("stream-batch/split", S, keylen)
    rnd = rnd_streams("split/%d" % S, S, len(prim))
    bits = np.random.default_rng(S).integers(0, 2, (S, len(prim)), dtype=np.uint8)
    streams, wires, ev = [], {w: np.zeros(S, WIRE) for w in prim + [40]}, []
    for s in range(S):
        g = oracle.Stream(keys[s].tobytes(), rnd[s].tobytes(), prim)
        e = oracle.StreamEval(keys[s].tobytes())
        for w, bit in zip(prim, bits[s]):
            wire = g.get(w)
            e.set(w, wire["l1"] if bit else wire["l0"])
        data = g.garble(c.Gates, c.NumWires, steps[0][1], steps[0][2])
        assert e.circuit(c.NumGates, c.NumWires, 41, data) == len(data)
        streams.append([data])
        for w in wires:
            wires[w][s] = g.get(w)
        ev.append(e.get(40))
    ref = dict(steps=steps, prim=prim, keys=keys, rnd=rnd, streams=streams, wires=wires, bits=bits)
    run = Run(ctx, ref, S, keylen, lead=3)
    for s in range(S):
        assert run.session(s) == streams[s][0], "session %d against the oracle" % s
        one = engine.Stream(ctx, keys[s].tobytes(), rnd[s].tobytes(), prim)
        alone = one.garble(c.Gates, c.NumWires, steps[0][1], steps[0][2])
        one.close()
        assert run.session(s) == alone, "session %d against gc_stream_*" % s
    assert run.untouched()
    se = engine.StreamEvalBatch(ctx, S, run.d_keys, keylen)
    se.set_wires(prim, engine.DeviceBuffer(ctx, data=active_labels(ref, S)))
    d_bad = engine.DeviceBuffer(ctx, shape=S, dtype=np.uint32)
    assert eval_step(se, ref, 0, streams[2][0], run.d_out + run.lead, run.stride, d_bad) == len(streams[2][0])
    assert (d_bad.numpy() == 0).all()
    got = se.get(40)
    for s in range(S):
        assert (int(got[s]["d0"]), int(got[s]["d1"])) == ev[s], s
    se.close(), run.close()
    ctx.close()
