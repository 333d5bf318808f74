"""gc_batch_garble_keyed / gc_batch_eval_keyed on the level-walking kernels with the wires in HBM (path 2 of
gc_batch_keyed_path: k_garble_hbm_keyed / k_eval_hbm_keyed, mpc_amd/csrc/fused_hbm_keyed_kernels.hip): the batches the
flattened keyed kernels cannot serve — a circuit without a usable LDS plan — and any schedule-1 batch sent there with
set_keyed_path(2).

Every case compares R, slab, output L0s, active outputs and decoded bits per instance with the oracle under that instance's
key; path 2 leaves every wire in the global array, so read_wires (garbler: {L0, L1} of every wire) and read_labels (evaluator:
the active label of every wire) are compared for the same instances.  Large batches are checked in the two layers of
tests/test_gpu_batch_keyed_shapes.py: the oracle on kg.sample(), every instance against three one-key passes under
kg.pool_keys.  Pair(..., shape) asserts the scope of the flattened kernels, so forced cases pass shape=None and assert the
tile width themselves (the tile rule of tests/keyed_geometry.py; an HBM-wire batch is never cut by LDS)."""
import numpy as np
import pytest

import oracle
from mpc_amd import LABEL, engine
from tests import keyed_geometry as kg
from tests.test_gpu_batch_keyed import Pair
from tests.test_gpu_batch_keyed import ctx  # noqa: F401  (the module-scoped fixture)
from tests.util import drbg

pytestmark = pytest.mark.gpu

FIELDS = ("R", "slab", "l0", "active", "bits", "wires", "labels")


def tile_by_batch(batch):
    t = 0
    while t < 6 and (batch >> (t + 1)) >= 256:
        t += 1
    return 1 << t


class HbmPair(Pair):
    """Pair whose results carry every wire of both batches"""

    def force(self):
        for b in (self.gb, self.ev):
            b.set_keyed_path(2)
            assert b.keyed_path == 2 and b.keyed_supported()

    def results(self):
        got = super().results()
        got["wires"], got["labels"] = self.gb.read_wires(), self.ev.read_labels()
        return got

    def reference(self, i, key):
        c = self.c
        ref = oracle.garble(c.Gates, c.NumWires, c.num_inputs, bytes(key), self.rnd[i * self.stride:(i + 1) * self.stride])
        w = np.zeros(c.NumWires, LABEL)
        io = ref["wires"][: c.num_inputs]
        w[: c.num_inputs] = np.where(self.bits[i].astype(bool), io["l1"], io["l0"])
        oracle.eval_(c.Gates, c.NumWires, bytes(key), w, ref["slab"])
        plain = oracle.compute(c.Gates, c.NumWires, c.num_inputs, self.bits[i])
        return {"R": ref["R"], "slab": ref["slab"], "l0": ref["wires"]["l0"][c.NumWires - c.num_outputs:],
                "active": w[c.NumWires - c.num_outputs:], "bits": plain[c.NumWires - c.num_outputs:], "wires": ref["wires"],
                "labels": w}

    def check(self, got, i, key, what=""):
        ref = self.reference(i, key)
        assert got["R"][i] == ref["R"], "%s R of instance %d" % (what, i)
        for f in FIELDS[1:]:
            if f in got:
                assert (got[f][i] == ref[f]).all(), "%s %s of instance %d" % (what, f, i)

    def check_same(self, got, one, idx, what=""):
        idx = np.asarray(idx)
        for f in FIELDS:
            if f not in got or f not in one:
                continue
            eq = got[f][idx] == one[f][idx]
            bad = idx[~eq.reshape(len(idx), -1).all(axis=1)]
            assert not len(bad), "%s %s of instances %s ..." % (what, f, bad[:8].tolist())


def report(name, batch, keylen, p, n_oracle, n_full):
    print("keyed HBM case: %s x %d, %d-byte keys: TI = %d, k_{garble,eval}_hbm_keyed<%d, %s>, %d instances against the oracle, "
          "%d against the one-key passes" % (name, batch, keylen, p.gb.tile_instances, keylen // 4 + 6,
                                             "true" if p.c.stats()["OR"] else "false", n_oracle, n_full))


def layered(p, name, batch, keylen):
    """kg.sample against the oracle, every instance against three one-key passes under kg.pool_keys"""
    tag = "hbm/%s/%d/%d" % (name, batch, keylen)
    pool, keys = kg.pool_keys(tag, batch, keylen)
    p.keyed(p.ctx.to_device(keys), keylen)
    got = p.results()
    smp = kg.sample(batch, p.gb.tile_instances)
    for i in smp:
        p.check(got, i, keys[i], "keyed:")
    for k in range(3):
        p.one_key(pool[k].tobytes())
        one = Pair.results(p)  # (the one-key pass of a batch with its wires in LDS leaves no wire array)
        p.check_same(got, one, np.arange(k, batch, 3), "against the one-key pass %d:" % k)
    report(name, batch, keylen, p, len(smp), batch)


# ---- 1. natural scope: a circuit whose wires are not in LDS -----------------------------------------------------------------

NATURAL = kg.N_FIT + 16  # tests/test_keyed_geometry.py: from N_FIT + 16 inputs on, not even the one-key image of one instance fits


def natural_pair(ctx, batch, tag):
    p = HbmPair(ctx, kg.lds_edge(NATURAL), batch, tag)
    for b in (p.gb, p.ev):  # before any byte is compared
        assert not b.lds_wires and b.keyed_path == 2 and b.keyed_supported()
    assert p.gb.tile_instances == tile_by_batch(batch)
    return p


@pytest.mark.parametrize("keylen", [32, 16])
def test_natural_scope_three_instances(ctx, keylen):
    """lds_edge(N_FIT + 16): 6 120 levels of one gate, headed by an OR, an INV and an AND.  GC_E_ARG before path 2 existed."""
    p = natural_pair(ctx, 3, "hbm/natural/%d" % keylen)
    keys = kg.edge_keys("hbm/natural/%d" % keylen, 3, keylen)
    p.keyed(ctx.to_device(keys), keylen)
    got = p.results()
    for i in range(3):
        p.check(got, i, keys[i])
    report("lds_edge", 3, keylen, p, 3, 0)
    p.close()


def test_natural_scope_1027_instances(ctx):
    """tiles of four by the tile rule (LDS does not cut an HBM-wire batch), the last one ragged"""
    p = natural_pair(ctx, 1027, "hbm/natural/1027")
    assert p.gb.tile_instances == 4
    layered(p, "lds_edge", 1027, 32)
    p.close()


# ---- 2. all twelve instantiations -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("batch", [5, 1027])
@pytest.mark.parametrize("name", ["adder8", "mixed", "wide"])
@pytest.mark.parametrize("keylen", [16, 24, 32])
def test_all_twelve_instantiations_forced(ctx, keylen, name, batch):
    """3 key lengths x (adder8, wide: HAS_OR = false; mixed: HAS_OR = true) x garble / eval, at tiles of one (5) and of four
    with a ragged last tile (1 027).  wide and mixed have 320 gates per level: 20 passes of 1 024 column lanes at TI 4 on the
    garbler, the last one partial for mixed."""
    tag = "hbm/len/%s/%d/%d" % (name, batch, keylen)
    p = HbmPair(ctx, kg.build(name), batch, tag)
    assert p.gb.keyed_path == 1
    p.force()
    assert p.gb.tile_instances == p.ev.tile_instances == kg.predict(name, batch).ti == (1 if batch == 5 else 4)
    keys = kg.edge_keys(tag, batch, keylen)
    p.keyed(ctx.to_device(keys), keylen)
    got = p.results()
    smp = list(range(batch)) if batch == 5 else kg.sample(batch, 4)
    for i in smp:
        p.check(got, i, keys[i])
    report(name, batch, keylen, p, len(smp), 0)
    for b in (p.gb, p.ev):
        b.set_keyed_path(0)
        assert b.keyed_path == 1
    p.close()


# ---- 3. every tile width ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,batch,ti", [("adder8", 515, 2), ("adder8", 2051, 8), ("adder8", 4099, 16), ("adder8", 8195, 32),
                                           ("adder8", 16389, 64), ("mixed_small", 2051, 8), ("mixed_small", 16389, 64)])
def test_every_tile_width_forced(ctx, name, batch, ti):
    p = HbmPair(ctx, kg.build(name), batch, "hbm/ti/%s/%d" % (name, batch))
    p.force()
    assert p.gb.tile_instances == p.ev.tile_instances == ti and batch % ti != 0
    layered(p, name, batch, 24 if name == "mixed_small" else 32)
    p.close()


# ---- 4. key semantics -------------------------------------------------------------------------------------------------------


def test_key_semantics(ctx):
    batch, name = 1027, "mixed"
    p = HbmPair(ctx, kg.build(name), batch, "hbm/sem")
    p.force()
    key0 = drbg("keyed/hbm/sem/key0", 32)
    p.one_key(key0)
    one = Pair.results(p)
    same = np.tile(np.frombuffer(key0, np.uint8), (batch, 1))
    d_keys = ctx.to_device(same)
    p.keyed(d_keys, 32)  # all keys equal: the bytes of the one-key call on the same batch
    got = p.results()
    p.check_same(got, one, np.arange(batch), "equal keys against the one-key pass:")
    keys = kg.edge_keys("hbm/sem", batch, 32)  # zero key, all-ones key, keys that differ in one end byte: instances 0..5
    d_keys.upload(keys)
    p.keyed(d_keys, 32)
    a = p.results()
    for i in range(6):
        p.check(a, i, keys[i], "edge keys:")
    for i in range(batch):
        assert (a["slab"][i] != one["slab"][i]).any(), "instance %d ignores its key" % i
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


# ---- 5. a replayed graph ----------------------------------------------------------------------------------------------------


def test_a_replayed_graph_on_path_2(ctx):
    name, batch, keylen = "mixed", 1027, 16
    p = HbmPair(ctx, kg.build(name), batch, "hbm/graph16")
    p.force()
    p.gb.set_graph(True)
    p.ev.set_graph(True)
    smp = kg.sample(batch, 4)
    keys_a, keys_b = kg.edge_keys("hbm/graph16/a", batch, keylen), kg.edge_keys("hbm/graph16/b", batch, keylen)[::-1].copy()
    d_keys = ctx.to_device(keys_a)
    p.keyed(d_keys, keylen)  # direct
    got = p.results()
    for i in smp:
        p.check(got, i, keys_a[i], "direct:")
    g = ctx.capture(lambda: p.keyed(d_keys, keylen))
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


# ---- 6. the band that stays refused by default ------------------------------------------------------------------------------


def test_key_table_band_runs_forced_and_stays_refused_by_default(ctx):
    shape = kg.predict("edge_over", 3)
    assert shape.wires_in_lds and not shape.keyed
    p = HbmPair(ctx, kg.build("edge_over"), 3, "hbm/over", shape)
    assert p.gb.keyed_path == 0 and p.ev.keyed_path == 0
    p.force()
    assert p.gb.lds_wires and p.gb.tile_instances == 1
    keys = kg.edge_keys("hbm/over", 3, 32)
    d_keys = ctx.to_device(keys)
    p.keyed(d_keys, 32)
    got = p.results()
    for i in range(3):
        p.check(got, i, keys[i])
    for b in (p.gb, p.ev):
        b.set_keyed_path(0)
        assert b.keyed_path == 0 and not b.keyed_supported()
    with pytest.raises(engine.EngineError) as e:
        p.gb.garble_keyed(d_keys, 32, p.d_rnd)
    assert e.value.code == engine.GC_E_ARG
    msg = engine.lib().gc_last_error()
    assert b"gc_batch_garble_keyed" in msg and b"key table" in msg
    with pytest.raises(engine.EngineError) as e:
        p.ev.eval_keyed(d_keys, 32, p.gb)
    assert e.value.code == engine.GC_E_ARG
    msg = engine.lib().gc_last_error()
    assert b"gc_batch_eval_keyed" in msg and b"key table" in msg
    p.close()


# ---- 7. errors --------------------------------------------------------------------------------------------------------------


def test_error_contract_of_the_forced_path(ctx):
    batch = 3
    p = HbmPair(ctx, kg.build("adder8"), batch, "hbm/err")
    keys = kg.edge_keys("hbm/err", batch, 32)
    d_keys = ctx.to_device(keys)
    for bad in (1, 3, -1):
        with pytest.raises(engine.EngineError) as e:
            p.gb.set_keyed_path(bad)
        assert e.value.code == engine.GC_E_ARG
    assert p.gb.keyed_path == 1
    p.force()
    for b in (p.gb, p.ev):  # the forced value survives a change of schedule and answers 0 outside schedule 1
        b.set_schedule(0)
        assert b.keyed_path == 0 and not b.keyed_supported()
        with pytest.raises(engine.EngineError) as e:
            b.set_keyed_path(2)
        assert e.value.code == engine.GC_E_ARG
    with pytest.raises(engine.EngineError) as e:
        p.gb.garble_keyed(d_keys, 32, p.d_rnd)
    assert e.value.code == engine.GC_E_ARG and b"gc_batch_garble_keyed" in engine.lib().gc_last_error()
    with pytest.raises(engine.EngineError) as e:
        p.ev.eval_keyed(d_keys, 32, p.gb)
    assert e.value.code == engine.GC_E_ARG and b"gc_batch_eval_keyed" in engine.lib().gc_last_error()
    key = drbg("keyed/hbm/err/key", 32)
    p.one_key(key)  # ... and the batch still serves the one-key calls
    got = Pair.results(p)
    for i in range(batch):
        Pair.check(p, got, i, key)
    for b in (p.gb, p.ev):
        b.set_schedule(1)
        assert b.keyed_path == 2
    p.keyed(d_keys, 32)
    got = p.results()
    for i in range(batch):
        p.check(got, i, keys[i])
    p.close()
