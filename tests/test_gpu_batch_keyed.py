"""gc_batch_garble_keyed / gc_batch_eval_keyed: one AES key per instance of a device-resident batch (circuit.Garbler draws
a fresh key per session, garbler.go:47-53, and sends it to the peer, :64).  The expected bytes of instance i are the oracle's
for key i and instance i's slice of the random stream: R, the slab in reference order, the output labels, the decoded bits.

Batches of 1, 3, 5 and 8 instances get tiles of ONE instance from the planner (it widens tiles only from 512 instances on), so
the parity cases add 1 027 instances: tiles of four with three instances in the last one — neighbouring lanes then hold
different keys, and the last tile has an instance past the batch (zero keys, never read from the caller's buffer)."""
import numpy as np
import pytest

import oracle
from mpc_amd import LABEL, circuit, engine
from tests import keyed_geometry as kg
from tests.util import bits_lsb, drbg, int_from_bits

pytestmark = pytest.mark.gpu


def stream(tag, n):
    """n seeded bytes: the SHA-256 counter stream, past 1 MiB numpy's generator (a hash call per 32 bytes takes seconds there)"""
    if n <= 1 << 20:
        return drbg(tag, n)
    return np.random.default_rng(int.from_bytes(drbg(tag, 8), "big")).bytes(n)


def distinct_keys(tag, batch, keylen):
    keys = np.frombuffer(drbg("keyed/" + tag, batch * keylen), np.uint8).reshape(batch, keylen).copy()
    assert len({k.tobytes() for k in keys}) == batch
    return keys


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


class Pair:
    """a garbler and an evaluator batch of one circuit with their device buffers"""

    def __init__(self, ctx, c, batch, tag, shape=None):
        """shape: the kg.Shape predicted for (c, batch); both batches must have got it"""
        self.ctx, self.c, self.batch = ctx, c, batch
        self.dc = engine.DeviceCircuit(ctx, c)
        self.gb, self.ev = engine.Batch(self.dc, batch), engine.Batch(self.dc, batch)
        if shape is not None:
            assert (int(self.dc.info.n_flat_slots),) + self.dc.flat_geometry() == (shape.nls, shape.ustride, shape.parts)
            kg.check_batch(self.gb, shape)
            kg.check_batch(self.ev, shape)
        self.stride = 16 * (c.num_inputs + 1)
        self.rnd = stream("keyed/rnd/" + tag, self.stride * batch)
        self.bits = (np.frombuffer(stream("keyed/bits/" + tag, batch * c.num_inputs), np.uint8) & 1).reshape(batch, -1)
        self.d_rnd, self.d_bits = ctx.to_device(self.rnd), ctx.to_device(self.bits)
        self.d_out, self.d_mis = ctx.zeros((batch, c.num_outputs)), ctx.zeros(1, np.int32)

    def rest(self, eval_call):
        self.ev.select_inputs(self.gb, self.d_bits)
        eval_call()
        self.gb.decode(self.ev, self.d_out, self.d_mis)

    def keyed(self, d_keys, keylen):
        self.gb.garble_keyed(d_keys, keylen, self.d_rnd)
        self.rest(lambda: self.ev.eval_keyed(d_keys, keylen, self.gb))

    def one_key(self, key):
        self.gb.garble(key, self.d_rnd)
        self.rest(lambda: self.ev.eval(key, self.gb))

    def results(self):
        self.ctx.sync()
        assert int(self.d_mis.numpy()[0]) == 0
        self.d_mis.zero()
        return {"R": self.gb.read_r(), "slab": self.gb.read_slab(), "l0": self.gb.read_outputs(),
                "active": self.ev.read_outputs(), "bits": self.d_out.numpy().copy()}

    def reference(self, i, key):
        """the oracle's run of instance i under `key`"""
        c = self.c
        ref = oracle.garble(c.Gates, c.NumWires, c.num_inputs, bytes(key), self.rnd[i * self.stride:(i + 1) * self.stride])
        w = np.zeros(c.NumWires, LABEL)
        io = ref["wires"][: c.num_inputs]
        w[: c.num_inputs] = np.where(self.bits[i].astype(bool), io["l1"], io["l0"])
        oracle.eval_(c.Gates, c.NumWires, bytes(key), w, ref["slab"])
        plain = oracle.compute(c.Gates, c.NumWires, c.num_inputs, self.bits[i])
        return {"R": ref["R"], "slab": ref["slab"], "l0": ref["wires"]["l0"][c.NumWires - c.num_outputs:],
                "active": w[c.NumWires - c.num_outputs:], "bits": plain[c.NumWires - c.num_outputs:]}

    def check(self, got, i, key, what=""):
        ref = self.reference(i, key)
        assert got["R"][i] == ref["R"], "%s R of instance %d" % (what, i)
        for f in ("slab", "l0", "active", "bits"):
            assert (got[f][i] == ref[f]).all(), "%s %s of instance %d" % (what, f, i)

    def check_same(self, got, one, idx, what=""):
        """instances idx of `got` equal those of `one` (the results of another pass) in all five fields"""
        idx = np.asarray(idx)
        for f in ("R", "slab", "l0", "active", "bits"):
            eq = got[f][idx] == one[f][idx]
            bad = idx[~eq.reshape(len(idx), -1).all(axis=1)]
            assert not len(bad), "%s %s of instances %s ..." % (what, f, bad[:8].tolist())

    def close(self):
        self.gb.close()
        self.ev.close()
        self.dc.close()


# ---- 1. key schedule ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("keylen", [16, 24, 32])
def test_key_schedule_on_the_device_equals_the_hosts(ctx, keylen):
    """k_expand_keys against aes_host.h's schedule (and the oracle's, an implementation of its own), word for word, in the
    form the kernels hash with: big-endian words, the last round key XORed with round key 0.  One lane is one instance and a
    block 256 lanes: 5 is a partly filled block, 256 a full one, 257 and 1 027 go past it (the `gi >= batch` guard in a
    second and a fifth block).  Keys with the edge patterns of kg.edge_keys."""
    nr = keylen // 4 + 6
    for batch in (5, 256, 257, 1027):
        p = Pair(ctx, circuit.adder(8), batch, "sched")
        keys = distinct_keys("sched%d" % keylen, batch, keylen) if batch == 5 else kg.edge_keys("sched%d" % keylen, batch, keylen)
        dev, host = p.gb.debug_keyed_schedule(ctx.to_device(keys), keylen)
        assert dev.shape == (batch, 4 * (nr + 1))
        assert (dev == host).all()
        for i in range(batch):
            rk, rounds = oracle.aes_round_keys(keys[i].tobytes())
            w = np.frombuffer(rk, ">u4").astype(np.uint32)
            assert rounds == nr and len(w) == 4 * (nr + 1)
            w[4 * nr:] ^= w[:4]
            assert (dev[i] == w).all(), "%d instances: instance %d" % (batch, i)
        p.close()


# ---- 2. parity with the oracle -------------------------------------------------------------------------------------------

# adder8: narrow units only; wide: 320 ANDs per level, several passes of 1 024 column lanes per unit; mixed: every gate kind,
# the HAS_OR build, odd gate counts leave the last pass of a unit partial (tests/keyed_geometry.py, whose host test pins the
# tile width each batch gets)
CIRCUITS = {name: kg.CIRCUITS[name] for name in ("adder8", "wide", "mixed")}


@pytest.mark.parametrize("batch", [1, 3, 5, 8, 1027])
@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_every_instance_equals_the_oracle_under_its_own_key(ctx, name, batch):
    c = CIRCUITS[name]()
    if name == "mixed":
        s = c.stats()
        assert s["OR"] and s["INV"] and s["XNOR"] and s["AND"]
    p = Pair(ctx, c, batch, "%s/%d" % (name, batch), kg.predict(name, batch))
    assert p.gb.keyed_supported() and p.ev.keyed_supported()
    ti = p.gb.tile_instances
    print("%s x %d: TI = %d" % (name, batch, ti))
    if batch == 1027:  # neighbouring lanes hold different keys, and the last tile is ragged
        assert ti >= 2 and batch % ti != 0
    keys = distinct_keys("%s/%d" % (name, batch), batch, 32)
    p.keyed(ctx.to_device(keys), 32)
    got = p.results()
    for i in range(batch):
        p.check(got, i, keys[i])
    p.close()


# ---- 3. keys really per instance ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("batch", [8, 1027])
def test_keys_are_per_instance(ctx, batch):
    c = CIRCUITS["wide"]()
    p = Pair(ctx, c, batch, "per/%d" % batch)
    key0 = drbg("keyed/per/key0", 32)
    p.one_key(key0)
    one = p.results()
    # all keys equal: the bytes of the one-key calls
    same = np.tile(np.frombuffer(key0, np.uint8), (batch, 1))
    d_keys = ctx.to_device(same)
    p.keyed(d_keys, 32)
    got = p.results()
    for f in one:
        assert (got[f] == one[f]).all(), f
    # distinct keys (instance 0 keeps key0): every other instance's slab differs from its one-key slab
    keys = distinct_keys("per/%d" % batch, batch, 32)
    keys[0] = same[0]
    d_keys.upload(keys)
    p.keyed(d_keys, 32)
    a = p.results()
    assert (a["slab"][0] == one["slab"][0]).all()
    for i in range(1, batch):
        assert (a["slab"][i] != one["slab"][i]).any(), "instance %d ignores its key" % i
    # swapping two instances' keys (same tile / different tiles) changes exactly those two instances
    i, j = (2, 5) if batch == 8 else (513, 514)
    swapped = keys.copy()
    swapped[[i, j]] = keys[[j, i]]
    d_keys.upload(swapped)
    p.keyed(d_keys, 32)
    b = p.results()
    others = [k for k in range(batch) if k not in (i, j)]
    for f in a:
        assert (a[f][others] == b[f][others]).all(), f
    assert (a["slab"][i] != b["slab"][i]).any() and (a["slab"][j] != b["slab"][j]).any()
    for k in (i, j):
        p.check(b, k, swapped[k], "after the swap:")
    p.close()


# ---- 4. graph replay reads the buffer -----------------------------------------------------------------------------------


def test_a_replayed_graph_hashes_with_the_keys_the_buffer_holds_then(ctx):
    c = CIRCUITS["mixed"]()
    batch = 5
    p = Pair(ctx, c, batch, "graph")
    p.gb.set_graph(True)
    p.ev.set_graph(True)
    keys_a, keys_b = distinct_keys("graph/a", batch, 32), distinct_keys("graph/b", batch, 32)
    d_keys = ctx.to_device(keys_a)
    p.keyed(d_keys, 32)  # direct
    got = p.results()
    for i in range(batch):
        p.check(got, i, keys_a[i], "direct:")
    g = ctx.capture(lambda: p.keyed(d_keys, 32))  # recorded once ...
    for keys in (keys_b, keys_a):  # ... replayed with other contents in the same buffer
        d_keys.upload(keys)
        g.launch()
        got = p.results()
        for i in range(batch):
            p.check(got, i, keys[i], "replay:")
    g.close()
    p.close()


# ---- 5. errors ---------------------------------------------------------------------------------------------------------


def test_error_contract(ctx):
    c = circuit.adder(8)
    batch = 3
    p = Pair(ctx, c, batch, "err")
    keys = distinct_keys("err", batch, 32)
    d_keys = ctx.to_device(keys)
    with pytest.raises(engine.EngineError) as e:
        p.gb.garble_keyed(d_keys, 20, p.d_rnd)
    assert e.value.code == engine.GC_E_KEYSIZE
    with pytest.raises(engine.EngineError) as e:
        p.ev.eval_keyed(d_keys, 20, p.gb)
    assert e.value.code == engine.GC_E_KEYSIZE
    with pytest.raises(engine.EngineError) as e:
        p.gb.garble_keyed(None, 32, p.d_rnd)
    assert e.value.code == engine.GC_E_ARG
    with pytest.raises(engine.EngineError) as e:
        p.gb.garble_keyed(d_keys, 32, None)
    assert e.value.code == engine.GC_E_ARG
    with pytest.raises(engine.EngineError) as e:
        p.ev.eval_keyed(None, 32, p.gb)
    assert e.value.code == engine.GC_E_ARG
    # outside the scope: schedule 0
    for b in (p.gb, p.ev):
        b.set_schedule(0)
        assert not b.keyed_supported()
    with pytest.raises(engine.EngineError) as e:
        p.gb.garble_keyed(d_keys, 32, p.d_rnd)
    assert e.value.code == engine.GC_E_ARG
    assert b"gc_batch_garble_keyed" in engine.lib().gc_last_error()
    with pytest.raises(engine.EngineError) as e:
        p.ev.eval_keyed(d_keys, 32, p.gb)
    assert e.value.code == engine.GC_E_ARG
    assert b"gc_batch_eval_keyed" in engine.lib().gc_last_error()
    # ... and the batch still serves the one-key calls
    key = drbg("keyed/err/key", 32)
    p.one_key(key)
    got = p.results()
    for i in range(batch):
        p.check(got, i, key)
    # back inside the scope it serves the keyed ones
    for b in (p.gb, p.ev):
        b.set_schedule(1)
        assert b.keyed_supported()
    p.keyed(d_keys, 32)
    got = p.results()
    for i in range(batch):
        p.check(got, i, keys[i])
    p.close()


# ---- 6. one real shape --------------------------------------------------------------------------------------------------


def test_aes128_x8_with_32_byte_keys(ctx, aes_circ):
    c = aes_circ
    batch = 8
    p = Pair(ctx, c, batch, "aes")
    aes_keys = [drbg("keyed/aes/k%d" % i, 16) for i in range(batch)]
    pts = [drbg("keyed/aes/p%d" % i, 16) for i in range(batch)]
    for i in range(batch):
        p.bits[i, :128] = bits_lsb(int.from_bytes(aes_keys[i], "big"), 128)
        p.bits[i, 128:] = bits_lsb(int.from_bytes(pts[i], "big"), 128)
    p.d_bits.upload(p.bits)
    assert p.gb.keyed_supported()
    keys = distinct_keys("aes", batch, 32)
    p.keyed(ctx.to_device(keys), 32)
    got = p.results()
    for i in range(batch):
        assert int_from_bits(got["bits"][i]).to_bytes(16, "big") == oracle.aes_encrypt(aes_keys[i], pts[i]), "instance %d" % i
    for i in (0, 7):
        p.check(got, i, keys[i])
    p.close()
