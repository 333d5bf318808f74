"""gc_batch_garble_keyed / gc_batch_eval_keyed over everything the code can be asked to do: the three key lengths (NR = 10, 12,
14) with and without OR gates, every tile width from 1 to 64, XOR lists in two and four parts, and a key table that ends at
the last byte of LDS.  Byte equality with the oracle throughout; the circuits, the keys and the predicted shape of every case
come from tests/keyed_geometry.py, whose host test (tests/test_keyed_geometry.py) pins each case to its code path.  Every
case first asserts that the device batch got the predicted tile width, wire placement and keyed scope.

Large batches are checked in two layers that leave no instance out:
  * the oracle, every byte, on kg.sample(): tile 0, the last two tiles (the last one ragged: it has instances past the
    batch), every 37th instance in between;
  * every instance against the one-key kernels: key i = pool[i % 3] (3 is coprime to every tile width, so lane neighbours
    differ), three one-key passes over the same random stream, and instance i of the keyed pass equals instance i of the
    pass under pool[i % 3] in R, slab, output zero-labels, active labels and decoded bits.  (test_large_tiles compares the
    one-key kernels with the oracle at these widths.)
Each case prints the tile width, the kernel instantiation and how many instances went to the oracle."""
import numpy as np
import pytest

from mpc_amd import engine
from tests import keyed_geometry as kg
from tests.test_gpu_batch_keyed import Pair
from tests.test_gpu_batch_keyed import ctx  # noqa: F401  (the module-scoped fixture)
from tests.util import drbg

pytestmark = pytest.mark.gpu


def instantiation(c, keylen):
    return "k_{garble,eval}_flat_keyed<%d, %s>" % (keylen // 4 + 6, "true" if c.stats()["OR"] else "false")


def report(name, batch, keylen, p, n_oracle, n_full):
    print("keyed case: %s x %d, %d-byte keys: TI = %d, %s, %d instances against the oracle, %d against the one-key passes"
          % (name, batch, keylen, p.gb.tile_instances, instantiation(p.c, keylen), n_oracle, n_full))


def layered(ctx, name, batch, keylen, one_key_oracle=False):
    """the two layers of the module docstring; one_key_oracle: the first one-key pass goes to the oracle on the sample too"""
    tag = "%s/%d/%d" % (name, batch, keylen)
    shape = kg.predict(name, batch)
    assert shape.keyed and (shape.ti == 1 or batch % shape.ti != 0)
    p = Pair(ctx, kg.build(name), batch, tag, shape)
    pool, keys = kg.pool_keys(tag, batch, keylen)
    p.keyed(ctx.to_device(keys), keylen)
    got = p.results()
    smp = kg.sample(batch, shape.ti)
    for i in smp:
        p.check(got, i, keys[i], "keyed:")
    for k in range(3):
        p.one_key(pool[k].tobytes())
        one = p.results()
        if one_key_oracle and k == 0:
            for i in smp:
                p.check(one, i, pool[0], "one key:")
        p.check_same(got, one, np.arange(k, batch, 3), "against the one-key pass %d:" % k)
    report(name, batch, keylen, p, len(smp), batch)
    p.close()


# ---- B. every key length ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("batch", [5, 1027])
@pytest.mark.parametrize("name", ["adder8", "mixed", "wide"])
@pytest.mark.parametrize("keylen", [16, 24, 32])
def test_every_key_length_every_instance_against_the_oracle(ctx, keylen, name, batch):
    """3 key lengths x (adder8, wide: HAS_OR = false; mixed: HAS_OR = true) x garble / eval = the twelve instantiations, at tiles
    of one instance (batch 5) and of four with three instances in the last one (1 027).  NR fixes the stride of the LDS key
    table, the length of the AES chain and the size of the prologue copy: with keys that are all zero (instance 0), all 0xFF
    (1), equal but for the last byte (2, 3) and but for the first (4, 5), a stride or a length that is wrong for NR = 10 or 12
    changes an instance's bytes.  Every instance goes to the oracle."""
    tag = "len/%s/%d/%d" % (name, batch, keylen)
    p = Pair(ctx, kg.build(name), batch, tag, kg.predict(name, batch))
    keys = kg.edge_keys(tag, batch, keylen)
    p.keyed(ctx.to_device(keys), keylen)
    got = p.results()
    for i in range(batch):
        p.check(got, i, keys[i])
    report(name, batch, keylen, p, batch, 0)
    p.close()


# ---- C. every tile width ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("keylen", [32, 16])
@pytest.mark.parametrize("batch", [515, 2051, 4099, 8195, 16389])
def test_every_tile_width(ctx, batch, keylen):
    """adder8 (one-part lists, 25 live labels: neither the part cap nor LDS cuts the tile) at tiles of 2, 8, 16, 32 and 64
    instances, every batch ragged.  Oracle-checked instances: 22, 74, 145, 287, 573 (tests/test_keyed_geometry.py counts the
    last); all instances against the one-key passes."""
    layered(ctx, "adder8", batch, keylen)


@pytest.mark.parametrize("batch", [2051, 16389])
def test_tile_widths_8_and_64_with_every_gate_kind(ctx, batch):
    """AND, OR, INV, XOR and XNOR gates (the HAS_OR build) at tiles of 8 and 64, 24-byte keys; 74 and 573 instances to the
    oracle, all against the one-key passes"""
    layered(ctx, "mixed_small", batch, 24)


def test_a_replayed_graph_at_tiles_of_four_with_16_byte_keys(ctx):
    """test_a_replayed_graph_hashes_with_the_keys_the_buffer_holds_then at 1 027 instances (TI = 4) and NR = 10: the replay
    expands and hashes with what the key buffer holds then.  40 instances to the oracle per pass."""
    name, batch, keylen = "mixed", 1027, 16
    shape = kg.predict(name, batch)
    p = Pair(ctx, kg.build(name), batch, "graph16", shape)
    p.gb.set_graph(True)
    p.ev.set_graph(True)
    smp = kg.sample(batch, shape.ti)
    keys_a, keys_b = kg.edge_keys("graph16/a", batch, keylen), kg.edge_keys("graph16/b", batch, keylen)[::-1].copy()
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
        if keys is keys_a:  # the same keys as the direct pass: the same bytes in every instance
            p.check_same(again, got, np.arange(batch), "replay against the direct pass:")
    report(name, batch, keylen, p, len(smp), batch)
    g.close()
    p.close()


# ---- D. XOR lists in parts -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,batch,keylen", [("parity2", 300, 32), ("parity2", 4099, 32), ("parity2", 4099, 16),
                                               ("parity4", 300, 32), ("parity4", 4099, 32), ("parity4", 4099, 16)])
def test_xor_lists_in_parts(ctx, name, batch, keylen):
    """XOR lists of 9..16 terms (parity2: two parts) and 17..32 terms (parity4: four parts) between hash phases, some of them
    circuit outputs (kXoStore), some with an odd number of XNORs (kXoRpar), beside lists of one part.  The parts of a list sit
    TI lanes apart and are joined with DPP row shifts: at 300 instances TI = 1; at 4 099 the planner's caps give TI = 8 for two
    parts (the join_parts<8> branch) and TI = 4 for four.  parity4 has 116 four-part lists in one round: more than a unit
    holds, so a unit breaks between two of them.  (The planner sorts the lists of a round longest first, so a leader's index
    is a multiple of its part count without padding: the padded dummies of build_flat do not occur in the early schedule and
    no circuit can ask for them.)  16 / 123 (TI 4) / 129 (TI 8) instances to the oracle, for the keyed pass AND for the
    one-key pass under pool[0]: the one-key kernels' 2- and 4-part joins on the device; all instances of the keyed pass
    against the three one-key passes."""
    assert kg.predict(name, batch).parts == (2 if name == "parity2" else 4)
    layered(ctx, name, batch, keylen, one_key_oracle=True)


# ---- E. the end of LDS -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("keylen", [32, 16])
def test_key_table_that_ends_at_the_last_byte_of_lds(ctx, keylen):
    """lds_edge(N_FIT): the keyed image of a tile is exactly 160 KiB, so with 32-byte keys the last round key of the tile's
    instance is the last 16 bytes of the allocation; with 16-byte keys the table is shorter inside the same image.  An LDS
    read past the allocation returns zeros and a write there is dropped: either shows as wrong bytes here."""
    shape = kg.predict("edge_fit", 3)
    assert shape.keyed_lds == kg.LDS_LIMIT and shape.ti == 1
    p = Pair(ctx, kg.build("edge_fit"), 3, "edge/%d" % keylen, shape)
    keys = kg.edge_keys("edge/%d" % keylen, 3, keylen)
    p.keyed(ctx.to_device(keys), keylen)
    got = p.results()
    for i in range(3):
        p.check(got, i, keys[i])
    report("edge_fit", 3, keylen, p, 3, 0)
    p.close()


def test_refused_when_only_the_key_table_does_not_fit(ctx):
    """lds_edge(N_FIT + 7): the one-key image fits, the key table behind it does not.  Both keyed calls are argument errors
    that name themselves and the key table, they leave R, slab and outputs of the pass before them alone, and the one-key
    kernels still serve the batch."""
    shape = kg.predict("edge_over", 3)
    assert shape.wires_in_lds and not shape.keyed and shape.lds <= kg.LDS_LIMIT < shape.keyed_lds
    p = Pair(ctx, kg.build("edge_over"), 3, "over", shape)
    assert p.gb.lds_wires and not p.gb.keyed_supported() and not p.ev.keyed_supported()
    key = drbg("keyed/over/key", 32)
    p.one_key(key)
    before = p.results()
    for i in range(3):
        p.check(before, i, key)
    d_keys = ctx.to_device(kg.edge_keys("over", 3, 32))
    for keylen in (32, 16):
        with pytest.raises(engine.EngineError) as e:
            p.gb.garble_keyed(d_keys, keylen, p.d_rnd)
        assert e.value.code == engine.GC_E_ARG
        msg = engine.lib().gc_last_error()
        assert b"gc_batch_garble_keyed" in msg and b"key table" in msg
        with pytest.raises(engine.EngineError) as e:
            p.ev.eval_keyed(d_keys, keylen, p.gb)
        assert e.value.code == engine.GC_E_ARG
        msg = engine.lib().gc_last_error()
        assert b"gc_batch_eval_keyed" in msg and b"key table" in msg
    p.ctx.sync()
    after = {"R": p.gb.read_r(), "slab": p.gb.read_slab(), "l0": p.gb.read_outputs(), "active": p.ev.read_outputs(),
             "bits": p.d_out.numpy()}
    p.check_same(after, before, np.arange(3), "after the refused calls:")
    p.one_key(key)
    again = p.results()
    for i in range(3):
        p.check(again, i, key, "one key, after the refused calls:")
    p.close()


def test_the_lds_edge_circuit_at_1027_instances(ctx):
    """The circuit of test_key_table_that_ends_at_the_last_byte_of_lds at a batch that would get tiles of four: LDS cuts the
    tile to ONE instance for the one-key image, and the key table of one instance then still fits, so the keyed calls are in
    scope.  This pins what the engine does today (the tile is chosen for the one-key image and the keyed calls take it or
    refuse); whether they should fall back to a narrower tile of their own is a design question this test does not answer.
    35 instances to the oracle."""
    shape = kg.predict("edge_fit", 1027)
    assert (shape.ti, shape.keyed) == (1, True)
    p = Pair(ctx, kg.build("edge_fit"), 1027, "edge1027", shape)
    keys = kg.edge_keys("edge1027", 1027, 32)
    p.keyed(ctx.to_device(keys), 32)
    got = p.results()
    smp = kg.sample(1027, 1)
    for i in smp:
        p.check(got, i, keys[i])
    report("edge_fit", 1027, 32, p, len(smp), 0)
    p.close()
