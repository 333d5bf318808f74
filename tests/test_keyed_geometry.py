"""The shapes the keyed-kernel GPU tests rely on, checked on the host: every circuit of tests/keyed_geometry.py is planned
(engine.Plan, no GPU) and the tile width, part count and keyed scope that the plain-Python restatement predicts for each
(circuit, batch) of the GPU matrix are compared with values written out here.  A change of the planner or of a generator that
moves a case off the code path it is there for fails here first; so does a change of the restated tile rule or LDS formulas."""
import ctypes as C

import pytest

from mpc_amd import engine
from tests import keyed_geometry as kg

# (n_flat_slots, stage stride in uint4, largest part count) of every circuit's plan
FIGURES = {
    "adder8": (25, 12, 1),
    "wide": (744, 256, 1),
    "mixed": (693, 256, 1),
    "mixed_small": (69, 44, 1),
    "parity2": (64, 44, 2),
    "parity4": (291, 668, 4),
    "edge_fit": (6104, 4, 1),
    "edge_over": (6111, 4, 1),
}

# (circuit, batch) -> (instances per tile, parts, keyed calls in scope): the matrix of tests/test_gpu_batch_keyed_shapes.py
# and of the parity cases of tests/test_gpu_batch_keyed.py
MATRIX = {
    # every key length x HAS_OR x role: tiles of 1 and of 4 with a ragged last tile
    ("adder8", 5): (1, 1, True), ("adder8", 1027): (4, 1, True),
    ("wide", 5): (1, 1, True), ("wide", 1027): (4, 1, True),
    ("mixed", 5): (1, 1, True), ("mixed", 1027): (4, 1, True),
    # every tile width (one-part lists, small live set: neither cap nor LDS cuts the tile)
    ("adder8", 515): (2, 1, True), ("adder8", 2051): (8, 1, True), ("adder8", 4099): (16, 1, True),
    ("adder8", 8195): (32, 1, True), ("adder8", 16389): (64, 1, True),
    ("mixed_small", 2051): (8, 1, True), ("mixed_small", 16389): (64, 1, True),
    # lists in parts: the caps parts * TI <= 16
    ("parity2", 300): (1, 2, True), ("parity2", 4099): (8, 2, True),
    ("parity4", 300): (1, 4, True), ("parity4", 4099): (4, 4, True),
    # the end of LDS
    ("edge_fit", 3): (1, 1, True), ("edge_over", 3): (1, 1, False), ("edge_fit", 1027): (1, 1, True),
    # not run on the device by the keyed tests; here they hold the two LDS formulas in place: LDS cuts the tile of `wide`
    # from 8 to 4, and `mixed` keeps tiles of 8 whose one-key image fits (162 816 bytes) while the keyed one does not
    ("wide", 2051): (4, 1, True), ("mixed", 2051): (8, 1, False),
}


@pytest.mark.parametrize("name", sorted(FIGURES))
def test_plan_figures(name):
    assert kg.plan_figures(kg.build(name)) == FIGURES[name]


@pytest.mark.parametrize("name,batch", sorted(MATRIX))
def test_predicted_shape(name, batch):
    s = kg.predict(name, batch)
    assert s.wires_in_lds
    assert s.as_tuple() == MATRIX[(name, batch)]


def test_restated_rule_on_written_out_figures():
    """the tile rule and the two formulas on figures chosen by hand, without a plan"""
    # 4112 + 2 * 12 + 26 * 64 = 5 800 uint4
    assert kg.one_key_bytes(25, 12, 64) == 5800 * 16 and kg.keyed_bytes(25, 12, 64) == 5800 * 16 + 15360
    assert [kg.tile_log2(b, 25, 12, 1) for b in (511, 512, 1023, 1024, 16383, 16384, 1 << 20)] == [0, 1, 1, 2, 5, 6, 6]
    assert [kg.tile_log2(1 << 20, 25, 12, parts) for parts in (1, 2, 4)] == [6, 3, 2]
    # LDS cuts: 4112 + 512 + 745 TI <= 10 240 uint4 holds up to TI = 4 (7 092), not 8 (10 584)
    assert kg.tile_log2(1 << 20, 744, 256, 1) == 2
    # one instance does not fit (4112 + 8 + 6 121 = 10 241 uint4): the wires stay in HBM and LDS does not cut the tile
    assert kg.one_key_bytes(6120, 4, 1) == kg.LDS_LIMIT + 16 and kg.tile_log2(1 << 20, 6120, 4, 1) == 6
    s = kg.Shape(6120, 4, 1, 3)
    assert not s.wires_in_lds and not s.keyed


def test_the_key_table_of_edge_fit_ends_at_the_last_byte_of_lds():
    s = kg.predict("edge_fit", 3)
    assert (s.ti, s.lds, s.keyed_lds) == (1, kg.LDS_LIMIT - 240, kg.LDS_LIMIT)


def test_one_more_input_is_one_more_slot_up_to_the_end_of_the_one_key_image():
    """N_FIT is the largest n whose keyed image fits; n = N_FIT + 1 .. N_FIT + 15 fit the one-key kernels only; N_FIT + 16 does
    not fit LDS at all"""
    for d in range(-1, 17):
        nls, ustride, parts = kg.plan_figures(kg.lds_edge(kg.N_FIT + d))
        assert (nls, ustride, parts) == (kg.N_FIT + d + 3, 4, 1)
        s = kg.Shape(nls, ustride, parts, 3)
        assert s.keyed == (d <= 0), d
        assert s.wires_in_lds == (d <= 15), d
        assert s.keyed_lds == kg.LDS_LIMIT + 16 * d


def test_mixed_small_has_every_gate_kind_and_parity_circuits_every_list_flag():
    st = kg.build("mixed_small").stats()
    assert all(st[k] for k in ("AND", "OR", "INV", "XOR", "XNOR"))
    for name in ("parity2", "parity4"):
        st = kg.build(name).stats()
        assert all(st[k] for k in ("AND", "OR", "INV", "XOR", "XNOR"))


def test_samples_cover_the_first_and_the_last_two_tiles():
    s = kg.sample(16389, 64)
    assert set(range(64)) <= set(s) and set(range(16320, 16389)) <= set(s) and 37 * 100 in s
    assert len(s) == 573
    assert kg.sample(5, 1) == [0, 1, 2, 3, 4]


def test_keys_have_the_edge_patterns():
    for keylen in (16, 24, 32):
        k = kg.edge_keys("t", 1027, keylen)
        assert not k[0].any() and (k[1] == 0xFF).all()
        assert (k[2][:-1] == k[3][:-1]).all() and k[2][-1] != k[3][-1]
        assert (k[4][1:] == k[5][1:]).all() and k[4][0] != k[5][0]
        pool, keys = kg.pool_keys("t", 100, keylen)
        assert all((keys[i] == pool[i % 3]).all() for i in range(100))


def test_flat_geometry_call():
    L = engine.lib()
    c = kg.build("parity2")
    p = engine.Plan(c.Gates, c.NumWires, c.num_inputs, c.num_outputs)
    assert p.flat_geometry() == (44, 2)
    us, mp = C.c_uint32(7), C.c_uint32(7)
    assert L.gc_plan_flat_geometry(p.h, None, C.byref(mp)) == engine.GC_OK and mp.value == 2
    assert L.gc_plan_flat_geometry(p.h, C.byref(us), None) == engine.GC_OK and us.value == 44
    assert L.gc_plan_flat_geometry(None, C.byref(us), C.byref(mp)) == engine.GC_E_ARG
    # more than 65 534 live labels: no flattened plan
    c = kg.lds_edge(66000)
    p = engine.Plan(c.Gates, c.NumWires, c.num_inputs, c.num_outputs)
    assert p.info.n_flat_slots == 0xFFFFFFFF
    us.value = 7
    assert L.gc_plan_flat_geometry(p.h, C.byref(us), C.byref(mp)) == engine.GC_E_ARG and us.value == 7
    with pytest.raises(engine.EngineError) as e:
        p.flat_geometry()
    assert e.value.code == engine.GC_E_ARG
