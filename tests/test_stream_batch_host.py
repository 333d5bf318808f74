"""The session-batched streaming calls (gc_stream_batch_* / gc_stream_eval_batch_*) through what needs no GPU: the step size
that every session shares (gc_stream_batch_step_bytes against the oracle's Streaming.Garble), the steps refused by their
shape, the keyed scope of the program the device tests run, and the bindings."""
import numpy as np
import pytest

import oracle
from mpc_amd import engine
from mpc_amd.circuit import GATE
from tests import keyed_geometry as kg
from tests.test_oracle_stream import make_program
from tests.util import drbg

# the byte counts DESIGN.md section 16 quotes: appended steps start at offsets = 0, 8, 14 mod 16 at base 0
STEP_BYTES = {0: (2552, 11526, 4158), 0x20000: (2926, 12550, 4798)}


def alias_gates():
    """the in-place circuit of tests/test_gpu_stream.py: wires 0, 1 inputs; 2 tmp; 3, 4 outputs; in = [0, 1], out = [0, 2]"""
    gates = np.zeros(4, GATE)
    gates[0] = (0, 1, 2, 2, 0)
    gates[1] = (2, 1, 3, 0, 0)
    gates[2] = (0, 1, 4, 2, 0)
    gates[3] = (4, 0, 4, 0, 0)
    return gates


@pytest.mark.parametrize("base", [0, 0x20000])
def test_step_bytes_equal_the_oracles_stream(base):
    steps, prim = make_program(base)
    og = oracle.Stream(drbg("sbk", 32), drbg("sbr", 16 * (len(prim) + 1)), prim)
    for (c, in_, out_), want in zip(steps, STEP_BYTES[base]):
        n = engine.stream_batch_step_bytes(c.Gates, c.NumWires, in_, out_)
        assert n == len(og.garble(c.Gates, c.NumWires, in_, out_)) == want
    if base:
        # both id forms within one step: gates on tmp wires alone keep the 16-bit form
        c, in_, out_ = steps[0]
        data = og.garble(c.Gates, c.NumWires, in_, out_)
        from tests import hostile_fuzz as hf
        gates, err = hf.parse(data, c.NumGates)
        assert err is None and len({bool(data[q[0]] & 0x10) for q in gates}) == 2


def test_step_bytes_of_the_in_place_step():
    og = oracle.Stream(drbg("alias", 32), drbg("alias-rnd", 64), [0, 1, 2])
    assert engine.stream_batch_step_bytes(alias_gates(), 5, [0, 1], [0, 2]) == len(og.garble(alias_gates(), 5, [0, 1], [0, 2]))


def test_steps_refused_by_their_shape_have_no_size():
    L = engine.lib()
    g = alias_gates()
    assert engine.stream_batch_step_bytes(g, 5, [0, 1], [0, 2]) > 0
    # the output range overlaps the input range: nwires - nout < nin
    assert engine.stream_batch_step_bytes(g, 5, [0, 1, 5, 6], [0, 2]) == 0
    assert "overlaps" in L.gc_last_error().decode()
    # a gate writes an input-mapped wire
    bad = g.copy()
    bad[1]["out"] = 1
    assert engine.stream_batch_step_bytes(bad, 5, [0, 1], [0, 2]) == 0
    assert "input-mapped" in L.gc_last_error().decode()
    # the garble call itself answers both, and a null handle, with GC_E_ARG
    i, o, n = np.array([0, 1], np.uint32), np.array([0, 2], np.uint32), engine.C.c_size_t(0)
    assert L.gc_stream_batch_garble(None, engine._p(g), 4, 5, engine._p(i), 2, engine._p(o), 2, None, 64, engine.C.byref(n)) == engine.GC_E_ARG
    assert L.gc_stream_eval_batch_circuit(None, 0, 0, 0, None, 0, None, 0, None, engine.C.byref(n)) == engine.GC_E_ARG
    st = engine.C.c_int(0)
    assert L.gc_stream_batch_create(None, 4, None, 32, None, None, 0, engine.C.byref(st)) is None and st.value == engine.GC_E_ARG


def test_the_program_of_the_device_tests_is_inside_the_keyed_scope():
    """every step has a flattened plan and a keyed image that fits at the session counts the device tests use: tiles of one
    instance at 3, 5 and 67 sessions, of four at 1 027"""
    steps, _ = make_program(0)
    for c, _, _ in steps:
        fig = kg.plan_figures(c)
        for S, ti in ((3, 1), (5, 1), (67, 1), (1027, 4)):
            shape = kg.Shape(*fig, S)
            assert shape.keyed and shape.ti == ti, (c.NumGates, S, shape.as_tuple())


def test_python_binding_has_the_classes():
    for cls, names in ((engine.StreamBatch, ("garble", "get", "gather_wires", "cache_stats", "close")),
                       (engine.StreamEvalBatch, ("set_wires", "get", "circuit", "cache_stats", "close"))):
        for m in names:
            assert callable(getattr(cls, m)), m


# ---- what tests/test_gpu_stream_batch_bounds.py relies on (tests/stream_batch_bounds_cases.py) ----------------------------


def bounds_references():
    """(tag, reference) of every program of the bounds tests (the 65 535-session one on a handful of sessions)"""
    from tests import stream_batch_bounds_cases as bc
    wide = bc.wide_program()
    return [("lru", bc.reference("lru", bc.lru_program(), bc.LRU_SESSIONS, 32)),
            ("growth", bc.reference("growth", bc.growth_program(), bc.GROWTH_SESSIONS, bc.GROWTH_KEYLEN)),
            ("cap", bc.reference("cap", bc.cap_program(), bc.CAP_SESSIONS, 32)),
            ("big/host", bc.reference("big/host", bc.big_program(), 7, 32)),
            ("wide", bc.reference("wide", wide, bc.WIDE_SESSIONS, 32, store=wide[0][0][2] + wide[0][1][2]))]


def test_the_oracle_evaluates_every_bounds_program_to_its_plaintext_values():
    from tests import stream_batch_bounds_cases as bc
    for tag, ref in bounds_references():
        assert bc.evaluates_to_plaintext(ref), tag
        # single assignment, and no step writes a wire it reads: the final store holds every wire as its step left it
        outs = ref["outs"]
        assert len(set(outs)) == len(outs) and not set(outs) & set(ref["prim"]), tag
        for c, in_, out_ in ref["steps"]:
            assert len(in_) == c.num_inputs and len(out_) == c.num_outputs and len(set(in_)) == len(in_), tag


def test_the_id_maps_of_the_bounds_programs_grow_the_store_as_claimed():
    from tests import stream_batch_bounds_cases as bc
    # B4: the garbler starts with the primary inputs (below 1024), the evaluator empty.  Without the calls in between, step 2
    # and step 3 each grow the store under live labels, step 3 past the doubling and with ids in the 32-bit form
    steps, prim = bc.growth_program()
    garbler, evaluator = bc.growth_calls(False)
    assert bc.row_sequence(0, [i for _, i in garbler]) == [1024, 1024, 3001, 0x11000 + 40]
    assert bc.row_sequence(0, [i for _, i in evaluator]) == [1024, 1024, 1024, 3001, 0x11000 + 40]
    assert 0x11000 + 40 > 2 * 3001 and min(steps[2][2]) == 0x11000 > 0xFFFF
    assert max(prim) < 1024 and max(steps[0][1] + steps[0][2]) < 1024
    assert max(steps[1][1]) < 1024 and steps[1][2] == [3000]
    assert set(steps[2][1]) == set(steps[0][2] + steps[1][2])
    # with them, between steps 2 and 3: the gather of never-set ids and the set at 90000 each lie beyond the rows held when
    # they are made, so it is those calls that grow the store (and step 3 then finds room)
    garbler, evaluator = bc.growth_calls(True)
    seq = bc.row_sequence(0, [i for _, i in garbler])
    assert seq == [1024, 1024, 3001, 70004, 70004]
    assert min(bc.GROWTH_GATHER) >= dict(zip([c for c, _ in garbler], [0] + seq))["gather_wires"] == 3001
    seq = bc.row_sequence(0, [i for _, i in evaluator])
    assert seq == [1024, 1024, 1024, 3001, 90001, 90001]
    assert bc.GROWTH_SET >= dict(zip([c for c, _ in evaluator], [0] + seq))["set_wires"] == 3001
    # B5: both handles hold 1024 rows when the steps begin; the clamp is taken on the last
    steps, prim = bc.cap_program()
    ids = [max(max(i), max(o)) for _, i, o in steps]
    assert ids == list(bc.CAP_OUT_IDS) and max(prim) < 1024
    assert bc.row_sequence(1024, ids, bc.CAP) == [2048, 4096, 5000] and bc.row_sequence(1024, ids)[-1] == 8192
    for top in (bc.CAP - 1, bc.CAP):
        c, in_, out_ = bc.cap_edge_step(top)
        assert max(in_) < 1024 and max(out_) == top and len(set(out_)) == len(out_)
    # the restatement itself
    assert bc.rows_after(0, 0) == 1024 and bc.rows_after(1024, 1023) == 1024 and bc.rows_after(1024, 1024) == 2048
    assert bc.rows_after(4096, 4999, 5000) == 5000 and bc.rows_after(5000, 4999, 5000) == 5000


def test_every_step_of_the_bounds_programs_is_inside_the_keyed_scope():
    """a flattened plan and a keyed image that fits at the session count of its test (path 1 of gc_batch_keyed_path); the
    wide step has no LDS plan at all — 66 000 live inputs — so its wires are in HBM: path 2"""
    from tests import stream_batch_bounds_cases as bc
    small = [(c, bc.LRU_SESSIONS) for c in bc.lru_circuits()]
    small += [(c, bc.GROWTH_SESSIONS) for c, _, _ in bc.growth_program()[0]]
    small += [(c, bc.CAP_SESSIONS) for c, _, _ in bc.cap_program()[0]] + [(bc.cap_edge_step(0)[0], bc.CAP_SESSIONS)]
    for c, S in small:
        shape = kg.Shape(*kg.plan_figures(c), S)
        assert shape.keyed and shape.ti == 1, (c.name, shape.as_tuple())
    for c, _, _ in bc.big_program()[0]:
        for S in (bc.MAX_SESSIONS, 7):
            shape = kg.Shape(*kg.plan_figures(c), S)
            assert shape.keyed and shape.ti == (bc.BIG_TILE if S > 7 else 1), (c.name, S, shape.as_tuple())
    assert bc.MAX_SESSIONS % bc.BIG_TILE == 63  # the ragged last tile
    (wide, in_, out_), (c2, in2, _) = bc.wide_program()[0]
    plan = engine.Plan(wide.Gates, wide.NumWires, wide.num_inputs, wide.num_outputs)
    assert plan.info.n_flat_slots == 0xFFFFFFFF and plan.info.n_lds_slots * 16 > kg.LDS_LIMIT
    assert kg.Shape(*kg.plan_figures(c2), bc.WIDE_SESSIONS).keyed
    # more ids than a grid has rows, as permutations, and the second step reads across the 65 535th output
    assert len(in_) == len(out_) == bc.WIDE_N > 65535 and sorted(in_) != in_ and sorted(out_) != out_
    assert len(set(in_)) == len(set(out_)) == bc.WIDE_N and not set(in_) & set(out_)
    assert [out_.index(w) for w in in2[: len(bc.WIDE_READ)]] == list(bc.WIDE_READ)
    ops = wide.Gates["op"]
    assert (ops[96::97] == 2).all() and ops.tolist().count(2) == bc.WIDE_N // 97 and ops.tolist().count(0) == bc.WIDE_N - bc.WIDE_N // 97


def test_the_lru_model_on_a_hand_written_example():
    from tests import stream_batch_bounds_cases as bc
    m = bc.Lru(10)
    got = [m.step(n, s) + (m.stats(),) for n, s in (("a", 4), ("b", 4), ("a", 4), ("c", 4), ("b", 4), ("d", 11), ("d", 11), ("a", 4))]
    assert got == [("load", [], (1, 4, 1, 0)),
                   ("load", [], (2, 8, 2, 0)),
                   ("hit", [], (2, 8, 2, 0)),
                   ("load", ["b"], (2, 8, 3, 1)),           # b was used before a
                   ("load", ["a"], (2, 8, 4, 2)),
                   ("load", ["c", "b"], (1, 11, 5, 4)),     # larger than the whole budget: kept alone
                   ("hit", [], (1, 11, 5, 4)),
                   ("load", ["d"], (1, 4, 6, 5))]
    # the sequence of the device test with sizes of the right order: two evictions at c4, and c2 and c1 come back
    size = {0: 30, 1: 70, 2: 130, 3: 250}
    m = bc.Lru(size[0] + size[1] + max(size[2], size[3]) - 1)
    got = [m.step(k, size[k]) for k in bc.LRU_SEQUENCE]
    assert got == [("load", []), ("load", []), ("hit", []), ("load", []), ("hit", []), ("load", [1, 2]), ("load", [0]),
                   ("load", [3]), ("hit", [])]
    assert m.stats() == (2, 100, 6, 4)
    # a budget of one byte: every entry alone, evictions == loads - 1, the repeated step a hit
    m = bc.Lru(1)
    for k in bc.LRU_SEQUENCE:
        m.step(k, size[k])
        assert m.stats()[0] == 1 and m.stats()[3] == m.stats()[2] - 1 and m.stats()[1] == size[k]
    assert m.loads == len(bc.LRU_SEQUENCE) - 1
