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
    for cls, names in ((engine.StreamBatch, ("garble", "get", "gather_wires", "close")),
                       (engine.StreamEvalBatch, ("set_wires", "get", "circuit", "close"))):
        for m in names:
            assert callable(getattr(cls, m)), m
