"""Host-only GMW plan (gc_gmw_plan_describe, mpc_amd/csrc/gmw_plan.cpp) against the plain-Python restatement of
AssignLevels(TargetGMW) and the reference's triple-word accounting.  No GPU needed."""
import numpy as np
import pytest

from mpc_amd import engine
from mpc_amd.circuit import AND, GATE, OR, XOR
from tests import py_gmw_reference as R


def _describe(c):
    return engine.gmw_plan_describe(c.Gates, c.NumWires, c.num_inputs, c.num_outputs)


def _matches_restatement(c):
    info, lv, ai, wl = _describe(c)
    want_lv, mx = R.assign_levels_gmw(c)
    ands, rest = R.buckets(c)
    w, _, tw = R.triple_words(c)
    assert info.nlevels == mx + 1 == len(ands)
    assert lv.tolist() == want_lv
    assert wl.tolist() == w
    assert info.triple_words == tw and info.max_level_words == max(w)
    assert info.n_and_levels == sum(1 for a in ands if a)
    for level in ands:
        for k, g in enumerate(level):
            assert ai[g] == k
    ops = c.Gates["op"]
    assert (ai[ops != AND] == 0xFFFFFFFF).all()
    s = c.stats()
    assert (info.n_and, info.n_xor, info.n_xnor, info.n_inv) == (s["AND"], s["XOR"], s["XNOR"], s["INV"])
    assert (info.ngates, info.nwires, info.ninputs, info.noutputs) == (c.NumGates, c.NumWires, c.num_inputs, c.num_outputs)
    return info


def test_shipped_circuits(aes_circ, add64_circ):
    i = _matches_restatement(aes_circ)
    assert (i.nlevels, i.n_and_levels, i.triple_words) == (61, 60, 130)
    assert i.max_free_depth <= 16  # the longest XOR chain between two exchanges of aes_128
    i = _matches_restatement(add64_circ)
    assert (i.nlevels, i.n_and_levels, i.triple_words) == (64, 63, 63)


@pytest.mark.parametrize("nargs", [2, 3])
def test_fuzz_circuits_with_wire_reuse(nargs):
    rng = np.random.default_rng(40 + nargs)
    for k in range(40):
        c = R.fuzz_circuit(rng, int(rng.integers(nargs, 120)), int(rng.integers(1, 700)), [0.0, 0.05, 0.3][k % 3], nargs=nargs,
                           p_and=float(rng.choice([0.0, 0.1, 0.3, 0.6])))
        _matches_restatement(c)


def test_or_is_rejected(sha_circ):
    """sha256xor has one OR: "gate OR not supported" (network.go:609)"""
    assert sha_circ.stats()["OR"] == 1
    with pytest.raises(engine.EngineError) as e:
        _describe(sha_circ)
    assert e.value.code == engine.GC_E_GATE


def test_bad_arguments_are_rejected():
    g = np.zeros(1, GATE)
    g[0] = (0, 1, 2, XOR, 0)
    L = engine.lib()
    assert L.gc_gmw_plan_describe(None, 1, 3, 2, 1, None, None, None, None) == engine.GC_E_ARG  # gates NULL
    assert L.gc_gmw_plan_describe(engine._p(g), 1, 3, 4, 1, None, None, None, None) == engine.GC_E_ARG  # ninputs > nwires
    assert L.gc_gmw_plan_describe(engine._p(g), 1, 3, 2, 4, None, None, None, None) == engine.GC_E_ARG  # noutputs > nwires
    for bad, code in (((0, 1, 2, 9, 0), engine.GC_E_GATE), ((0, 1, 2, OR, 0), engine.GC_E_GATE),
                      ((0, 2, 2, XOR, 0), engine.GC_E_WIRE), ((0, 1, 5, XOR, 0), engine.GC_E_WIRE)):
        g[0] = bad
        with pytest.raises(engine.EngineError) as e:
            engine.gmw_plan_describe(g, 3, 2, 1)
        assert e.value.code == code, bad
    g[0] = (0, 1, 2, XOR, 0)
    info, lv, ai, wl = engine.gmw_plan_describe(g, 3, 2, 1)
    assert (info.nlevels, info.n_and_levels, info.triple_words) == (1, 0, 0)


def test_and_output_level_and_words():
    """70 ANDs on one level take two whole triple words; an AND's output is one level up"""
    n = 70
    g = np.zeros(n + 1, GATE)
    for k in range(n):
        g[k] = (k % 4, (k + 1) % 4, 4 + k, AND, 0)
    g[n] = (4, 5, 4 + n, XOR, 0)
    info, lv, ai, wl = engine.gmw_plan_describe(g, 5 + n, 4, 1)
    assert lv.tolist() == [0] * n + [1]
    assert ai.tolist() == list(range(n)) + [0xFFFFFFFF]
    assert wl.tolist() == [2, 0] and info.triple_words == 2 and info.max_level_words == 2
