"""Small levelised circuits for the split form of the keyed HBM-wire kernels (mpc_amd/csrc/fused_hbm_keyed_split_kernels.hip):
consecutive levels with prescribed gate counts, so that a level has exactly the column lanes a test needs at a tile width.

levels_circuit places every gate of level k on one output of level k - 1 (operand a; level 0: an input) and one input (operand
b), so the plan's levels are the lists given here (tests/test_keyed_split_cases_host.py asserts it on the host plan).  lanes()
is the column-form lane count of col_lanes.h per level: garbler AND 16, OR 16, INV 8 lanes per gate-instance, evaluator 8, 4,
4, free gates one."""
import numpy as np

from mpc_amd import engine
from mpc_amd.circuit import AND, GATE, INV, OR, XNOR, XOR, Circuit

NINPUTS = 48


def levels_circuit(name, levels, seed=1):
    """levels: [{AND: n, OR: n, INV: n, XOR: n, XNOR: n}]; the gates of a level in a shuffled order.  The last level's gates
    are the circuit's outputs."""
    rng = np.random.default_rng(seed)
    gates, nw, prev = [], NINPUTS, list(range(NINPUTS))
    for lv in levels:
        ops = [op for op, n in lv.items() for _ in range(n)]
        rng.shuffle(ops)
        cur = []
        for i, op in enumerate(ops):
            a = prev[i % len(prev)]
            b = int(rng.integers(0, NINPUTS))
            gates.append((a, 0 if op == INV else b, nw, op, 0))
            cur.append(nw)
            nw += 1
        prev = cur
    return Circuit(nw, [NINPUTS // 2, NINPUTS - NINPUTS // 2], [len(prev)], np.array(gates, GATE), name)


def lanes(lv, ti, ev):
    """column-form lanes of a level at tiles of ti instances: (hashed, free)"""
    a, o, i = (8, 4, 4) if ev else (16, 16, 8)
    return ti * (a * lv.get(AND, 0) + o * lv.get(OR, 0) + i * lv.get(INV, 0)), ti * (lv.get(XOR, 0) + lv.get(XNOR, 0))


def boundary(ti):
    """exactly 1 024 lanes and then the narrowest split level (1 024 + ti lanes), for the garbler and then for the evaluator:
    the plain single pass and the split on both sides of the form boundary"""
    g, e, x = 960 // (16 * ti), 960 // (8 * ti), 64 // ti
    return [{AND: g, XOR: x - 1, XNOR: 1}, {AND: g, XOR: x, XNOR: 1}, {AND: e, XOR: x}, {AND: e, XOR: x - 1, XNOR: 2}, {AND: 3, XOR: 2}]


def free_only(ti):
    """free gates only and wider than 1 024 lanes (H = 0), between two narrow levels"""
    return [{AND: 2, INV: 1, XOR: 5}, {XOR: 1100 // ti, XNOR: 7}, {AND: 2, XOR: 3}]


def one_and(ti):
    """one AND beside 400 XORs, and beside enough of them for a split at every tile width: fewer hash lanes than one wave"""
    return [{AND: 1, XOR: 400}, {AND: 1, XOR: 1100, XNOR: 30}, {INV: 1, XOR: 1200}, {AND: 2}]


def narrow_wide_narrow(ti):
    """narrow, wide, narrow, wide, narrow: the prefetched descriptor across a change of form; every gate kind"""
    wide = {AND: 100, OR: 21, INV: 33, XOR: 301, XNOR: 40}
    return [{AND: 5, OR: 2, INV: 3, XOR: 9, XNOR: 1}, wide, {AND: 4, OR: 1, INV: 2, XOR: 3},
            {AND: 120, OR: 9, INV: 15, XOR: 280, XNOR: 3}, {AND: 3, OR: 2, INV: 1, XNOR: 2}]


CASES = {"boundary": boundary, "free_only": free_only, "one_and": one_and, "narrow_wide_narrow": narrow_wide_narrow}


def build(name, ti):
    return levels_circuit("%s_ti%d" % (name, ti), CASES[name](ti), seed=len(name) + ti)


def plan_levels(c):
    """[{op: count}] per level of the circuit's host plan"""
    p = engine.Plan(c.Gates, c.NumWires, c.num_inputs, c.num_outputs)
    out = [dict() for _ in range(int(p.info.nlevels))]
    for lv, op in zip(p.level_of_gate, c.Gates["op"]):
        d = out[int(lv)]
        d[int(op)] = d.get(int(op), 0) + 1
    return out
