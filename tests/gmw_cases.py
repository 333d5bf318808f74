"""The circuits both GMW test sides run: tests/test_gmw_plan_walk.py walks the host plan of each on the CPU, and
tests/test_gpu_gmw.py sends the same ones through the engine.  Directed circuits, each with what it pins, and the parameters
of the seeded random ones (tests/py_gmw_reference.py: fuzz_circuit)."""
import numpy as np

from mpc_amd.circuit import AND, GATE, INV, XNOR, XOR, Circuit
from tests import py_gmw_reference as R

GC_E_WIRE = -8


def _circ(name, inputs, nout, nwires, gates):
    g = np.zeros(len(gates), GATE)
    for k, (a, b, out, op) in enumerate(gates):
        g[k] = (a, b, out, op, 0)
    return Circuit(nwires, inputs, [nout], g, name=name)


def _one_and_level(n):
    """one level of exactly n ANDs over 16 inputs, every AND an output: the level's last triple word is full (64, 128) or
    holds one gate (65), and the outputs fill whole words or spill one bit"""
    gates = [(k % 16, (7 * k + 1) % 16, 16 + k, AND) for k in range(n)]
    return _circ("one_level_%d_ands" % n, [8, 8], n, 16 + n, gates)


def _mixed(nout):
    """40 inputs, 70 gates on fresh wires (an AND every fifth), the last nout wires the outputs"""
    ops = [XOR, XNOR, INV, XOR, AND]
    gates = []
    for k in range(70):
        op = ops[k % 5]
        a = (3 * k) % (40 + k)
        gates.append((a, 0 if op == INV else (5 * k + 1) % (40 + k), 40 + k, op))
    return _circ("noutputs_%d" % nout, [20, 20], nout, 110, gates)


def directed():
    """[(circuit, status)]: status is what the planner answers (0, or GC_E_WIRE for the one it must refuse)"""
    out = []

    def add(c, status=0):
        out.append((c, status))

    # no gates at all: nlevels 1, one round that neither closes nor opens anything; the outputs are input wires
    add(_circ("no_gates", [2, 2], 2, 4, []))
    # free gates only, a chain four deep beside two independent gates: one round, sub-rounds, no triples, no message
    add(_circ("free_only", [2, 2], 3, 10,
              [(0, 1, 4, XOR), (4, 2, 5, XNOR), (5, 0, 6, INV), (6, 3, 7, XOR), (2, 3, 8, XNOR), (1, 0, 9, INV)]))
    # ANDs only, two levels: rounds with no free gate (nsub = 0), so the open reads straight after the close
    add(_circ("ands_only", [2, 2], 1, 7, [(0, 1, 4, AND), (2, 3, 5, AND), (4, 5, 6, AND)]))
    # an AND on the last level feeds the output: the closing round is empty but for the z fold and the output read
    add(_circ("and_on_last_level", [2, 1], 1, 5, [(0, 1, 3, XOR), (3, 2, 4, AND)]))
    add(_one_and_level(64))
    add(_one_and_level(65))
    add(_one_and_level(128))
    # x ^ x, x XNOR x and x & x: one slot read twice by one gate
    add(_circ("same_wire_twice", [1, 1], 3, 5, [(0, 0, 2, XOR), (0, 0, 3, XNOR), (1, 1, 4, AND)]))
    # a free gate overwrites input wire 1, a later gate reads the new value, and the overwritten wire is an output
    add(_circ("free_gate_overwrites_input", [1, 1], 2, 3, [(0, 1, 1, XOR), (0, 1, 2, XNOR)]))
    # wire 0 is overwritten by a free gate of level 0 that stands AFTER an AND of level 0 reading wire 0: in the bucketed
    # order the free gate runs first, so the AND reads the new value (circuit order would give it the old one)
    add(_circ("free_gate_before_and_of_its_level", [2, 1], 1, 5, [(0, 1, 3, AND), (0, 2, 0, XOR), (3, 0, 4, XOR)]))
    # AND A sets wire 3, a free gate of the same level sets it again (so wire 3 is back on level 0), AND B of that level
    # reads it: both ANDs read before either writes, so B reads the free gate's value and wire 3 ends as A's output, which
    # the last gate (level 1) reads
    add(_circ("ands_read_before_they_write", [2, 1], 2, 6, [(0, 1, 3, AND), (1, 2, 3, XOR), (3, 0, 4, AND), (3, 4, 5, XOR)]))
    add(_mixed(0))
    add(_mixed(64))
    add(_mixed(65))
    # the output wire 3 is set by no gate and is no input
    add(_circ("output_never_set", [1, 1], 1, 4, [(0, 1, 2, XOR)]), GC_E_WIRE)
    return out


def directed_parties(k):
    """parties of the k-th directed circuit: 2 .. 5 in turn"""
    return 2 + k % 4


REUSE = (0.0, 0.05, 0.3, 0.6)
P_AND = (0.0, 0.05, 0.3, 0.6, 0.9)
N_FUZZ = 1000  # circuits the host walk runs


def fuzz_case(seed):
    """(circuit, P) of seed: P, reuse and p_and walk their whole grid every 80 seeds; 1 .. 1 199 gates, P .. 149 inputs"""
    rng = np.random.default_rng(7000 + seed)
    P = 2 + seed % 4
    reuse = REUSE[(seed // 4) % 4]
    p_and = P_AND[(seed // 16) % 5]
    ni = int(rng.integers(P, 150))
    ng = int(rng.integers(1, 1200))
    return R.fuzz_circuit(rng, ni, ng, reuse, nargs=P, p_and=p_and), P


# the fuzz circuits the engine runs: (seed, batch, device form).  P = 2 + seed % 4, so P = 5 runs in both forms.
GPU_BATCHES = (1, 63, 64, 65, 257, 1000)
GPU_FUZZ = [(7 * k, GPU_BATCHES[k % 6], k % 4 == 3 or k % 3 == 1) for k in range(24)] + [(83, 65, False), (166, 257, True)]


def pass_data(c, P, n, seed):
    """(bits [n][ninputs], input shares, triples) of one pass"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, (n, c.num_inputs)).astype(np.uint8)
    shares = R.share_inputs(rng, c, bits, P)
    trip = R.beaver_triples(rng, P, R.triple_words(c)[2], n)
    return bits, shares, trip


def plain_bucketed_batch(c, bits):
    """R.plain_bucketed over a batch: bits [n][ninputs] -> [noutputs][n].  The same walk (free gates of a level in circuit
    order, then its ANDs, all reading before any writes) with the instances as a numpy axis."""
    ands, rest = R.buckets(c)
    gin0, gin1, gout, gop = (c.Gates[k].tolist() for k in ("in0", "in1", "out", "op"))
    bits = np.asarray(bits, np.uint8) & 1
    wv = np.zeros((c.NumWires, bits.shape[0]), np.uint8)
    wv[: c.num_inputs] = bits.T
    for i in range(len(ands)):
        for g in rest[i]:
            wv[gout[g]] = wv[gin0[g]] ^ 1 if gop[g] == INV else wv[gin0[g]] ^ wv[gin1[g]] ^ (1 if gop[g] == XNOR else 0)
        vals = [wv[gin0[g]] & wv[gin1[g]] for g in ands[i]]
        for g, v in zip(ands[i], vals):
            wv[gout[g]] = v
    return wv[c.NumWires - c.num_outputs:]
