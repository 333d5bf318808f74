"""Programs for the HOST side of the session-batched streaming handles (SbCore of mpc_amd/csrc/stream_batch.cpp): the circuit
cache and its eviction, growth of the wire store while labels are live, the wire-id cap, and the largest launch shapes.  Shared
by tests/test_stream_batch_host.py (what needs no GPU: the claims the device tests rely on) and
tests/test_gpu_stream_batch_bounds.py.

Every program is a list of steps (Circuit, in_, out_) over global wire ids plus the primary inputs `prim`, in the form of
tests/test_oracle_stream.make_program; reference() runs the oracle per session over it, in the form of
tests/test_gpu_stream_batch.reference.  The programs are single assignment (every out id is written once), so the final store
holds every wire as it was when its step ended.

Restated here in plain Python, from DESIGN.md section 16 and not by calling the library:
    rows_after()  the store's row count after an id is needed: min(max(id + 1, 2 * rows, 1024), cap)
    Lru           the cache: bounded in bytes, least recently used first, an entry larger than the budget kept alone"""
import numpy as np

import oracle
from mpc_amd.circuit import AND, GATE, INV, OR, XNOR, XOR, WIRE, Circuit, comparator64, synthetic_levelised
from tests import keyed_geometry as kg
from tests.test_oracle_stream import plain_program

MIN_ROWS = 1024
DEFAULT_CAP = 1 << 28  # far above every id used here; only the clamp at an explicit cap is restated


def rows_after(rows, max_id, cap=DEFAULT_CAP):
    """SbCore::ensure: the store holds ids [0, rows); an id past it doubles the store at the least, clamped to the cap"""
    if max_id < rows:
        return rows
    return min(max(max_id + 1, 2 * rows, MIN_ROWS), cap)


def row_sequence(rows, ids, cap=DEFAULT_CAP):
    """row count after each of the calls whose largest ids are ids[]"""
    out = []
    for i in ids:
        rows = rows_after(rows, i, cap)
        out.append(rows)
    return out


class Lru:
    """the circuit cache of a handle: step(name, size) -> ("hit" | "load", [names evicted])"""

    def __init__(self, budget):
        self.budget, self.tick, self.loads, self.evictions = budget, 0, 0, 0
        self.resident = {}  # name -> [size, last use]

    def step(self, name, size):
        self.tick += 1
        if name in self.resident:
            self.resident[name][1] = self.tick
            return "hit", []
        gone = []
        while self.resident and self.bytes() + size > self.budget:
            lru = min(self.resident, key=lambda n: self.resident[n][1])
            del self.resident[lru]
            gone.append(lru)
        self.evictions += len(gone)
        self.resident[name] = [size, self.tick]
        self.loads += 1
        return "load", gone

    def bytes(self):
        return sum(size for size, _ in self.resident.values())

    def stats(self):
        return (len(self.resident), self.bytes(), self.loads, self.evictions)


# ---- B1 / B2: four circuits of clearly different size, nine steps ------------------------------------------------------

# c1 c2 c1 c3 c1 c4 c2 c1, then c1 once more: a step applied twice in a row
LRU_SEQUENCE = (0, 1, 0, 2, 0, 3, 1, 0, 0)
LRU_SESSIONS = 5


def lru_circuits():
    return [synthetic_levelised(3, 8, 0.4, seed=71, ninputs=8, or_frac=0.1, inv_frac=0.1, xnor_frac=0.1),
            synthetic_levelised(4, 16, 0.4, seed=72, ninputs=8, or_frac=0.1, inv_frac=0.1, xnor_frac=0.1),
            synthetic_levelised(5, 24, 0.4, seed=73, ninputs=8, or_frac=0.1, inv_frac=0.1, xnor_frac=0.1),
            synthetic_levelised(6, 40, 0.4, seed=74, ninputs=8, or_frac=0.1, inv_frac=0.1, xnor_frac=0.1)]


def lru_program(sequence=LRU_SEQUENCE):
    """step k runs circuit sequence[k] on eight DISTINCT wires drawn from everything set so far and writes fresh ids: the
    same circuit gives other bytes every time it comes round, and every id stays below 1024 (the store does not grow)"""
    circs = lru_circuits()
    rng = np.random.default_rng(70)
    prim = list(range(1, 13))
    known, nxt, steps = list(prim), 20, []
    for k in sequence:
        c = circs[k]
        in_ = [int(w) for w in rng.choice(known, c.num_inputs, replace=False)]
        out_ = list(range(nxt, nxt + c.num_outputs))
        nxt += c.num_outputs
        known += out_
        steps.append((c, in_, out_))
    assert nxt <= MIN_ROWS
    return steps, prim


# ---- B4: growth with live labels ----------------------------------------------------------------------------------------

GROWTH_SESSIONS, GROWTH_KEYLEN = 5, 24
GROWTH_GATHER = [70000 + k for k in range(4)]  # never set, past the store when they are gathered (after step 2)
GROWTH_SET = 90000                             # set on the evaluator after step 2, past its store


def growth_program():
    """make_program's three circuits with another id map: step 1 below 1024, step 2 writes id 3000 (1024 -> 3001 rows), step 3
    reads the outputs of both and writes from 0x11000 up (the 32-bit id form; past the doubling)"""
    c1 = synthetic_levelised(5, 24, 0.3, seed=31, ninputs=16, or_frac=0.1, inv_frac=0.15, xnor_frac=0.1)
    c2 = comparator64()
    c3 = synthetic_levelised(4, 40, 0.5, seed=32, ninputs=c1.num_outputs + 1, inv_frac=0.1)
    in1, out1 = list(range(16)), [100 + i for i in range(c1.num_outputs)]
    in2, out2 = [200 + i for i in range(128)], [3000]
    out3 = [0x11000 + i for i in range(c3.num_outputs)]
    return [(c1, in1, out1), (c2, in2, out2), (c3, out1 + out2, out3)], in1 + in2


def growth_calls(between):
    """([(call, largest id)] of the garbler handle, of the evaluator handle) in the order tests/test_gpu_stream_batch_bounds.py
    makes them.  between: with the gather of never-set ids / the set at GROWTH_SET between steps 2 and 3 — those calls then do
    the growing that step 3 does without them, so the device test runs the program both ways."""
    steps, prim = growth_program()
    mx = [max(max(i), max(o)) for _, i, o in steps]
    garbler = [("create", max(prim)), ("step 1", mx[0]), ("step 2", mx[1]), ("gather_wires", max(GROWTH_GATHER)), ("step 3", mx[2])]
    evaluator = [("create", 0), ("set_wires prim", max(prim)), ("step 1", mx[0]), ("step 2", mx[1]), ("set_wires", GROWTH_SET),
                 ("step 3", mx[2])]
    if not between:
        garbler, evaluator = [c for c in garbler if c[0] != "gather_wires"], [c for c in evaluator if c[0] != "set_wires"]
    return garbler, evaluator


# ---- B5: the cap --------------------------------------------------------------------------------------------------------

CAP = 5000
CAP_SESSIONS = 5
CAP_OUT_IDS = (1500, 2500, CAP - 1)


def small_step(seed):
    return synthetic_levelised(3, 6, 0.4, seed=seed, ninputs=6, or_frac=0.15, inv_frac=0.15, xnor_frac=0.1)


def cap_program():
    """three steps whose last output goes to id 1500, 2500 and 4999: 1024 -> 2048 -> 4096 -> 5000 rows under a cap of 5000;
    each reads the primary inputs and the outputs of the step before"""
    prim = list(range(10, 16))
    steps, prev = [], []
    for k, top in enumerate(CAP_OUT_IDS):
        c = small_step(80 + k)
        in_ = (prev + prim)[: c.num_inputs]
        out_ = [300 + 10 * k + j for j in range(c.num_outputs - 1)] + [top]
        steps.append((c, in_, out_))
        prev = out_[-3:]
    return steps, prim


def cap_edge_step(top):
    """one step of the same shape whose last output goes to id `top` (4999: accepted, 5000: refused)"""
    c = small_step(90)
    return c, list(range(10, 16)), [400 + j for j in range(c.num_outputs - 1)] + [top]


# ---- B6: 65 535 sessions ------------------------------------------------------------------------------------------------

MAX_SESSIONS = 65535
BIG_TILE = 64  # the tile of both steps at 65 535 sessions (tests/test_stream_batch_host.py asserts it)


def forty():
    """40 gates, all five kinds, 8 inputs, 4 outputs: under one piece of the serialiser"""
    ops = (XOR, AND, OR, INV, XNOR)
    gates = np.zeros(40, GATE)
    for g in range(40):
        a = 8 + g - 1 if g else 0
        b = (3 * g + 1) % (8 + g)
        gates[g] = (a, 0 if ops[g % 5] == INV else b, 8 + g, ops[g % 5], 0)
    return Circuit(48, [4, 4], [4], gates, "forty")


def big_program():
    """stream_batch_cases.case("tiny"), then forty() over seven primary inputs and tiny's output"""
    from tests import stream_batch_cases as sbc
    tiny, tin, tout = sbc.case("tiny")
    prim = list(range(1, 8))
    return [(tiny, tin, tout), (forty(), prim + tout, [200, 201, 202, 203])], prim


def big_oracle_sessions():
    """kg.sample at the tile of 64 plus the last full wave and the ragged last tile of 63"""
    return sorted(set(kg.sample(MAX_SESSIONS, BIG_TILE)) | set(range(65472, MAX_SESSIONS)))


# ---- B7: more than 65 535 ids through k_sb_rows -------------------------------------------------------------------------

WIDE_N = 66000
WIDE_SESSIONS = 3
WIDE_READ = (0, 65534, 65535, 65536, 65999)  # output indices the second step must read


def wide_program():
    """step 1: WIDE_N inputs and outputs, out j = in[j] ^ in[(j + 1) % n], every 97th an AND; in[] and out[] are permutations
    of disjoint id ranges.  step 2: small_step-like circuit over 64 of those outputs, the indices of WIDE_READ among them."""
    n = WIDE_N
    gates = np.zeros(n, GATE)
    j = np.arange(n)
    gates["in0"], gates["in1"], gates["out"] = j, (j + 1) % n, n + j
    gates["op"] = np.where(j % 97 == 96, AND, XOR)
    wide = Circuit(2 * n, [n // 2, n - n // 2], [n], gates, "wide_%d" % n)
    rng = np.random.default_rng(97)
    in_ = [int(w) for w in rng.permutation(n) + 5]
    out_ = [int(w) for w in rng.permutation(n) + 70000]
    c2 = synthetic_levelised(3, 16, 0.4, seed=98, ninputs=64, or_frac=0.1, inv_frac=0.1, xnor_frac=0.1)
    idx = list(WIDE_READ) + [int(i) for i in rng.choice(np.setdiff1d(np.arange(n), WIDE_READ), 64 - len(WIDE_READ), replace=False)]
    in2 = [out_[i] for i in idx]
    out2 = [140000 + i for i in range(c2.num_outputs)]
    return [(wide, in_, out_), (c2, in2, out2)], in_


# ---- the oracle ---------------------------------------------------------------------------------------------------------

_refs = {}


def reference(tag, program, S, keylen, sessions=None, keys=None, store=None):
    """the oracle once per tag, in the form of tests/test_gpu_stream_batch.reference: keys, random streams, per session the
    bytes of every step, every program wire of the garbler's FINAL store (`wires`), the evaluator's input bits, its label of
    every output (`ev`, LABEL [S]) and the plaintext values.  sessions: the sessions the oracle runs (all by default); the rows
    of the others stay zero and their streams None.  store: the wires kept in `wires` (all primary inputs and outputs by default)."""
    from mpc_amd.circuit import LABEL
    from tests.test_gpu_stream_batch import rnd_streams
    if tag in _refs:
        return _refs[tag]
    steps, prim = program
    keys = kg.edge_keys("stream-batch/bounds/" + tag, S, keylen) if keys is None else keys
    rnd = rnd_streams("bounds/" + tag, S, len(prim))
    outs = [o for _, _, out_ in steps for o in out_]
    bits = np.random.default_rng(S + keylen + len(tag)).integers(0, 2, (S, len(prim)), dtype=np.uint8)
    sessions = list(range(S)) if sessions is None else list(sessions)
    streams, vals = [None] * S, [None] * S
    store = prim + outs if store is None else list(store)
    wires, ev = {w: np.zeros(S, WIRE) for w in store}, {o: np.zeros(S, LABEL) for o in outs}
    for s in sessions:
        g = oracle.Stream(keys[s].tobytes(), rnd[s].tobytes(), prim)
        e = oracle.StreamEval(keys[s].tobytes())
        for w, b in zip(prim, bits[s]):
            wire = g.get(w)
            e.set(w, wire["l1"] if b else wire["l0"])
        mine = []
        for c, in_, out_ in steps:
            data = g.garble(c.Gates, c.NumWires, in_, out_)
            assert e.circuit(c.NumGates, c.NumWires, max(max(in_), max(out_)) + 1, data) == len(data)
            mine.append(data)
        streams[s] = mine
        for w in store:
            wires[w][s] = g.get(w)
        for o in outs:
            ev[o][s] = e.get(o)
        vals[s] = plain_program(steps, prim, bits[s])
    _refs[tag] = dict(steps=steps, prim=prim, keys=keys, rnd=rnd, streams=streams, wires=wires, outs=outs, bits=bits, ev=ev,
                      vals=vals, sessions=sessions)
    return _refs[tag]


def evaluates_to_plaintext(ref):
    """the evaluator's label of every output is the garbler's label of the plaintext value, in every session the oracle ran"""
    for s in ref["sessions"]:
        for o in ref["outs"]:
            wire, val = ref["wires"][o][s], ref["vals"][s][o]
            if ref["ev"][o][s] != (wire["l1"] if val else wire["l0"]):
                return False
    return True
