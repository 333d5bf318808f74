"""The host side of the session-batched streaming handles — what owns device memory between the steps (SbCore of
mpc_amd/csrc/stream_batch.cpp, shared by gc_stream_batch and gc_stream_eval_batch): the circuit cache and its eviction
(GC_STREAM_BATCH_CACHE_BYTES, observed through cache_stats()), growth of the wire store while labels are live, the wire-id cap
(GC_STREAM_MAX_WIRES), 65 535 sessions, and more ids in one step than a grid has rows (k_sb_rows).

Every comparison is with oracle.Stream / oracle.StreamEval per session (tests/stream_batch_bounds_cases.reference); the programs
and the plain-Python restatements of the cache and of the store's growth live in tests/stream_batch_bounds_cases.py, and
tests/test_stream_batch_host.py asserts on the host what these tests rely on (growth sequences, keyed scope, kernel path).

Both switches are read once per process, so a test that sets one runs its body in a fresh child process, one after the other;
the child asserts, prints one JSON line, and the parent asserts on that."""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import oracle
from mpc_amd import engine
from mpc_amd.circuit import LABEL, WIRE
from tests import keyed_geometry as kg
from tests import stream_batch_bounds_cases as bc
from tests.test_gpu_stream_batch import FILL, active_labels, rnd_streams, stride_for
from tests.util import drbg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("GC_STREAM_BATCH_CACHE_BYTES", "GC_STREAM_MAX_WIRES")
TAG = "stream-batch bounds: "


class Pair:
    """a garbler handle and an evaluator handle over one reference; step(k) garbles step k for every session into a fresh
    buffer and feeds the evaluator those device bytes"""

    def __init__(self, ctx, ref, S, keylen, keys=None):
        self.ctx, self.ref, self.S, self.keylen = ctx, ref, S, keylen
        self.d_keys = engine.DeviceBuffer(ctx, data=ref["keys"] if keys is None else keys)
        self.d_rnd = engine.DeviceBuffer(ctx, data=ref["rnd"])
        self.sb = engine.StreamBatch(ctx, S, self.d_keys, keylen, self.d_rnd, ref["prim"])
        self.se = engine.StreamEvalBatch(ctx, S, self.d_keys, keylen)
        self.d_bad = engine.DeviceBuffer(ctx, shape=S, dtype=np.uint32)
        self.d_out = self.d_lab = None
        self.any = ref["sessions"][len(ref["sessions"]) // 2]  # the session whose bytes the evaluator parses

    def feed(self, from_device=False):
        """the evaluator's primary inputs: the active label of the reference's input bits (from_device: out of the garbler's
        own store, for references that do not hold every session's input wires)"""
        prim = self.ref["prim"]
        if from_device:
            d_w = engine.DeviceBuffer(self.ctx, shape=(self.S, len(prim)), dtype=WIRE)
            self.sb.gather_wires(prim, d_w)
            pairs = d_w.numpy()
            d_w.close()
            self.labels = np.ascontiguousarray(np.where(self.ref["bits"] == 1, pairs["l1"], pairs["l0"]))
        else:
            self.labels = np.ascontiguousarray(active_labels(self.ref, self.S))
        self.d_lab = engine.DeviceBuffer(self.ctx, data=self.labels)
        self.se.set_wires(prim, self.d_lab)

    def garble(self, k):
        c, in_, out_ = self.ref["steps"][k]
        self.n = engine.stream_batch_step_bytes(c.Gates, c.NumWires, in_, out_)
        self.stride, self.lead = stride_for(self.n), 1 + k % 3
        if self.d_out is not None:
            self.d_out.close()
        self.d_out = engine.DeviceBuffer(self.ctx, shape=self.lead + self.S * self.stride + 16)
        self.d_out.zero(FILL)
        assert self.sb.garble(c.Gates, c.NumWires, in_, out_, self.d_out + self.lead, self.stride) == self.n

    def evaluate(self, k, nwires=None):
        c, in_, out_ = self.ref["steps"][k]
        nwires = max(max(in_), max(out_)) + 1 if nwires is None else nwires
        block = self.ref["streams"][self.any][k]
        assert len(block) == self.n
        used = self.se.circuit(c.NumGates, c.NumWires, nwires, block, self.d_out + self.lead, self.stride, self.d_bad)
        assert used == self.n
        return self.d_bad.numpy()

    def step(self, k):
        """-> u8 [S][n]: every session's bytes of step k; nothing written around them, d_bad all zero"""
        self.garble(k)
        assert (self.evaluate(k) == 0).all()
        buf = self.d_out.numpy()
        body = buf[self.lead: self.lead + self.S * self.stride].reshape(self.S, self.stride)
        assert (buf[: self.lead] == FILL).all() and (buf[self.lead + self.S * self.stride:] == FILL).all()
        assert (body[:, self.n:] == FILL).all()
        return body[:, : self.n]

    def check_step(self, k, sessions=None):
        """step k on both handles: bytes, the garbler's store and the evaluator's labels of its outputs equal the oracle's"""
        ref = self.ref
        sessions = ref["sessions"] if sessions is None else sessions
        body = self.step(k)
        for s in sessions:
            assert body[s].tobytes() == ref["streams"][s][k], "step %d, session %d" % (k, s)
        self.check_wires(ref["steps"][k][2], sessions)
        return body

    def check_wires(self, wires, sessions=None):
        ref = self.ref
        idx = ref["sessions"] if sessions is None else sessions
        for w in wires:
            assert (self.sb.get(w)[idx] == ref["wires"][w][idx]).all(), "garbler, wire %d" % w
            if w in ref["ev"]:
                assert (self.se.get(w)[idx] == ref["ev"][w][idx]).all(), "evaluator, wire %d" % w

    def check_inputs(self):
        for j, w in enumerate(self.ref["prim"]):
            assert (self.se.get(w) == self.labels[:, j]).all(), "evaluator, input wire %d" % w

    def snapshot(self, extra=()):
        """every program wire (and `extra`) of both stores"""
        ws = list(self.ref["wires"]) + list(extra)
        return [self.sb.get(w).copy() for w in ws], [self.se.get(w).copy() for w in ws]

    def same(self, snap, extra=()):
        now = self.snapshot(extra)
        return all((a == b).all() for x, y in zip(snap, now) for a, b in zip(x, y))

    def close(self):
        self.sb.close(), self.se.close()
        for d in (self.d_keys, self.d_rnd, self.d_bad, self.d_out, self.d_lab):
            if d is not None:
                d.close()


def refused(fn, *args):
    """the call answers GC_E_ARG; -> gc_last_error()"""
    with pytest.raises(engine.EngineError) as err:
        fn(*args)
    assert err.value.code == engine.GC_E_ARG
    return engine.lib().gc_last_error().decode()


def run_child(call, env=None, timeout=120):
    """tests.test_gpu_stream_batch_bounds.<call> in ONE fresh process, without the two switches unless env sets them"""
    code = "import os, sys; sys.path.insert(0, os.getcwd()); from tests import test_gpu_stream_batch_bounds as t; t." + call
    args = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code]
    full = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    full.update(env or {})
    r = subprocess.run(args, cwd=ROOT, env=full, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, "child exit status %d\n%s\n%s" % (r.returncode, r.stdout[-4000:], r.stderr[-4000:])
    line = [l for l in r.stdout.splitlines() if l.startswith(TAG)][-1]
    return json.loads(line[len(TAG):])


# ---- B1 / B2: the circuit cache ---------------------------------------------------------------------------------------------


def lru_child(sizes=None):
    """the nine steps of bc.lru_program on both handles, the oracle's bytes and labels after every step.  sizes None (default
    budget): nothing is evicted; reports what each circuit adds to `bytes` on either handle.  Otherwise: after every step the
    counters of either handle equal those of bc.Lru over these sizes and the budget of this process."""
    S = bc.LRU_SESSIONS
    ref = bc.reference("lru", bc.lru_program(), S, 32)
    ctx = engine.Context(0)
    pair = Pair(ctx, ref, S, 32)
    pair.feed()
    handles = {"garbler": pair.sb, "evaluator": pair.se}
    out = {"steps": {h: [] for h in handles}, "kinds": {h: [] for h in handles}}
    if sizes is None:
        out["sizes"] = {h: [None] * 4 for h in handles}
    else:
        budget = int(os.environ["GC_STREAM_BATCH_CACHE_BYTES"])
        models = {h: bc.Lru(budget) for h in handles}
    assert pair.sb.cache_stats() == pair.se.cache_stats() == (0, 0, 0, 0)
    for k, circ in enumerate(bc.LRU_SEQUENCE):
        before = {h: handles[h].cache_stats() for h in handles}
        pair.check_step(k)
        for h in handles:
            got = handles[h].cache_stats()
            if sizes is None:
                first = circ not in bc.LRU_SEQUENCE[:k]
                assert got[2] == before[h][2] + first and got[3] == 0 and got[0] == got[2], (h, k, got)
                if first:
                    out["sizes"][h][circ] = got[1] - before[h][1]
                    assert got[1] > before[h][1]
                else:
                    assert got[1] == before[h][1]
            else:
                kind, gone = models[h].step(circ, sizes[h][circ])
                assert got == models[h].stats(), (h, k, got, models[h].stats())
                out["kinds"][h].append([kind, gone])
            out["steps"][h].append(list(got))
    pair.check_wires(ref["wires"])
    pair.check_inputs()
    pair.close()
    ctx.close()
    print(TAG + json.dumps(out))


_sizes = {}


def lru_sizes():
    """device bytes of c1..c4 in the cache of either handle, from a run under the default budget (once per test process)"""
    if not _sizes:
        got = run_child("lru_child()")
        _sizes.update(got["sizes"])
        for h, sizes in _sizes.items():
            assert all(sizes) and got["steps"][h][-1] == [4, sum(sizes), 4, 0], (h, got)
        g = _sizes["garbler"]
        assert g[0] < g[1] < g[2] < g[3], g
    return _sizes


def expected(sizes, budget):
    want = {}
    for h in sizes:
        m = bc.Lru(budget)
        want[h] = []
        for circ in bc.LRU_SEQUENCE:
            kind, gone = m.step(circ, sizes[h][circ])
            want[h].append((list(m.stats()), [kind, gone]))
    return want


def test_cache_evicts_least_recently_used_first_exactly():
    """budget = bytes(c1) + bytes(c2) + max(bytes(c3), bytes(c4)) - 1 of the garbler handle, the sizes measured by a run of
    their own; c1 c2 c1 c3 c1 c4 c2 c1 c1.  (entries, bytes, loads, evictions) after every step equal the model's on both
    handles (asserted in the child too, with the oracle's bytes, stores and labels): loading c4 evicts c2, then c3; c2 and
    c1 come back after their eviction."""
    sizes = lru_sizes()
    g = sizes["garbler"]
    budget = g[0] + g[1] + max(g[2], g[3]) - 1
    got = run_child("lru_child(%r)" % (sizes,), {"GC_STREAM_BATCH_CACHE_BYTES": str(budget)})
    want = expected(sizes, budget)
    for h in sizes:
        print("%s, budget %d, sizes %s: (entries, bytes, loads, evictions) per step %s" % (h, budget, sizes[h], got["steps"][h]))
        assert got["steps"][h] == [w[0] for w in want[h]] and got["kinds"][h] == [w[1] for w in want[h]], h
    kinds = got["kinds"]["garbler"]
    assert kinds == [["load", []], ["load", []], ["hit", []], ["load", []], ["hit", []], ["load", [1, 2]], ["load", [0]],
                     ["load", [3]], ["hit", []]]
    assert [s[0] for s in got["steps"]["garbler"]] == [1, 2, 2, 3, 3, 2, 2, 2, 2]
    assert got["steps"]["garbler"][-1][2:] == [6, 4]


def test_every_step_evicts_under_a_budget_of_one_byte():
    """GC_STREAM_BATCH_CACHE_BYTES=1: an entry larger than the whole budget is kept alone — entries == 1 after every step,
    evictions == loads - 1, bytes == that entry's size, the oracle's bytes throughout (in the child); the step applied twice
    in a row is a hit the second time"""
    sizes = lru_sizes()
    got = run_child("lru_child(%r)" % (sizes,), {"GC_STREAM_BATCH_CACHE_BYTES": "1"})
    for h in sizes:
        print("%s: (entries, bytes, loads, evictions) per step %s" % (h, got["steps"][h]))
        for k, (entries, nbytes, loads, evictions) in enumerate(got["steps"][h]):
            assert entries == 1 and evictions == loads - 1 and nbytes == sizes[h][bc.LRU_SEQUENCE[k]], (h, k)
        assert [s[2] for s in got["steps"][h]] == [1, 2, 3, 4, 5, 6, 7, 8, 8], h
        assert got["kinds"][h][-1] == ["hit", []]
    assert bc.LRU_SEQUENCE[-1] == bc.LRU_SEQUENCE[-2]


def test_a_refused_step_leaves_the_cache_alone():
    """the step outside the keyed scope of test_step_outside_the_keyed_scope_is_refused_and_the_store_stays after two cached
    steps, on both handles: GC_E_ARG, the four counters as they were (the refusal precedes the budget loop), and the next
    cached step is a hit"""
    S = bc.LRU_SESSIONS
    ctx = engine.Context(0)
    ref = bc.reference("lru", bc.lru_program(), S, 32)
    pair = Pair(ctx, ref, S, 32)
    pair.feed()
    pair.check_step(0), pair.check_step(1)
    c = kg.build("edge_over")
    assert not kg.predict("edge_over", S).keyed
    prim = ref["prim"]
    in_, out_ = [prim[i % len(prim)] for i in range(c.num_inputs)], [900]
    before = pair.sb.cache_stats(), pair.se.cache_stats()
    assert before[0][0] == before[0][2] == 2 and before[0][3] == 0
    snap = pair.snapshot(out_)
    n = engine.stream_batch_step_bytes(c.Gates, c.NumWires, in_, out_)
    d_tmp = engine.DeviceBuffer(ctx, shape=S * stride_for(n) + 16)
    assert "gc_batch_keyed_supported" in refused(pair.sb.garble, c.Gates, c.NumWires, in_, out_, d_tmp, stride_for(n))
    # the evaluator's circuit is what it parses out of the block: inputs are the DISTINCT global wires read, so the block that
    # is outside its scope names one wire per input (none of them is ever set: the block is refused before it is evaluated)
    far = list(range(1000, 1000 + c.num_inputs))
    og = oracle.Stream(ref["keys"][0].tobytes(), drbg("bounds/refused", 16 * (len(far) + 1)), far)
    block = og.garble(c.Gates, c.NumWires, far, out_)
    stride = (len(block) + 3) & ~3
    blocks = np.zeros((S, stride), np.uint8)
    blocks[:, : len(block)] = np.frombuffer(block, np.uint8)
    d_blocks = engine.DeviceBuffer(ctx, data=blocks)
    assert "gc_batch_keyed_supported" in refused(pair.se.circuit, c.NumGates, c.NumWires, max(far) + 1, block, d_blocks, stride,
                                                 pair.d_bad)
    d_tmp.close()
    assert (pair.sb.cache_stats(), pair.se.cache_stats()) == before
    assert pair.same(snap, out_)
    pair.check_step(2)  # c1 again
    after = pair.sb.cache_stats(), pair.se.cache_stats()
    assert after == before
    d_blocks.close(), pair.close()
    ctx.close()


# ---- B4: growth with live labels --------------------------------------------------------------------------------------------


@pytest.mark.parametrize("between", [False, True])
def test_store_grows_with_live_labels_on_both_handles(between):
    """1024 -> 3001 rows at step 2 and, without the calls in between, -> 0x11028 at step 3 (32-bit ids, past the doubling); with
    them, between steps 2 and 3, a gather of never-set ids past the garbler's store reads (0, R) and a set at id 90000 past
    the evaluator's store moves no other wire — those calls then do the growing (the row sequences: tests/test_stream_batch_host
    .py).  Every wire that was ever set equals the oracle's afterwards, on both handles."""
    S, keylen = bc.GROWTH_SESSIONS, bc.GROWTH_KEYLEN
    ctx = engine.Context(0)
    ref = bc.reference("growth", bc.growth_program(), S, keylen)
    pair = Pair(ctx, ref, S, keylen)
    pair.feed()
    pair.check_step(0), pair.check_step(1)
    pair.check_wires(ref["steps"][0][2])  # what step 1 set has survived the growth of step 2
    if between:
        w0 = ref["wires"][ref["prim"][0]]
        r = np.zeros(S, LABEL)
        r["d0"], r["d1"] = w0["l0"]["d0"] ^ w0["l1"]["d0"], w0["l0"]["d1"] ^ w0["l1"]["d1"]
        d_w = engine.DeviceBuffer(ctx, shape=(S, len(bc.GROWTH_GATHER)), dtype=WIRE)
        pair.sb.gather_wires(bc.GROWTH_GATHER, d_w)
        pairs = d_w.numpy()
        for j in range(len(bc.GROWTH_GATHER)):
            assert (pairs[:, j]["l0"] == np.zeros(S, LABEL)).all() and (pairs[:, j]["l1"] == r).all(), j
        lab = np.zeros((S, 1), LABEL)
        lab["d0"], lab["d1"] = np.arange(1, S + 1)[:, None] * 0x0123456789, np.arange(1, S + 1)[:, None] * 0x9876543211
        d_one = engine.DeviceBuffer(ctx, data=lab)
        pair.se.set_wires([bc.GROWTH_SET], d_one)
        assert (pair.se.get(bc.GROWTH_SET) == lab[:, 0]).all()
        for w in (bc.GROWTH_SET - 1, bc.GROWTH_SET + 1, 3001, 0x11000):
            assert (pair.se.get(w) == np.zeros(S, LABEL)).all(), w
        pair.check_wires(ref["steps"][0][2] + ref["steps"][1][2])
        pair.check_inputs()
    pair.check_step(2)
    pair.check_wires(ref["wires"])
    pair.check_inputs()
    if between:
        assert (pair.se.get(bc.GROWTH_SET) == lab[:, 0]).all()
        for w in bc.GROWTH_GATHER:
            got = pair.sb.get(w)
            assert (got["l0"] == np.zeros(S, LABEL)).all() and (got["l1"] == r).all(), w
        d_w.close(), d_one.close()
    pair.close()
    ctx.close()


# ---- B5: the cap ------------------------------------------------------------------------------------------------------------


def cap_child():
    """(runs in a process with GC_STREAM_MAX_WIRES=5000)"""
    S, cap = bc.CAP_SESSIONS, bc.CAP
    assert int(os.environ["GC_STREAM_MAX_WIRES"]) == cap
    ref = bc.reference("cap", bc.cap_program(), S, 32)
    prim = ref["prim"]
    ctx = engine.Context(0)
    said = {}
    # create: a primary input at 4999 is taken, one at 5000 refused
    rnd = rnd_streams("bounds/cap/create", S, len(prim) + 1)
    d_keys, d_rnd = engine.DeviceBuffer(ctx, data=ref["keys"]), engine.DeviceBuffer(ctx, data=rnd)
    sb = engine.StreamBatch(ctx, S, d_keys, 32, d_rnd, prim + [cap - 1])
    got = sb.get(cap - 1)
    for s in range(S):
        assert got[s] == oracle.Stream(ref["keys"][s].tobytes(), rnd[s].tobytes(), prim + [cap - 1]).get(cap - 1), s
    sb.close()
    said["create"] = refused(engine.StreamBatch, ctx, S, d_keys, 32, d_rnd, prim + [cap])
    # the steps: out ids 1500, 2500, 4999 — 1024 -> 2048 -> 4096 -> 5000 rows; every set wire after each growth
    pair = Pair(ctx, ref, S, 32)
    pair.feed()
    set_so_far = []
    for k in range(3):
        c, in_, out_ = ref["steps"][k]
        if k == 2:  # nwires = 5001 is refused, 5000 evaluates
            pair.garble(k)
            snap = pair.snapshot()[1]
            with pytest.raises(engine.EngineError) as err:
                pair.evaluate(k, nwires=cap + 1)
            assert err.value.code == engine.GC_E_ARG
            assert all((a == b).all() for a, b in zip(snap, pair.snapshot()[1]))
            assert max(max(in_), max(out_)) + 1 == cap
        pair.check_step(k)
        set_so_far += out_
        pair.check_wires(set_so_far)
        pair.check_inputs()
    pair.check_wires(ref["wires"])
    # id 5000 in a step's out[], in gather_wires and in set_wires: refused, the stores as they were
    snap = pair.snapshot([cap - 2])
    c, in_, out_ = bc.cap_edge_step(cap)
    n = engine.stream_batch_step_bytes(c.Gates, c.NumWires, in_, out_)
    d_tmp = engine.DeviceBuffer(ctx, shape=S * stride_for(n) + 16)
    said["garble"] = refused(pair.sb.garble, c.Gates, c.NumWires, in_, out_, d_tmp, stride_for(n))
    assert pair.same(snap, [cap - 2])
    d_w = engine.DeviceBuffer(ctx, shape=(S, 2), dtype=WIRE)
    pair.sb.gather_wires([prim[0], cap - 1], d_w)
    pairs = d_w.numpy()
    assert (pairs[:, 0] == ref["wires"][prim[0]]).all() and (pairs[:, 1] == ref["wires"][cap - 1]).all()
    said["gather_wires"] = refused(pair.sb.gather_wires, [prim[0], cap], d_w)
    assert pair.same(snap, [cap - 2])
    lab = np.zeros((S, 2), LABEL)
    lab["d0"], lab["d1"] = np.arange(1, 2 * S + 1).reshape(S, 2) * 0x1111, np.arange(1, 2 * S + 1).reshape(S, 2) * 0x7777
    d_lab = engine.DeviceBuffer(ctx, data=lab)
    said["set_wires"] = refused(pair.se.set_wires, [cap - 2, cap], d_lab)
    assert pair.same(snap, [cap - 2])
    pair.se.set_wires([cap - 2, cap - 1], d_lab)
    assert (pair.se.get(cap - 2) == lab[:, 0]).all() and (pair.se.get(cap - 1) == lab[:, 1]).all()
    pair.check_wires([w for w in ref["wires"] if w != cap - 1])
    for d in (d_tmp, d_w, d_lab, d_keys, d_rnd):
        d.close()
    pair.close()
    ctx.close()
    print(TAG + json.dumps(said))


def test_wire_id_cap():
    """GC_STREAM_MAX_WIRES=5000: id 4999 is taken by create, a step's out[], gather_wires and set_wires, id 5000 refused by each
    with GC_E_ARG and a text that names the call and the switch, the stores as they were; nwires = 5001 is refused by the
    evaluator and 5000 evaluates; the store's doubling is clamped to the cap and every set wire survives each growth"""
    said = run_child("cap_child()", {"GC_STREAM_MAX_WIRES": str(bc.CAP)})
    for call, fn in (("create", "gc_stream_batch_create"), ("garble", "gc_stream_batch_garble"),
                     ("gather_wires", "gc_stream_batch_gather_wires"), ("set_wires", "gc_stream_eval_batch_set_wires")):
        assert fn in said[call] and "GC_STREAM_MAX_WIRES" in said[call], said


# ---- B6: 65 535 sessions ----------------------------------------------------------------------------------------------------


def big_run(ctx, ref, keys, flip=False):
    """both steps of bc.big_program for 65 535 sessions on both handles -> everything they leave: the bytes of either step,
    every program wire of the garbler's store, the evaluator's label of every output"""
    S = bc.MAX_SESSIONS
    pair = Pair(ctx, ref, S, 32, keys=keys)
    pair.feed(from_device=True)
    got = {"bytes": [pair.step(k).copy() for k in range(len(ref["steps"]))]}
    got["wires"] = {w: pair.sb.get(w) for w in ref["wires"]}
    got["ev"] = {o: pair.se.get(o) for o in ref["outs"]}
    if flip:  # one skeleton byte of the last session's block of the last step: counted for that session alone
        at = pair.lead + (S - 1) * pair.stride
        pair.d_out.upload(np.array([got["bytes"][-1][S - 1, 0] ^ 0x01], np.uint8), offset=at)
        bad = pair.evaluate(len(ref["steps"]) - 1)
        assert np.flatnonzero(bad).tolist() == [S - 1], np.flatnonzero(bad)[:10]
    pair.close()
    return got


def test_65535_sessions_and_the_refusal_of_65536():
    """S = 65 535, the most a grid of the serialiser has rows for, and 65 536 refused by both creates.  Two steps (7 bytes; 40
    gates of all five kinds, 1 032 bytes), keys = pool[i % 3].  The oracle, every byte and label, on kg.sample(65535, 64) plus
    sessions 65472..65534 (the last full wave and the ragged last tile of 63); every session against the handle pair whose keys
    are all pool[i % 3] (three such runs, the two layers of tests/test_gpu_batch_keyed_shapes.py), the first of which goes to
    the oracle on its own third of the sample.  d_bad all zero; one flipped skeleton byte in session 65534 is counted there alone.
    Measured on the MI355X: 0.7 s for the whole test, 0.4 s of it the oracle and the first run (the printed line); the handles
    are closed one pair after the other, 1 GiB of store each."""
    t0 = time.perf_counter()
    S = bc.MAX_SESSIONS
    ctx = engine.Context(0)
    pool, keys = kg.pool_keys("stream-batch/bounds/big", S, 32)
    smp = bc.big_oracle_sessions()
    assert set(range(65472, S)) <= set(smp) and set(range(64)) <= set(smp)
    ref = bc.reference("big", bc.big_program(), S, 32, sessions=smp, keys=keys)
    d_keys, d_rnd = engine.DeviceBuffer(ctx, data=keys), engine.DeviceBuffer(ctx, data=ref["rnd"])
    for make in (lambda: engine.StreamBatch(ctx, S + 1, d_keys, 32, d_rnd, ref["prim"]),
                 lambda: engine.StreamEvalBatch(ctx, S + 1, d_keys, 32)):
        with pytest.raises(engine.EngineError) as err:
            make()
        assert err.value.code == engine.GC_E_ARG
    d_keys.close(), d_rnd.close()
    got = big_run(ctx, ref, keys, flip=True)
    t1 = time.perf_counter()

    def against_the_oracle(run, sessions):
        for k in range(len(ref["steps"])):
            for s in sessions:
                assert run["bytes"][k][s].tobytes() == ref["streams"][s][k], (k, s)
        for w in ref["wires"]:
            assert (run["wires"][w][sessions] == ref["wires"][w][sessions]).all(), w
        for o in ref["outs"]:
            assert (run["ev"][o][sessions] == ref["ev"][o][sessions]).all(), o

    against_the_oracle(got, smp)
    for j in range(3):
        one = big_run(ctx, ref, np.ascontiguousarray(np.broadcast_to(pool[j], (S, 32))))
        mine = np.arange(j, S, 3)
        if j == 0:
            against_the_oracle(one, [s for s in smp if s % 3 == 0])
        for k in range(len(ref["steps"])):
            assert (got["bytes"][k][mine] == one["bytes"][k][mine]).all(), (j, k)
        for w in ref["wires"]:
            assert (got["wires"][w][mine] == one["wires"][w][mine]).all(), (j, w)
        for o in ref["outs"]:
            assert (got["ev"][o][mine] == one["ev"][o][mine]).all(), (j, o)
    ctx.close()
    print("65535 sessions: %d against the oracle, all against three one-key runs; first run %.1f s, the test %.1f s"
          % (len(smp), t1 - t0, time.perf_counter() - t0))


# ---- B7: more ids than a grid has rows --------------------------------------------------------------------------------------


def test_more_than_65535_ids_through_the_row_movers():
    """one step of 66 000 inputs and 66 000 outputs (in[] and out[] permutations; its wires in HBM: path 2), S = 3: k_sb_rows
    walks its ids a second time (j += gridDim.y) on the way into the evaluator's batch and out of both batches.  Bytes by
    SHA-256 per session plus the first and last 4 096; every one of the 66 000 output wires of both stores; then a step that
    reads 64 of them, output indices 0, 65534, 65535, 65536 and 65999 among them."""
    S = bc.WIDE_SESSIONS
    prog = bc.wide_program()
    (wide, in1, out1), (_, _, out2) = prog[0]
    ref = bc.reference("wide", prog, S, 32, store=out1 + out2)
    ctx = engine.Context(0)
    dc = engine.DeviceCircuit(ctx, wide)
    b = engine.Batch(dc, S)
    assert not b.lds_wires and b.keyed_path == 2
    b.close(), dc.close()
    pair = Pair(ctx, ref, S, 32)
    pair.feed(from_device=True)
    body = pair.step(0)
    for s in range(S):
        want = ref["streams"][s][0]
        assert hashlib.sha256(body[s].tobytes()).digest() == hashlib.sha256(want).digest(), s
        assert body[s, :4096].tobytes() == want[:4096] and body[s, -4096:].tobytes() == want[-4096:], s
    d_w = engine.DeviceBuffer(ctx, shape=(S, len(out1)), dtype=WIRE)
    pair.sb.gather_wires(out1, d_w)
    have = d_w.numpy()
    want = np.stack([ref["wires"][o] for o in out1], axis=1)
    assert have.shape == want.shape == (S, bc.WIDE_N)
    assert np.flatnonzero((have != want).any(axis=0)).tolist() == []
    ev = np.stack([pair.se.get(o) for o in out1], axis=1)
    assert np.flatnonzero((ev != np.stack([ref["ev"][o] for o in out1], axis=1)).any(axis=0)).tolist() == []
    pair.check_wires([out1[i] for i in bc.WIDE_READ])  # (the garbler's, through get_wire as well)
    pair.check_step(1)
    d_w.close(), pair.close()
    ctx.close()
