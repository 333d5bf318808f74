"""The block parser of gc_stream_eval_batch_circuit (parse_block of stream_batch.cpp restates the one-session evaluator's
instead of sharing it) against hostile bytes: the mutants of tests/hostile_fuzz.mutate over the ten small blocks of
hostile_fuzz.programs(), for S = 3 sessions with distinct keys.

Per program the handle and three oracle.StreamEvals start from the same wire store: every wire below numWires holds a seeded
label per session.  The reference block of a call is the mutant; session s's device block is the mutant with the row bytes that
hostile_fuzz.parse finds in it replaced by seeded bytes of that session for s >= 1.  Required, by return codes alone:

  * ACCEPTED  =>  the oracle accepts every session's block and consumes the same number of bytes, d_bad == 0, and every wire
    the mutant names plus a sample of 32 others equals the oracle's in every session;
  * REFUSED   =>  with the code the one-session gc_stream_eval_circuit (pinned to the oracle by hostile_fuzz.run) answers for the
    same bytes; the oracle refuses or hostile_fuzz.stricter names the reason; the store is what it was; the valid block still
    evaluates to the oracle's labels on the same handle;
  * a mutant the parser takes but whose circuit is outside gc_batch_keyed_supported is GC_E_ARG naming that function: at most
    2 % of the accepted ones (with these small circuits none is expected).

Program (host only) is shared with tests/test_stream_batch_geometry_host.py, which predicts the coverage without a GPU."""
import time

import numpy as np
import pytest

import oracle
from mpc_amd import engine
from mpc_amd.circuit import GATE, LABEL
from tests import hostile_fuzz as hf
from tests import keyed_geometry as kg

pytestmark = pytest.mark.gpu

S, KEYLEN = 3, 32
SEED, PER_PROGRAM = 1, 16  # 160 mutants
KINDS = 11
NSAMPLE = 32


def check_coverage(kinds, accepted, refused):
    assert len(kinds) == KINDS and min(kinds.values()) >= 5, kinds
    assert accepted >= 25 and refused >= 25, (accepted, refused)


class Program:
    """program k of hostile_fuzz.programs(): its valid block per session, the seeded store both sides start from (`model`,
    LABEL [S][numWires], kept equal to what the stores must hold), and one oracle.StreamEval per session that is given a wire
    of the model when a block first names it"""

    def __init__(self, k):
        from tests.test_gpu_stream_batch import rnd_streams
        self.k = k
        self.c, self.in_, self.out_ = hf.programs()[k]
        c = self.c
        self.ng, self.ntmp, self.nw = c.NumGates, c.NumWires, max(max(self.in_), max(self.out_)) + 1
        self.wires = sorted(set(self.in_) | set(self.out_))
        prim = sorted(set(self.in_))
        self.keys = kg.edge_keys("stream-batch/hostile", S, KEYLEN)
        rnd = rnd_streams("hostile/%d" % k, S, len(prim))
        self.valid = [oracle.Stream(self.keys[s].tobytes(), rnd[s].tobytes(), prim).garble(c.Gates, c.NumWires, self.in_, self.out_)
                      for s in range(S)]
        assert len({len(v) for v in self.valid}) == 1
        rng = np.random.default_rng([SEED, k, 1])
        self.model = np.zeros((S, self.nw), LABEL)
        self.model["d0"] = rng.integers(1, 1 << 63, (S, self.nw), dtype=np.uint64)
        self.model["d1"] = rng.integers(1, 1 << 63, (S, self.nw), dtype=np.uint64)
        self.sample = sorted(int(w) for w in rng.choice(self.nw, NSAMPLE, replace=False))
        self.oe = [oracle.StreamEval(self.keys[s].tobytes()) for s in range(S)]
        self.known = set()

    def mutants(self):
        rng = np.random.default_rng([SEED, self.k, 2])
        return [hf.mutate(rng, self.valid[0], self.ng) for _ in range(PER_PROGRAM)]

    def session_blocks(self, m, mut, mng):
        """u8 [S][stride]: the mutant, with other row bytes for sessions 1.."""
        stride = max(4, (len(mut) + 3) & ~3)
        blocks = np.zeros((S, stride), np.uint8)
        blocks[:, : len(mut)] = np.frombuffer(mut, np.uint8)
        for s in range(1, S):
            rng = np.random.default_rng([SEED, self.k, 3, m, s])
            for q in hf.parse(mut, mng)[0]:
                blocks[s, q[6]: q[6] + 16 * q[7]] = rng.integers(0, 256, 16 * q[7], dtype=np.uint8)
        return blocks

    def named(self, block, ngates):
        """the global wires below numWires that the block could read or write, with the program's own"""
        ids = set(self.wires)
        for q in hf.parse(block, ngates)[0]:
            ids |= {v for v in q[4] if v < self.nw}
        return sorted(ids)

    def oracle_run(self, blocks, ngates, nbytes=None):
        """every session's block through its oracle.  Returns ([bytes used, None where refused], the named wires); the model
        follows where all accepted, and the oracles are put back to the model where one stopped half-way"""
        nbytes = blocks.shape[1] if nbytes is None else nbytes
        named = self.named(blocks[0, :nbytes].tobytes(), ngates)
        for w in named:
            if w not in self.known:
                self.known.add(w)
                for s in range(S):
                    self.oe[s].set(w, self.model[s, w])
        used = []
        for s in range(S):
            try:
                used.append(self.oe[s].circuit(ngates, self.ntmp, self.nw, blocks[s, :nbytes].tobytes()))
            except oracle.OracleError:
                used.append(None)
        if all(u is not None for u in used):
            for s in range(S):
                for w in named:
                    self.model[s, w] = self.oe[s].get(w)
        else:
            for s in range(S):
                for w in named:
                    self.oe[s].set(w, self.model[s, w])
        return used, named


def forget_last_error():
    """gc_last_error keeps the text of the LAST refusal that wrote one, and the parser's refusals write none: a refusal by
    shape, on the host, puts a known text there, so that the text of the keyed scope after a call is that call's"""
    g = np.zeros(1, GATE)
    g[0] = (0, 1, 2, 0, 0)
    assert engine.stream_batch_step_bytes(g, 3, [0, 1, 5], [2, 3]) == 0
    assert "overlaps" in engine.lib().gc_last_error().decode()


def store_differs(se, prog, ws):
    """the wires among ws on which the handle's store is not the model"""
    return [w for w in ws if (se.get(w) != prog.model[:, w]).any()]


def run_program(ctx, k, stats, kinds):
    prog = Program(k)
    d_keys = engine.DeviceBuffer(ctx, data=prog.keys)
    se = engine.StreamEvalBatch(ctx, S, d_keys, KEYLEN)
    d_model = engine.DeviceBuffer(ctx, data=prog.model)
    se.set_wires(np.arange(prog.nw), d_model)
    one = engine.StreamEval(ctx, prog.keys[0].tobytes())
    d_bad = engine.DeviceBuffer(ctx, shape=S, dtype=np.uint32)
    nvalid = len(prog.valid[0])
    valid = np.zeros((S, (nvalid + 3) & ~3), np.uint8)
    for s in range(S):
        valid[s, :nvalid] = np.frombuffer(prog.valid[s], np.uint8)
    d_valid = engine.DeviceBuffer(ctx, data=valid)

    def valid_block(tag):
        used, named = prog.oracle_run(valid, prog.ng, nvalid)
        assert used == [nvalid] * S
        assert se.circuit(prog.ng, prog.ntmp, prog.nw, prog.valid[0], d_valid, valid.shape[1], d_bad) == nvalid, tag
        assert (d_bad.numpy() == 0).all(), tag
        assert store_differs(se, prog, named + prog.sample) == [], tag

    assert store_differs(se, prog, prog.wires[::7] + prog.sample) == []
    valid_block("program %d: the valid block" % k)
    for m, (mut, mng, what) in enumerate(prog.mutants()):
        tag = "program %d mutant %d (%s)" % (k, m, what)
        kinds[what] = kinds.get(what, 0) + 1
        blocks = prog.session_blocks(m, mut, mng)
        d_blocks = engine.DeviceBuffer(ctx, data=blocks)
        why = hf.stricter(mut, mng, prog.ntmp, prog.nw)
        named = prog.named(mut, mng)
        forget_last_error()
        try:
            used = se.circuit(mng, prog.ntmp, prog.nw, mut, d_blocks, blocks.shape[1], d_bad)
            code = 0
        except engine.EngineError as e:
            code, used = e.code, None
            outside = code == engine.GC_E_ARG and "gc_batch_keyed_supported" in engine.lib().gc_last_error().decode()
        if code == 0:
            stats["accepted"] += 1
            assert why is None, "%s: accepted what the engine refuses by design (%s)" % (tag, why)
            oused, named = prog.oracle_run(blocks, mng, len(mut))  # (the model follows the oracle)
            assert oused == [used] * S, "%s: consumed %d, the oracle %s" % (tag, used, oused)
            assert (d_bad.numpy() == 0).all(), tag
            assert store_differs(se, prog, named + prog.sample) == [], tag
        elif outside:
            stats["outside"] += 1
            assert why is None and all(u is not None for u in prog.oracle_run(blocks, mng, len(mut))[0]), tag
            # (the oracles went on: the handle's store did not)
            labels = np.ascontiguousarray(prog.model[:, named])
            se.set_wires(named, engine.DeviceBuffer(ctx, data=labels))
        else:
            stats["refused"] += 1
            for w in named:
                one.set(w, prog.model[0, w])
            with pytest.raises(engine.EngineError) as alone:
                one.circuit(mng, prog.ntmp, prog.nw, mut)
            assert code == alone.value.code, "%s: %d, the one-session evaluator %d" % (tag, code, alone.value.code)
            assert why or None in prog.oracle_run(blocks, mng, len(mut))[0], "%s: refused (%d) what the reference's loop walks" % (tag, code)
            assert store_differs(se, prog, named + prog.sample) == [], "%s: a refused block changed the store" % tag
            valid_block("the valid block after " + tag)
        d_blocks.close()
    one.close(), se.close()
    for d in (d_keys, d_model, d_bad, d_valid):
        d.close()


def test_mutants_of_the_ten_small_blocks():
    """160 mutants, 16 per program, seed 1: 60 accepted, 100 refused, none outside the keyed scope.  Measured on an MI355X:
    3.7 s for the whole test (every accepted mutant is a new circuit for the handle: a plan, a device circuit and a batch of
    three instances); the test prints its time."""
    t0 = time.perf_counter()
    ctx = engine.Context(0)
    stats, kinds = {"accepted": 0, "refused": 0, "outside": 0}, {}
    for k in range(len(hf.programs())):
        run_program(ctx, k, stats, kinds)
    ctx.close()
    print("hostile blocks for %d sessions: %s, by kind %s, %.1f s" % (S, stats, kinds, time.perf_counter() - t0))
    check_coverage(kinds, stats["accepted"], stats["refused"])
    assert stats["outside"] <= 0.02 * stats["accepted"], stats
