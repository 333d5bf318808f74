"""k_sb_serialise and k_sb_ingest (the 4096-byte pieces built in LDS around the keyed batch pass of gc_stream_batch_garble /
gc_stream_eval_batch_circuit) at the piece edges: the steps of tests/stream_batch_cases.py — table rows that straddle a piece
boundary by every 1..15 bytes, end on one and start on one, with both id widths; steps of 4096 + t bytes and of two pieces
exactly; a step shorter than one 16-byte line; a step without a row — at every alignment of a session's bytes in device memory.

Every byte of every session is compared with the oracle's Streaming.Garble, every label with its StreamEvaluator, and d_bad with
the NUMBER of tampered structure bytes worked out on the host from hostile_fuzz.parse.  The geometry the cases claim is asserted
without a GPU by tests/test_stream_batch_geometry_host.py."""
import numpy as np
import pytest

import oracle
from mpc_amd import engine
from tests import hostile_fuzz as hf
from tests import stream_batch_cases as sc
from tests.test_gpu_stream_batch import FILL, Run, active_labels, check_store, eval_step

pytestmark = pytest.mark.gpu

KEYLEN = 32


class RunAt(Run):
    """Run with the distance between two sessions' streams given: the garbler's side of a one-step program on the device"""

    def __init__(self, ctx, ref, S, stride, lead):
        self.ref, self.S, self.stride, self.lead = ref, S, stride, lead
        self.total = len(ref["streams"][0][0])
        assert stride % 4 == 0 and stride >= self.total
        self.d_keys = engine.DeviceBuffer(ctx, data=ref["keys"])
        self.d_rnd = engine.DeviceBuffer(ctx, data=ref["rnd"])
        self.d_out = engine.DeviceBuffer(ctx, data=np.full(lead + S * stride + 16, FILL, np.uint8))
        self.sb = engine.StreamBatch(ctx, S, self.d_keys, KEYLEN, self.d_rnd, ref["prim"])
        c, in_, out_ = ref["steps"][0]
        assert self.sb.garble(c.Gates, c.NumWires, in_, out_, self.d_out + lead, stride) == self.total
        self.offs = [0]
        self.buf = self.d_out.numpy()

    def starts(self):
        """the low four address bits of every session's first byte"""
        return [(self.d_out.ptr + self.lead + s * self.stride) & 15 for s in range(self.S)]


def stride_mod16(total, r):
    """the smallest stride >= total that is r mod 16"""
    return total + (r - total) % 16


def alignments(ctx, name, S=5):
    """the case garbled five times: a stride = 4 mod 16 at lead 0, 1, 2, 3 — five sessions 4 bytes apart mod 16, times four leads:
    every one of the sixteen alignments — and a stride that is a multiple of 16 at lead 7"""
    ref = sc.reference(name, S)
    total = len(ref["streams"][0][0])
    seen = set()
    for lead in range(4):
        run = RunAt(ctx, ref, S, stride_mod16(total, 4), lead)
        seen |= set(run.starts())
        yield ref, run
        run.close()
    assert seen == set(range(16))
    run = RunAt(ctx, ref, S, stride_mod16(total, 0), 7)
    assert set(run.starts()) == {(run.d_out.ptr + 7) & 15} and run.stride % 16 == 0
    yield ref, run
    run.close()


@pytest.mark.parametrize("name", sc.NAMES)
def test_serialiser_at_every_alignment(name):
    ctx = engine.Context(0)
    for ref, run in alignments(ctx, name):
        tag = "lead %d, stride %d" % (run.lead, run.stride)
        for s in range(run.S):
            assert run.session(s) == ref["streams"][s][0], "session %d, %s" % (s, tag)
        assert run.untouched(), tag
        check_store(run.sb, ref)
    ctx.close()


def check_labels(se, ref, sessions, tag=""):
    for o in ref["outs"]:
        got = se.get(o)
        for s in sessions:
            assert (int(got[s]["d0"]), int(got[s]["d1"])) == ref["ev"][o][s], "wire %d of session %d %s" % (o, s, tag)


def evaluator(ctx, ref, run, S):
    se = engine.StreamEvalBatch(ctx, S, run.d_keys, KEYLEN)
    se.set_wires(ref["prim"], engine.DeviceBuffer(ctx, data=active_labels(ref, S)))
    return se


@pytest.mark.parametrize("name", sc.NAMES)
def test_ingester_reads_clean_blocks_at_every_alignment(name):
    """the garbler's device buffer in place; d_bad holds 0xFFFFFFFF before the call, which owns the reset"""
    ctx = engine.Context(0)
    d_bad = engine.DeviceBuffer(ctx, shape=5, dtype=np.uint32)
    for ref, run in alignments(ctx, name):
        tag = "lead %d, stride %d" % (run.lead, run.stride)
        se = evaluator(ctx, ref, run, run.S)
        d_bad.zero(0xFF)
        assert (d_bad.numpy() == 0xFFFFFFFF).all()
        block = ref["streams"][run.S // 2][0]
        assert eval_step(se, ref, 0, block, run.d_out + run.lead, run.stride, d_bad) == len(block), tag
        assert (d_bad.numpy() == 0).all(), tag
        check_labels(se, ref, range(run.S), tag)
        se.close()
    ctx.close()


def flip(block, at, rng):
    block[at] ^= 1 << int(rng.integers(0, 8))


@pytest.mark.parametrize("name", ["straddle", "straddle_long"] + sc.TAIL_CASES)
def test_ingester_counts_exactly_the_tampered_structure_bytes(name):
    """session 1: every byte outside the rows inverted; 2: every row byte changed; 3: single bits in the first and last structure
    byte of every piece, the last byte of the step, the four bytes of one aligned word and the structure bytes next to every
    straddling row; 4: the two bytes of every straddling row on either side of its boundary; 0 and 5 untouched.  (The steps of
    4096 + t bytes end in three XORs, so their one boundary lies in structure: no row straddles it and session 4 stays as it
    is; tail2x has one such row, the straddle cases fifteen.)"""
    S = 6
    ctx = engine.Context(0)
    ref = sc.reference(name, S)
    c, in_, out_ = ref["steps"][0]
    n = len(ref["streams"][0][0])
    run = RunAt(ctx, ref, S, stride_mod16(n, 4), 0)
    parsed, err = hf.parse(ref["streams"][0][0], c.NumGates)
    assert err is None
    isrow = sc.row_mask(parsed, n)
    structure = np.flatnonzero(~isrow)
    strad = sc.straddlers(parsed, n)
    assert strad or not name.startswith("straddle")
    rng = np.random.default_rng(len(name) + n)
    blocks = run.buf[: S * run.stride].reshape(S, run.stride).copy()
    for s in range(S):
        assert blocks[s, :n].tobytes() == ref["streams"][s][0]
    blocks[1, :n][~isrow] ^= 0xFF
    blocks[2, :n][isrow] ^= rng.integers(1, 256, int(isrow.sum()), dtype=np.uint8)
    flipped = {n - 1}
    for lo in range(0, n, sc.PIECE):
        mine = structure[(structure >= lo) & (structure < lo + sc.PIECE)]
        flipped |= {int(mine[0]), int(mine[-1])}
    word = next(k for k in range(n // 8, n // 4) if not isrow[4 * k: 4 * k + 4].any())
    flipped |= set(range(4 * word, 4 * word + 4))
    for off, b in strad:
        flipped |= {int(structure[structure < off][-1]), int(structure[structure >= off + 16][0])}
    assert not isrow[sorted(flipped)].any()
    for at in sorted(flipped):
        flip(blocks[3], at, rng)
    for off, b in strad:
        flip(blocks[4], b - 1, rng), flip(blocks[4], b, rng)
        assert isrow[b - 1] and isrow[b]
    want_bad = [0, int((~isrow).sum()), 0, len(flipped), 0, 0]
    print("%s: %d bytes, %d outside the rows, %d single structure bytes flipped, %d straddling rows" % (
        name, n, want_bad[1], want_bad[3], len(strad)))
    d_blocks = engine.DeviceBuffer(ctx, data=blocks)
    se = evaluator(ctx, ref, run, S)
    d_bad = engine.DeviceBuffer(ctx, shape=S, dtype=np.uint32)
    d_bad.zero(0xFF)
    assert eval_step(se, ref, 0, ref["streams"][0][0], d_blocks, run.stride, d_bad) == n
    assert d_bad.numpy().tolist() == want_bad
    # sessions whose rows are their own: the honest labels — the structure is the reference block's
    check_labels(se, ref, (0, 1, 3, 5))
    # changed rows are evaluated as they are: what StreamEvaluator computes from the tampered bytes
    lab = active_labels(ref, S)
    for s in (2, 4):
        oe = oracle.StreamEval(ref["keys"][s].tobytes())
        for j, w in enumerate(ref["prim"]):
            oe.set(w, lab[s, j])
        assert oe.circuit(c.NumGates, c.NumWires, max(max(in_), max(out_)) + 1, blocks[s, :n].tobytes()) == n
        for o in out_:
            got = se.get(o)
            assert (int(got[s]["d0"]), int(got[s]["d1"])) == oe.get(o), (o, s)
    se.close(), run.close()
    ctx.close()


def test_straddle_for_67_sessions():
    """a ragged wave on the movers between store and batch; every session byte for byte, through garbler and evaluator"""
    S = 67
    ctx = engine.Context(0)
    ref = sc.reference("straddle", S)
    c, _, _ = ref["steps"][0]
    dc = engine.DeviceCircuit(ctx, c)
    b = engine.Batch(dc, S)
    assert b.keyed_path == sc.PATH["straddle"]
    b.close(), dc.close()
    n = len(ref["streams"][0][0])
    run = RunAt(ctx, ref, S, stride_mod16(n, 12), 5)
    for s in range(S):
        assert run.session(s) == ref["streams"][s][0], "session %d" % s
    assert run.untouched()
    check_store(run.sb, ref)
    se = evaluator(ctx, ref, run, S)
    d_bad = engine.DeviceBuffer(ctx, shape=S, dtype=np.uint32)
    d_bad.zero(0xFF)
    assert eval_step(se, ref, 0, ref["streams"][S - 1][0], run.d_out + run.lead, run.stride, d_bad) == n
    assert (d_bad.numpy() == 0).all()
    check_labels(se, ref, range(S))
    se.close(), run.close()
    ctx.close()
