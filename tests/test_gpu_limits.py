"""GPU tests of the code around the main kernels that only runs past a size limit or when something is already wrong:

- the decode mismatch guard (k_decode): invalid evaluator labels are counted exactly and decoded as 0xff;
- the movers' loops past their grid clamps: more than 65 535 inputs / outputs (k_select_inputs, k_decode,
  k_gather_rows) and more than 32 768 instances (k_tables_egress, k_tables_ingest, k_slab_be);
- the split level kernels past 2^24 workgroups (split_grid.h), where a 1-D grid is refused;
- the whole-gate level kernels (GC_LEVEL_WHOLE_GATES=1) on levels with hashed gates.

Everything is compared with the oracle (garble / eval_ / tables_serialize) or with the plaintext result."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from mpc_amd import engine
from mpc_amd.circuit import AND, GATE, INV, LABEL, OR, WIRE, XNOR, XOR, Circuit, bitwise, synthetic_levelised

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = bytes(range(32))


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


def rnd_bytes(c, seed, batch):
    """the garbler's random stream (R and input labels of every instance); numpy, as the batches here are large"""
    return np.random.default_rng(seed).bytes(16 * (c.num_inputs + 1) * batch)


def oracle_instance(c, rnd, i, key=KEY):
    stride = 16 * (c.num_inputs + 1)
    return oracle.garble(c.Gates, c.NumWires, c.num_inputs, key, rnd[i * stride:(i + 1) * stride])


def oracle_outputs(c, ref, inputs, key=KEY):
    """Circuit.Eval of one instance from its input labels: the output labels"""
    w = np.zeros(c.NumWires, LABEL)
    w[: c.num_inputs] = inputs
    oracle.eval_(c.Gates, c.NumWires, key, w, ref["slab"])
    return w[c.NumWires - c.num_outputs:]


def plaintext(c, bits):
    """computer.go:42-88 over a batch: bits [batch][ninputs] -> output bits [batch][noutputs]"""
    wires = np.zeros((bits.shape[0], c.NumWires), np.uint8)
    wires[:, : c.num_inputs] = bits
    for i0, i1, out, op in zip(c.Gates["in0"].tolist(), c.Gates["in1"].tolist(), c.Gates["out"].tolist(), c.Gates["op"].tolist()):
        a, b = wires[:, i0], wires[:, i1]
        wires[:, out] = {XOR: a ^ b, XNOR: a ^ b ^ 1, AND: a & b, OR: a | b, INV: a ^ 1}[op]
    return wires[:, c.NumWires - c.num_outputs:]


def batches(dc, batch, schedule):
    gb, ev = engine.Batch(dc, batch), engine.Batch(dc, batch)
    gb.set_schedule(schedule)
    ev.set_schedule(schedule)
    return gb, ev


# ---- A. the decode guard ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("schedule", [0, 1])
def test_decode_counts_invalid_labels_exactly(ctx, schedule):
    """bitwise(300, AND): output j depends on inputs j and 300 + j only.  Random labels in place of the garbler's for a
    set of (instance, input) pairs, on both sides of the 256-instance block boundary: *mismatch counts every distinct
    (instance, output) they reach, exactly those bytes decode as 0xff, every other byte is the plaintext bit — with and
    without a counter.  The evaluated labels are the oracle's Eval of the same (partly invalid) inputs."""
    n, batch = 300, 300
    c = bitwise(n, AND)
    nin = c.num_inputs
    dc = engine.DeviceCircuit(ctx, c)
    gb, ev = batches(dc, batch, schedule)
    rnd = rnd_bytes(c, 11 + schedule, batch)
    gb.garble(KEY, ctx.to_device(rnd))
    d_w = ctx.zeros(batch * nin * WIRE.itemsize)
    gb.gather_input_wires(0, nin, d_w)
    wires = d_w.download(WIRE, (batch, nin))
    rng = np.random.default_rng(12)
    bits = rng.integers(0, 2, (batch, nin), np.uint8)
    labels = np.where(bits.astype(bool), wires["l1"], wires["l0"])
    hits = [(0, 0), (0, n), (5, 7), (5, n + 7), (17, n + 42), (255, n - 1), (256, 0), (256, 1), (257, 2 * n - 1),
            (299, 150), (299, n + 151)]
    junk = np.frombuffer(rng.bytes(16 * len(hits)), LABEL)
    for (i, j), lab in zip(hits, junk):
        assert lab != wires[i, j]["l0"] and lab != wires[i, j]["l1"]
        labels[i, j] = lab
    bad = sorted({(i, j % n) for i, j in hits})
    assert len(bad) == 9  # (0, 0) and (5, 7) are hit through both inputs
    ev.set_inputs(ctx.to_device(labels))
    ev.eval(KEY, gb)
    d_bits = ctx.zeros((batch, n))
    d_mis = ctx.zeros(1, np.uint32)
    gb.decode(ev, d_bits, d_mis)
    want = plaintext(c, bits)
    for i, j in bad:
        want[i, j] = 0xFF
    assert int(d_mis.numpy()[0]) == len(bad)
    assert (d_bits.numpy() == want).all()
    # a second decode adds to the counter; one without a counter decodes the same bytes
    gb.decode(ev, d_bits, d_mis)
    assert int(d_mis.numpy()[0]) == 2 * len(bad)
    d_bits2 = ctx.zeros((batch, n)).zero(0x55)
    gb.decode(ev, d_bits2, None)
    assert (d_bits2.numpy() == want).all()
    # what the evaluator computed from those labels is the oracle's Eval, valid or not
    outs, R = ev.read_outputs(), gb.read_r()
    for i in (0, 5, 100, 255, 256, 299):
        ref = oracle_instance(c, rnd, i)
        assert R[i] == ref["R"] and (wires[i] == ref["wires"][:nin]).all()
        assert (outs[i] == oracle_outputs(c, ref, labels[i])).all(), "instance %d" % i
    gb.close(); ev.close(); dc.close()


# ---- B. the movers past their grid clamps ----------------------------------------------------------------------------


@pytest.fixture(scope="module")
def wide_circ():
    return bitwise(65600, AND)  # 131 200 inputs, 65 600 outputs


@pytest.mark.parametrize("schedule", [0, 1])
def test_movers_past_65535_inputs_and_outputs(ctx, wide_circ, schedule):
    """k_select_inputs / k_decode / k_gather_rows clamp grid.y at 65 535 and loop over the rest: garble -> select_inputs ->
    eval -> decode of 131 200 inputs and 65 600 outputs is the plaintext result with no mismatch, and the output labels
    (gather_outputs, read_outputs) are the oracle's at outputs 0, 65 534, 65 535, 65 536 and the last one."""
    c, n = wide_circ, wide_circ.num_outputs
    nin = c.num_inputs
    dc = engine.DeviceCircuit(ctx, c)
    for batch in (3, 70):
        gb, ev = batches(dc, batch, schedule)
        rnd = rnd_bytes(c, 21 + batch, batch)
        gb.garble(KEY, ctx.to_device(rnd))
        bits = np.random.default_rng(22 + batch).integers(0, 2, (batch, nin), np.uint8)
        ev.select_inputs(gb, ctx.to_device(bits))
        ev.eval(KEY, gb)
        d_out = ctx.zeros((batch, n))
        d_mis = ctx.zeros(1, np.uint32)
        gb.decode(ev, d_out, d_mis)
        assert int(d_mis.numpy()[0]) == 0
        assert (d_out.numpy() == plaintext(c, bits)).all()
        outs, gouts = ev.read_outputs(), gb.read_outputs()
        stride = ev.stride  # of the schedule-0 / tiled layout this batch has now
        assert stride == gb.stride and stride >= batch
        if schedule == 0:
            assert stride == (batch + 63) & ~63
        d_rows = ctx.zeros(n * stride * LABEL.itemsize)  # gather_outputs writes [noutputs][stride]
        ev.gather_outputs(d_rows)
        cols = [0, 65534, 65535, 65536, n - 1]
        rows = {j: d_rows.download(LABEL, (stride,), offset=j * stride * LABEL.itemsize) for j in cols}
        for j in cols:
            assert (rows[j][batch:] == np.zeros(1, LABEL)).all(), "padding of output row %d" % j
        for i in sorted({0, 1, batch // 2, batch - 1}):
            ref = oracle_instance(c, rnd, i)
            want = oracle_outputs(c, ref, np.where(bits[i].astype(bool), ref["wires"]["l1"][:nin], ref["wires"]["l0"][:nin]))
            assert (outs[i] == want).all(), "instance %d" % i
            assert (gouts[i] == ref["wires"]["l0"][c.NumWires - n:]).all(), "garbler outputs of instance %d" % i
            for j in cols:
                assert rows[j][i] == want[j], "gather_outputs: instance %d output %d" % (i, j)
        gb.close(); ev.close()
    dc.close()


def every_gate_type():
    return synthetic_levelised(3, 24, 0.3, seed=71, ninputs=16, or_frac=0.15, inv_frac=0.15, xnor_frac=0.1)


def wire_bytes(c, slab):
    """the wire format (garbler.go:69-82) of every instance at once: BE gate count; per gate BE row count and its rows,
    each BE(D0) || BE(D1)"""
    batch, rows = slab.shape
    lab = np.empty((batch, rows, 2), ">u8")
    lab[..., 0], lab[..., 1] = slab["d0"], slab["d1"]
    lab = lab.view(np.uint8).reshape(batch, rows, 16)
    ng = c.NumGates
    out = np.zeros((batch, 4 + 4 * ng + 16 * rows), np.uint8)
    out[:, :4] = np.frombuffer(ng.to_bytes(4, "big"), np.uint8)
    row, off = 0, 4
    for op in c.Gates["op"].tolist():
        k = {AND: 2, OR: 3, INV: 1}.get(op, 0)
        out[:, off:off + 4] = np.frombuffer(k.to_bytes(4, "big"), np.uint8)
        out[:, off + 4:off + 4 + 16 * k] = lab[:, row:row + k].reshape(batch, 16 * k)
        row, off = row + k, off + 4 + 16 * k
    return out, lab.reshape(batch, 16 * rows)


@pytest.mark.parametrize("schedule", [0, 1])
def test_table_movers_past_32768_instances(ctx, schedule):
    """k_tables_egress / k_tables_ingest / k_slab_be clamp grid.y at 32 768 instances and loop over the rest: at
    32 768 + 37 and 2 x 32 768 + 5 instances the egressed bytes (wire format and dense) are the oracle's at instances 0,
    32 767, 32 768, 32 769, 65 535 and the last, and the serialisation of the device slab at every instance; ingest of
    them reproduces the slab; a gate-count header corrupted in one instance >= 32 768 is counted exactly once."""
    c = every_gate_type()
    assert all(c.stats()[k] for k in ("AND", "OR", "INV", "XOR", "XNOR"))
    rows = c.slab_rows()
    dc = engine.DeviceCircuit(ctx, c)
    nbytes = dc.tables_wire_bytes
    stride = (nbytes + 3) & ~3
    for batch in (32768 + 37, 2 * 32768 + 5):
        gb, ev = batches(dc, batch, schedule)
        rnd = rnd_bytes(c, 31 + batch, batch)
        gb.garble(KEY, ctx.to_device(rnd))
        d_wire = ctx.zeros(batch * stride)
        gb.egress_tables(d_wire, stride)
        d_dense = ctx.zeros(batch * 16 * rows)
        gb.egress_tables_dense(d_dense, 16 * rows)
        wire = d_wire.numpy().reshape(batch, stride)
        dense = d_dense.numpy().reshape(batch, 16 * rows)
        slab = gb.read_slab()
        sample = [i for i in (0, 32767, 32768, 32769, 65535, batch - 1) if i < batch]
        for i in sample:
            ref = oracle_instance(c, rnd, i)
            assert (slab[i] == ref["slab"]).all(), "slab of instance %d" % i
            assert wire[i, :nbytes].tobytes() == oracle.tables_serialize(c.Gates, ref["slab"]), "egress of instance %d" % i
            assert dense[i].tobytes() == b"".join(oracle.label_to_bytes(l) for l in ref["slab"]), "dense of instance %d" % i
        want_wire, want_dense = wire_bytes(c, slab)
        assert (wire[:, :nbytes] == want_wire).all()
        assert (dense == want_dense).all()
        zeros = np.zeros((batch, rows), LABEL)
        d_bad = ctx.zeros(1, np.uint32)
        ev.write_slab(zeros)
        ev.ingest_tables(d_wire, stride, d_bad)
        assert int(d_bad.numpy()[0]) == 0
        assert (ev.read_slab() == slab).all()
        ev.write_slab(zeros)
        ev.ingest_tables_dense(d_dense, 16 * rows)
        assert (ev.read_slab() == slab).all()
        # the evaluator's own ingested tables evaluate and decode to the plaintext result
        bits = np.random.default_rng(32 + batch).integers(0, 2, (batch, c.num_inputs), np.uint8)
        ev.select_inputs(gb, ctx.to_device(bits))
        ev.eval(KEY, ev)
        d_out = ctx.zeros((batch, c.num_outputs))
        d_mis = ctx.zeros(1, np.uint32)
        gb.decode(ev, d_out, d_mis)
        assert int(d_mis.numpy()[0]) == 0
        assert (d_out.numpy() == plaintext(c, bits)).all()
        # one corrupted gate count, in an instance past the first 32 768
        w2 = wire.copy()
        w2[batch - 2, 3] ^= 1
        d_bad.zero()
        ev.ingest_tables(ctx.to_device(w2.reshape(-1)), stride, d_bad)
        assert int(d_bad.numpy()[0]) == 1
        gb.close(); ev.close()
    dc.close()


# ---- C. the split level kernels at the old grid limit -----------------------------------------------------------------


def test_split_level_past_2_24_workgroups(ctx):
    """Schedule 0 garbles a level of N = 2^18 + 3 INV gates fanning out of one input at 4 096 instances with the split
    kernel: N x ceil(4 096 / 64) = 2^24 + 192 hash workgroups, past the 2^24 - 1 a 1-D grid may hold (split_grid.h); a
    second level (one more INV) makes run_levels record the pass as a graph.  R and sampled table rows of sampled
    instances are the oracle's.  Peak device memory ~32 GiB (arithmetic, not measured): wire labels
    (N + 2) x 4 096 x 16 B = 16 GiB and table rows (N + 1) x 4 096 x 16 B = 16 GiB.  Takes a few seconds."""
    N, batch = (1 << 18) + 3, 4096
    g = np.zeros(N + 1, GATE)
    g["in0"][:N] = 0
    g["out"][:N] = 1 + np.arange(N)
    g["op"][:N] = INV
    g[N] = (N, 0, N + 1, INV, 0)
    c = Circuit(N + 2, [1], [1], g, "inv_fanout")
    assert N * ((batch + 63) // 64) > (1 << 24) - 1
    dc = engine.DeviceCircuit(ctx, c, schedule=0)
    assert dc.info.nlevels == 2 and dc.info.slab_rows == N + 1
    gb = engine.Batch(dc, batch)
    gb.set_schedule(0)
    assert gb.stride == batch
    rnd = rnd_bytes(c, 41, batch)
    gb.garble(KEY, ctx.to_device(rnd))
    R = gb.read_r()
    # the slab is [row][bstride]: copy whole rows (64 KiB each) out of it on the device, download only those
    row_ids = [0, 1, 255, 256, 1 << 17, N - 2, N - 1, N]
    row_bytes = batch * LABEL.itemsize
    d_rows = ctx.empty(len(row_ids) * row_bytes)
    base = engine.lib().gc_batch_dev_slab(gb.h)
    for k, r in enumerate(row_ids):
        d_rows.copy_from(base + r * row_bytes, row_bytes, offset=k * row_bytes)
    rows = d_rows.download(LABEL, (len(row_ids), batch))
    for i in (0, 1, 63, 64, 2047, 4032, batch - 1):
        ref = oracle_instance(c, rnd, i)
        assert R[i] == ref["R"], "R of instance %d" % i
        for k, r in enumerate(row_ids):
            assert rows[k, i] == ref["slab"][r], "row %d of instance %d" % (r, i)
    d_rows.close()
    gb.close()
    dc.close()
    ctx.sync()


# ---- D. the whole-gate level kernels ----------------------------------------------------------------------------------

WHOLE_GATES_CHILD = r"""
import os, sys
sys.path.insert(0, os.getcwd())
assert os.environ.get("GC_LEVEL_WHOLE_GATES") == "1"
from mpc_amd import engine
from mpc_amd.circuit import parse_file, synthetic_levelised
from tests.test_gpu_garble_eval import KEY128, KEY256, check_garble_eval
ctx = engine.Context(0)
c = synthetic_levelised(10, 48, 0.3, seed=5, ninputs=40, or_frac=0.1, inv_frac=0.1, xnor_frac=0.1)
for batch in (1, 5, 32, 33, 257, 1030):  # lg < 6 (UNIFORM = false) up to 32 instances, lg >= 6 from 33
    check_garble_eval(ctx, c, KEY256, batch, "whole%d" % batch, schedule=0)
ck = synthetic_levelised(6, 70, 0.4, seed=9, ninputs=32, or_frac=0.1, inv_frac=0.1, xnor_frac=0.1)
for key in (KEY128, bytes(range(7, 31)), KEY256):
    check_garble_eval(ctx, ck, key, 70, "wholekey%d" % len(key), schedule=0)
check_garble_eval(ctx, parse_file(os.path.join("tests", "golden", "aes_128.gcf")), KEY256, 6, "wholeaes", schedule=0)
ctx.close()
print("whole-gate level kernels ok")
"""


def test_whole_gate_level_kernels():
    """GC_LEVEL_WHOLE_GATES=1 (read once per process, so in one child process): schedule 0 runs k_garble_level /
    k_eval_level on the levels with AND, OR and INV gates; garble and eval are the oracle's on every gate type at batches
    1, 5, 32 (UNIFORM = false) and 33, 257, 1 030 (UNIFORM = true), with the three key sizes, and on aes_128 x 6.
    Takes a few seconds."""
    env = dict(os.environ, GC_LEVEL_WHOLE_GATES="1")
    args = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", WHOLE_GATES_CHILD]
    r = subprocess.run(args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "child exit status %d\n%s\n%s" % (r.returncode, r.stdout[-4000:], r.stderr[-4000:])
    assert "whole-gate level kernels ok" in r.stdout
