"""S sessions of one streamed program per call (gc_stream_batch_* / gc_stream_eval_batch_*) beside what the same caller had
before: S one-session gc_streams on one ctx, one after the other.  Program: ed25519like1 of scripts/bench_stream.py (2 605
steps, 10.4 M gates per session), 32-byte keys, S = 64, 256 and 1 024; one JSON line per S.

Method (scripts/bench_batch_keyed.py, bench.py): all forms alternate in one process.  One untimed pass of each first — it loads
and plans the circuits and brings the card to its sustained clocks — then --reps rounds; a window is one whole pass of the
program between two gc_ctx_sync, timed by the host clock; the median of the rounds is reported with every round beside it.

  batch garble        every step through gc_stream_batch_garble.  Every step's bytes go to the SAME device buffer (S x the
                      largest step): the whole streams of 1 024 sessions are 234 GB, and a host drains them as they come.
  batch garble+eval   step k garbled, then evaluated out of that buffer by gc_stream_eval_batch_circuit on the same ctx stream
                      (the reference block of a step is any session's bytes: the one-session run's); eval = this minus garble
  baseline            --sample one-session gc_streams (gc_stream_garble_begin_h / _finish_async at bench_stream.py's window,
                      then gc_stream_eval_circuit over the bytes), run one after the other and scaled to S sessions

--kernel-stats CSV adds the split of the device time of a pass from a `rocprofv3 --kernel-trace --stats` run of `--once S` (a
run of its own: one garble+eval pass and nothing else): keyed pass (k_garble_flat_keyed / k_eval_flat_keyed + k_expand_keys),
movers (k_gather, k_sb_rnd_form, k_sb_rows), serialiser (k_sb_serialise) and ingester (k_sb_ingest), and the serialiser's and
ingester's bytes per second against 8 TB/s.

--program big130_16: a program of WIDE steps instead — the first 16 steps of bench_stream.py's big130 (131 072 gates per step,
64 levels of 2 048, four circuits in turn), whose circuits keep their wires in HBM and take the keyed HBM-wire kernels
(k_garble_hbm_keyed / k_eval_hbm_keyed); the parent refused them.  Its four batches are larger than the default cache of a
handle together, so the run raises GC_STREAM_BATCH_CACHE_BYTES to 16 GiB unless the caller set it.

--egress: the way of the garbler's bytes to HOST memory instead, one JSON line per S.  Windows of 1 MiB per
session; four forms alternate after an untimed pass of each, a window is one whole pass between two gc_ctx_sync:
  (a) device   today's device-only pass above: the reused buffer, nothing leaves
  (b) sync     what a host had before gc_stream_batch_out_*: the steps appended in a device window [S][1 MiB], and a synchronous
               gc_dev_download of the window into pinned memory whenever the next step does not fit
  (c) windows  gc_stream_batch_out_* with three windows, a 20-byte prefix per step and a consumer thread that only releases
  copy         (b)'s downloads alone, no garbling: the link
The criterion: all (c) windows below all (b) windows.  GC_STREAM_BATCH_OUT_WHOLE_ROWS=1 in the environment makes (c) copy whole
windows in one piece instead of the used columns.

--egress --split: today's window handle beside the split handle (gc_stream_batch_out_create_split), one JSON line
per (S, --windows).  Windows of 1 MiB per session; the two handles alternate after an untimed pass of each with the consumer
thread of (c); per form the time, the bytes the handle pins (the unsplit handle's windows grow to the step: its sizes are
worked out from the rule of stream_batch_windows.h), `grown` and `sealed`.  With --program big130_16 every step exceeds the window.
--split-once S runs three passes of each form and nothing else: the run a kernel trace is taken of.

--intake: the evaluator driven from the garbler's windows, one JSON line per S.  The program is garbled ONCE
through gc_stream_batch_out_* behind real OpCircuit headers, windows of 1 MiB per session, and every window is kept in pinned
memory.  Two forms alternate after an untimed pass of each, which also checks that both leave the same store
(gc_stream_eval_batch_return_labels of the program's last outputs); a window is one whole pass between two gc_ctx_sync:
  (a) per step  the header read on the host from session 0, one gc_stream_eval_batch_circuit_host per step
  (b) intake    one gc_stream_eval_batch_in_feed per window
--intake-once S runs one pass of (b) and nothing else timed: the run a kernel trace is taken of."""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mpc_amd import engine  # noqa: E402
from scripts import bench_stream as bs  # noqa: E402

PROGRAM = "ed25519like1"
PROGRAMS = dict(bs.PROGRAMS, big130_16=lambda: bs.program_big(16 * 131072))
HBM_BYTES_PER_S = 8e12


class Program:
    """the steps with their ctypes arguments converted once, their byte counts and (from a one-session run) a reference block
    per step"""

    def __init__(self, max_steps=None):
        self.steps, self.prim = PROGRAMS[PROGRAM]()
        if max_steps:
            self.steps = self.steps[:max_steps]
        self.args = bs._Args(self.steps)
        self.gates = sum(c.NumGates for c, _, _ in self.steps)
        self.sizes = [engine.stream_batch_step_bytes(c.Gates, c.NumWires, i, o) for c, i, o in self.steps]
        assert all(self.sizes)
        self.bytes = sum(self.sizes)
        self.stride = (max(self.sizes) + 15) & ~15
        self.window = bs.WINDOWS.get(PROGRAM, 64)
        self.eval_args = [(c.NumGates, c.NumWires, max(max(i), max(o)) + 1) for c, i, o in self.steps]


def one_session(ctx, prog, key, rnd, evaluate=True):
    """(garble seconds, eval seconds, stream bytes, sizes) of one gc_stream / gc_stream_eval over the program"""
    stream, sizes, dt, _, g = bs.garble_program(ctx, key, prog.steps, prog.prim, rnd, prog.window)
    de = bs.eval_program(ctx, key, prog.steps, prog.prim, g, stream, sizes)[0] if evaluate else 0.0
    g.close()
    return dt, de, stream, sizes


class Batch:
    def __init__(self, ctx, prog, S, ref_stream):
        self.ctx, self.prog, self.S = ctx, prog, S
        rng = np.random.default_rng(S)
        self.keys = rng.integers(0, 256, (S, 32), dtype=np.uint8)
        self.d_keys = engine.DeviceBuffer(ctx, data=self.keys)
        rnd = rng.integers(0, 256, (S, 1 + len(prog.prim), 16), dtype=np.uint8)
        self.d_rnd = engine.DeviceBuffer(ctx, data=rnd)
        self.d_buf = engine.DeviceBuffer(ctx, shape=S * prog.stride)
        self.d_bad = engine.DeviceBuffer(ctx, shape=S, dtype=np.uint32)
        self.sb = engine.StreamBatch(ctx, S, self.d_keys, 32, self.d_rnd, prog.prim)
        self.se = engine.StreamEvalBatch(ctx, S, self.d_keys, 32)
        # all-zero inputs: the evaluator's active labels are the garbler's L0s
        d_w = engine.DeviceBuffer(ctx, shape=(S, len(prog.prim)), dtype=engine.WIRE)
        self.sb.gather_wires(prog.prim, d_w)
        self.se.set_wires(prog.prim, engine.DeviceBuffer(ctx, data=np.ascontiguousarray(d_w.numpy()["l0"])))
        offs = np.concatenate([[0], np.cumsum(prog.sizes)]).astype(np.int64)
        self.refs = [np.ascontiguousarray(ref_stream[offs[k]: offs[k + 1]]) for k in range(len(prog.steps))]
        self.n = C.c_size_t(0)

    def run(self, evaluate):
        L, pn, h, e = engine.lib(), C.byref(self.n), self.sb.h, self.se.h
        buf, bad, stride = C.c_void_p(self.d_buf.ptr), C.c_void_p(self.d_bad.ptr), self.prog.stride
        garble, circuit = L.gc_stream_batch_garble, L.gc_stream_eval_batch_circuit
        for k, b in enumerate(self.prog.args.begin):
            rc = garble(h, *b, buf, stride, pn)
            if rc:
                raise engine.EngineError(rc, "gc_stream_batch_garble(step %d)" % k)
            if evaluate:
                a, r = self.prog.eval_args[k], self.refs[k]
                rc = circuit(e, a[0], a[1], a[2], r.ctypes.data_as(C.c_void_p), len(r), buf, stride, bad, pn)
                if rc:
                    raise engine.EngineError(rc, "gc_stream_eval_batch_circuit(step %d)" % k)

    def window(self, evaluate):
        self.ctx.sync()
        t0 = time.perf_counter()
        self.run(evaluate)
        self.ctx.sync()
        return time.perf_counter() - t0

    def check(self):
        """the evaluator's labels of the last outputs are the garbler's L0 or L1 in every session, no block differed"""
        assert (self.d_bad.numpy() == 0).all()
        for o in self.prog.steps[-1][2][:4]:
            got, wire = self.se.get(o), self.sb.get(o)
            assert ((got == wire["l0"]) | (got == wire["l1"])).all(), o

    def close(self):
        self.sb.close()
        self.se.close()


def measure(ctx, prog, S, reps, sample):
    key0 = bytes(range(32))
    rnd0 = bs.stream_rnd(PROGRAM, len(prog.prim))
    _, _, ref_stream, _ = one_session(ctx, prog, key0, rnd0)  # (untimed: circuits loaded and planned, clocks up)
    b = Batch(ctx, prog, S, ref_stream)
    b.window(True)
    b.check()
    rng = np.random.default_rng(1)
    singles = [(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, 16 * (len(prog.prim) + 1), dtype=np.uint8).tobytes())
               for _ in range(sample)]
    t = {"garble": [], "garble_eval": [], "base_garble": [], "base_eval": []}
    for _ in range(reps):
        dg = de = 0.0
        for key, rnd in singles:
            a, e, _, _ = one_session(ctx, prog, key, rnd)
            dg, de = dg + a, de + e
        t["base_garble"].append(dg / sample * S)
        t["base_eval"].append(de / sample * S)
        t["garble"].append(b.window(False))
        t["garble_eval"].append(b.window(True))
    b.check()
    med = {k: statistics.median(v) for k, v in t.items()}
    ev = med["garble_eval"] - med["garble"]
    n, total = len(prog.steps), prog.gates * S
    row = {
        "bench": "stream_batch", "program": PROGRAM, "sessions": S, "key_bytes": 32, "steps": n, "gates_per_session": prog.gates,
        "bytes_per_session": prog.bytes, "reps": reps, "baseline_sessions_timed": sample, "baseline_window": prog.window,
        "garble_s": med["garble"], "garble_plus_eval_s": med["garble_eval"], "eval_s": ev,
        "garble_gates_per_s": total / med["garble"], "eval_gates_per_s": total / ev,
        "garble_us_per_step": med["garble"] / n * 1e6, "eval_us_per_step": ev / n * 1e6,
        "baseline_garble_s": med["base_garble"], "baseline_eval_s": med["base_eval"],
        "baseline_garble_gates_per_s": total / med["base_garble"], "baseline_eval_gates_per_s": total / med["base_eval"],
        "garble_speedup": med["base_garble"] / med["garble"], "eval_speedup": med["base_eval"] / ev,
        "seconds_all": t,
    }
    b.close()
    return row


EGRESS_WINDOW = 1 << 20
EGRESS_WINDOWS = 3


class Egress:
    """forms (b), (c) and the copy alone beside a Batch's form (a), on the Batch's garbler handle"""

    def __init__(self, ctx, prog, b):
        import threading
        self.threading = threading
        self.ctx, self.prog, self.b, self.S = ctx, prog, b, b.S
        self.cap = EGRESS_WINDOW
        assert max(prog.sizes) + 20 <= self.cap
        self.d_win = engine.DeviceBuffer(ctx, shape=self.S * self.cap)
        self.pin = engine.PinnedArray(self.S * self.cap, np.uint8)
        self.out = b.sb.out(self.cap, EGRESS_WINDOWS)
        self.prefix = np.arange(20, dtype=np.uint8)
        self.n = C.c_size_t(0)
        # where (b) downloads: before the first step that does not fit behind the ones in the window, and at the end
        self.cuts, at = [], 0
        for k, n in enumerate(prog.sizes):
            if at + n > self.cap:
                self.cuts.append(k)
                at = 0
            at += n
        self.downloads = len(self.cuts) + 1

    def download(self):
        rc = engine.lib().gc_dev_download(self.ctx.h, C.c_void_p(self.pin.ptr), C.c_void_p(self.d_win.ptr), self.S * self.cap)
        if rc:
            raise engine.EngineError(rc, "gc_dev_download")

    def run_sync(self):
        L, pn, h = engine.lib(), C.byref(self.n), self.b.sb.h
        garble, cuts, at = L.gc_stream_batch_garble, set(self.cuts), 0
        for k, a in enumerate(self.prog.args.begin):
            if k in cuts:
                self.download()
                at = 0
            rc = garble(h, *a, C.c_void_p(self.d_win.ptr + at), self.cap, pn)
            if rc:
                raise engine.EngineError(rc, "gc_stream_batch_garble(step %d)" % k)
            at += self.n.value
        self.download()

    def run_copy(self):
        for _ in range(self.downloads):
            self.download()

    def run_windows(self):
        L, pn, h = engine.lib(), C.byref(self.n), self.out.h
        garble, pre = L.gc_stream_batch_out_garble, self.prefix.ctypes.data_as(C.c_void_p)
        flushed, taken = self.threading.Event(), [0]

        def consumer():
            while True:
                last = flushed.is_set()
                if self.out.next() is None:
                    if last:
                        return
                    time.sleep(0.0001)
                    continue
                taken[0] += 1
                self.out.release()

        t = self.threading.Thread(target=consumer)
        t.start()
        try:
            for k, a in enumerate(self.prog.args.begin):
                while True:
                    rc = garble(h, pre, 20, *a, pn)
                    if rc != engine.GC_E_BUSY:
                        break
                    time.sleep(0.00005)  # (no window is free: let the consumer run)
                if rc:
                    raise engine.EngineError(rc, "gc_stream_batch_out_garble(step %d)" % k)
            self.out.flush()
        finally:
            flushed.set()
            t.join()
        return taken[0]

    def window(self, run):
        self.ctx.sync()
        t0 = time.perf_counter()
        run()
        self.ctx.sync()
        return time.perf_counter() - t0

    def close(self):
        self.out.close()
        self.pin.close()
        self.d_win.close()


def egress(ctx, prog, S, reps):
    ref_stream = np.zeros(prog.bytes, np.uint8)  # (the evaluator is not run here)
    b = Batch(ctx, prog, S, ref_stream)
    try:
        e = Egress(ctx, prog, b)
    except engine.EngineError as err:
        b.close()
        return {"bench": "stream_batch_egress", "program": PROGRAM, "sessions": S, "skipped": "windows not allocated: %s" % err}
    forms = {"device": lambda: b.run(False), "sync": e.run_sync, "windows": e.run_windows, "copy": e.run_copy}
    for run in forms.values():
        e.window(run)
    sealed0, busy0 = e.out.stats()[0], e.out.stats()[3]
    t = {k: [] for k in forms}
    for _ in range(reps):
        for k, run in forms.items():
            t[k].append(e.window(run))
    sealed, _, grown, busy = e.out.stats()
    med = {k: statistics.median(v) for k, v in t.items()}
    bound = max(med["device"], med["copy"])
    moved = (prog.bytes + 20 * len(prog.steps)) * S
    row = {
        "bench": "stream_batch_egress", "program": PROGRAM, "sessions": S, "key_bytes": 32, "steps": len(prog.steps),
        "bytes_per_session": prog.bytes, "window_bytes": e.cap, "windows": EGRESS_WINDOWS, "reps": reps,
        "whole_rows": bool(os.environ.get("GC_STREAM_BATCH_OUT_WHOLE_ROWS", "0") not in ("", "0")),
        "device_s": med["device"], "sync_s": med["sync"], "windows_s": med["windows"], "copy_s": med["copy"],
        "copy_bytes_per_s": e.downloads * S * e.cap / med["copy"], "windows_stream_bytes_per_s": moved / med["windows"],
        "windows_below_sync_in_all_rounds": max(t["windows"]) < min(t["sync"]),
        "windows_over_max_device_copy": med["windows"] / bound, "sync_over_device_plus_copy": med["sync"] / (med["device"] + med["copy"]),
        "pinned_bytes_of_the_handle": EGRESS_WINDOWS * S * e.cap, "windows_sealed_per_pass": (sealed - sealed0) / reps,
        "sync_downloads_per_pass": e.downloads, "grown": grown, "busy_answers_per_pass": (busy - busy0) / reps, "seconds_all": t,
    }
    e.close()
    b.close()
    return row


class SplitEgress:
    """today's window handle and the split handle on one Batch's garbler, each drained by a consumer thread that only releases"""

    def __init__(self, ctx, prog, b, nwindows):
        import threading
        self.threading = threading
        self.ctx, self.prog, self.b, self.S, self.cap, self.nwindows = ctx, prog, b, b.S, EGRESS_WINDOW, nwindows
        if max(prog.sizes) + 20 > (nwindows - 1) * self.cap:
            raise engine.EngineError(engine.GC_E_ARG, "a step of %d bytes needs more than %d windows" % (max(prog.sizes) + 20, nwindows))
        self.out = {"windows": b.sb.out(self.cap, nwindows), "split": b.sb.out(self.cap, nwindows, split=True)}
        self.prefix = np.arange(20, dtype=np.uint8)
        self.n = C.c_size_t(0)

    def unsplit_pinned_bytes(self):
        """what the unsplit handle pins after a pass: an empty window grows to a step that exceeds it, to a multiple of 4 096"""
        caps, w, off = [self.cap] * self.nwindows, 0, 0
        for n in self.prog.sizes:
            n += 20
            if off and off + n > caps[w]:
                w, off = (w + 1) % self.nwindows, 0
            if off == 0 and n > caps[w]:
                caps[w] = (n + 4095) & ~4095
            off += n
            if off == caps[w]:
                w, off = (w + 1) % self.nwindows, 0
        return self.S * sum(caps)

    def run(self, form):
        out = self.out[form]
        L, pn, h = engine.lib(), C.byref(self.n), out.h
        garble, pre = L.gc_stream_batch_out_garble, self.prefix.ctypes.data_as(C.c_void_p)
        flushed = self.threading.Event()

        def consumer():
            while True:
                last = flushed.is_set()
                if out.next() is None:
                    if last:
                        return
                    time.sleep(0.0001)
                    continue
                out.release()

        t = self.threading.Thread(target=consumer)
        t.start()
        try:
            for k, a in enumerate(self.prog.args.begin):
                while True:
                    rc = garble(h, pre, 20, *a, pn)
                    if rc != engine.GC_E_BUSY:
                        break
                    time.sleep(0.00005)  # (no window is free: let the consumer run)
                if rc:
                    raise engine.EngineError(rc, "gc_stream_batch_out_garble(step %d, %s)" % (k, form))
            out.flush()
        finally:
            flushed.set()
            t.join()

    def window(self, form):
        self.ctx.sync()
        t0 = time.perf_counter()
        self.run(form)
        self.ctx.sync()
        return time.perf_counter() - t0

    def close(self):
        for o in self.out.values():
            o.close()


def egress_split(ctx, prog, S, reps, nwindows):
    head = {"bench": "stream_batch_egress_split", "program": PROGRAM, "sessions": S, "window_bytes": EGRESS_WINDOW, "windows": nwindows}
    b = Batch(ctx, prog, S, np.zeros(prog.bytes, np.uint8))  # (the evaluator is not run here)
    try:
        e = SplitEgress(ctx, prog, b, nwindows)
    except engine.EngineError as err:
        b.close()
        return dict(head, skipped="windows not allocated: %s" % err)
    forms = ("windows", "split")
    for f in forms:
        e.window(f)
    first = {f: e.out[f].stats() for f in forms}
    t = {f: [] for f in forms}
    for _ in range(reps):
        for f in forms:
            t[f].append(e.window(f))
    row = dict(head, key_bytes=32, steps=len(prog.steps), bytes_per_session=prog.bytes + 20 * len(prog.steps), reps=reps,
               largest_step_bytes=max(prog.sizes) + 20)
    for f in forms:
        sealed, _, grown, busy = e.out[f].stats()
        row[f] = {"seconds": statistics.median(t[f]), "seconds_all": t[f], "grown": grown,
                  "sealed_per_pass": (sealed - first[f][0]) / reps, "busy_answers_per_pass": (busy - first[f][3]) / reps,
                  "pinned_bytes_of_the_handle": e.unsplit_pinned_bytes() if f == "windows" else nwindows * S * e.cap}
    steps, segments = e.out["split"].split_stats()
    row["split"].update(split_steps_per_pass=steps / (reps + 1), segments_per_pass=segments / (reps + 1))
    row["split_over_windows"] = row["split"]["seconds"] / row["windows"]["seconds"]
    row["ranges_overlap"] = not (max(t["split"]) < min(t["windows"]) or max(t["windows"]) < min(t["split"]))
    e.close()
    b.close()
    return row


class Intake:
    """the garbler's windows of a Batch in pinned memory, and the two ways of an evaluator through them"""

    def __init__(self, ctx, prog, b):
        self.ctx, self.prog, self.b, self.S = ctx, prog, b, b.S
        out = b.sb.out(EGRESS_WINDOW, EGRESS_WINDOWS)
        n = C.c_size_t(0)
        self.windows, self.msgs, self.pinned_bytes = [], [], 0

        def drain():
            while True:
                v = out.next_view()
                if v is None:
                    return
                p = engine.PinnedArray(v.shape, np.uint8)
                p.a[:] = v
                self.windows.append(p)
                self.pinned_bytes += v.size
                out.release()

        for k, (a, ev) in enumerate(zip(prog.args.begin, prog.eval_args)):
            hdr = np.frombuffer(struct.pack(">5I", 1, k, *ev), np.uint8)
            while True:
                rc = engine.lib().gc_stream_batch_out_garble(out.h, hdr.ctypes.data_as(C.c_void_p), 20, *a, C.byref(n))
                if rc != engine.GC_E_BUSY:
                    break
                drain()
            if rc:
                raise engine.EngineError(rc, "gc_stream_batch_out_garble(step %d)" % k)
        out.flush()
        drain()
        out.close()
        self.bytes_per_session = sum(w.a.shape[1] for w in self.windows)
        assert self.bytes_per_session == prog.bytes + 20 * len(prog.steps)
        # a second evaluator with the same input labels: (a) runs on the Batch's, (b) on this one
        self.se_b = engine.StreamEvalBatch(ctx, self.S, b.d_keys, 32)
        d_w = engine.DeviceBuffer(ctx, shape=(self.S, len(prog.prim)), dtype=engine.WIRE)
        b.sb.gather_wires(prog.prim, d_w)
        self.se_b.set_wires(prog.prim, engine.DeviceBuffer(ctx, data=np.ascontiguousarray(d_w.numpy()["l0"])))
        self.it = self.se_b.intake(0, EGRESS_WINDOW)
        self.n, self.op = C.c_size_t(0), C.c_uint32(0)

    def run_steps(self):
        """the parent's route: the caller reads the framing of session 0 and makes one call, and one upload, per step"""
        L, e, pn = engine.lib(), self.b.se.h, C.byref(self.n)
        call, unpack = L.gc_stream_eval_batch_circuit_host, struct.Struct(">5I").unpack_from
        calls = 0
        for w in self.windows:
            row0, base, (_, width) = w.a[0], w.ptr, w.a.shape
            at = 0
            while at < width:
                op, _, ngates, ntmp, nwires = unpack(row0, at)
                assert op == 1
                rc = call(e, ngates, ntmp, nwires, C.c_void_p(base + at + 20), width, width - at - 20, 0, pn)
                if rc:
                    raise engine.EngineError(rc, "gc_stream_eval_batch_circuit_host")
                at += 20 + self.n.value
                calls += 1
        return calls

    def run_feed(self):
        L, h, pn, po = engine.lib(), self.it.h, C.byref(self.n), C.byref(self.op)
        for w in self.windows:
            width = w.a.shape[1]
            rc = L.gc_stream_eval_batch_in_feed(h, C.c_void_p(w.ptr), width, width, pn, po)
            if rc or self.n.value != width or self.op.value != 1:
                raise engine.EngineError(rc, "gc_stream_eval_batch_in_feed: taken %d of %d, next op %d" % (self.n.value, width, self.op.value))
        return len(self.windows)

    def window(self, run):
        self.ctx.sync()
        t0 = time.perf_counter()
        run()
        self.ctx.sync()
        return time.perf_counter() - t0

    def check(self):
        """both routes leave the same labels on the outputs of the last steps, all of them the garbler's L0 or L1; no
        structure byte differed"""
        outs = [o for _, _, out_ in self.prog.steps[-8:] for o in out_]
        la, lb = self.b.se.return_labels(outs), self.se_b.return_labels(outs)
        assert (la == lb).all() and (self.b.se.bad() == 0).all() and (self.se_b.bad() == 0).all()
        for j in (0, len(outs) - 1):
            wire = self.b.sb.get(outs[j])
            assert ((lb[:, j] == wire["l0"]) | (lb[:, j] == wire["l1"])).all(), outs[j]

    def close(self):
        self.it.close()
        self.se_b.close()
        for w in self.windows:
            w.close()


def intake(ctx, prog, S, reps, once_only=False):
    b = Batch(ctx, prog, S, np.zeros(prog.bytes, np.uint8))
    try:
        x = Intake(ctx, prog, b)
    except engine.EngineError as err:
        b.close()
        return {"bench": "stream_batch_intake", "program": PROGRAM, "sessions": S, "skipped": "windows not kept: %s" % err}
    if once_only:
        x.window(x.run_feed)
        x.close(), b.close()
        return None
    calls = x.run_steps()
    ctx.sync()
    x.window(x.run_feed)
    x.check()
    t = {"per_step": [], "intake": []}
    for _ in range(reps):
        t["per_step"].append(x.window(x.run_steps))
        t["intake"].append(x.window(x.run_feed))
    x.check()
    steps, nbytes, uploads, carried = x.it.stats()
    med = {k: statistics.median(v) for k, v in t.items()}
    row = {
        "bench": "stream_batch_intake", "program": PROGRAM, "sessions": S, "key_bytes": 32, "steps": len(prog.steps),
        "bytes_per_session": x.bytes_per_session, "window_bytes": EGRESS_WINDOW, "windows": len(x.windows), "reps": reps,
        "pinned_bytes": x.pinned_bytes, "per_step_calls_per_pass": calls, "feeds_per_pass": len(x.windows),
        "per_step_s": med["per_step"], "intake_s": med["intake"], "intake_over_per_step": med["intake"] / med["per_step"],
        "per_step_spread_s": max(t["per_step"]) - min(t["per_step"]),
        "intake_not_slower_beyond_the_spread_of_per_step": med["intake"] <= max(t["per_step"]),
        "upload_bytes_per_s_intake": x.bytes_per_session * S / med["intake"],
        "intake_steps_per_pass": steps / (reps + 1), "intake_uploads_per_pass": uploads / (reps + 1), "intake_carried_bytes": carried,
        "intake_bytes_per_session_per_pass": nbytes / (reps + 1), "seconds_all": t,
    }
    x.close()
    b.close()
    return row


def once(ctx, prog, S):
    """one garble+eval pass and nothing else timed: the run a kernel trace is taken of"""
    _, _, ref_stream, _ = one_session(ctx, prog, bytes(range(32)), bs.stream_rnd(PROGRAM, len(prog.prim)), evaluate=False)
    b = Batch(ctx, prog, S, ref_stream)
    b.window(True)
    b.check()
    b.close()


def split(path, prog, S):
    """device seconds per group of kernels from a rocprofv3 kernel-stats csv of `--once S`"""
    groups = {"keyed_garble": ("k_garble_flat_keyed", "k_garble_hbm_keyed"), "keyed_eval": ("k_eval_flat_keyed", "k_eval_hbm_keyed"),
              "expand_keys": ("k_expand_keys",),
              "movers": ("k_gather", "k_sb_rnd_form", "k_sb_rows"), "serialiser": ("k_sb_serialise",), "ingester": ("k_sb_ingest",)}
    sec = {g: 0.0 for g in groups}
    calls = {g: 0 for g in groups}
    for r in csv.DictReader(open(path)):
        for g, names in groups.items():
            if any(n + "<" in r["Name"] or n + "(" in r["Name"] for n in names):
                sec[g] += float(r["TotalDurationNs"]) * 1e-9
                calls[g] += int(r["Calls"])
    moved = prog.bytes * S
    return {"bench": "stream_batch_split", "program": PROGRAM, "sessions": S, "steps": len(prog.steps), "device_seconds": sec,
            "launches": calls, "us_per_step": {g: v / len(prog.steps) * 1e6 for g, v in sec.items()},
            "serialiser_bytes_per_s": moved / sec["serialiser"] if sec["serialiser"] else None,
            "serialiser_fraction_of_8TBps": moved / sec["serialiser"] / HBM_BYTES_PER_S if sec["serialiser"] else None,
            "ingester_bytes_per_s": moved / sec["ingester"] if sec["ingester"] else None,
            "ingester_fraction_of_8TBps": moved / sec["ingester"] / HBM_BYTES_PER_S if sec["ingester"] else None}


def main():
    global PROGRAM
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, nargs="*", default=[64, 256, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=2, help="one-session streams the baseline is timed on")
    ap.add_argument("--max-steps", type=int, default=None, help="only the first steps of the program (a quick look)")
    ap.add_argument("--once", type=int, default=None, help="one garble+eval pass at this many sessions (for a kernel trace)")
    ap.add_argument("--kernel-stats", default=None, help="kernel-stats csv of a traced --once run: print its split (with --sessions S)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--egress", action="store_true", help="the garbler's bytes to host memory: device-only, synchronous download, "
                                                          "gc_stream_batch_out_* windows, the copy alone")
    ap.add_argument("--split", action="store_true", help="with --egress: today's window handle beside the split handle")
    ap.add_argument("--windows", type=int, nargs="*", default=[3, 4], help="with --egress --split: windows per handle")
    ap.add_argument("--split-once", type=int, default=None, help="three passes through today's window handle, then three through "
                                                                 "the split handle, at this many sessions (for a kernel trace)")
    ap.add_argument("--intake", action="store_true", help="the evaluator through the garbler's windows: one call per step beside "
                                                          "one gc_stream_eval_batch_in_feed per window")
    ap.add_argument("--intake-once", type=int, default=None, help="one intake pass at this many sessions (for a kernel trace)")
    ap.add_argument("--program", default=PROGRAM, choices=sorted(PROGRAMS), help="big130_16: wide steps, wires in HBM")
    a = ap.parse_args()
    PROGRAM = a.program
    if PROGRAM.startswith("big"):
        os.environ.setdefault("GC_STREAM_BATCH_CACHE_BYTES", str(16 << 30))
    prog = Program(a.max_steps)

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if a.kernel_stats:
        emit(split(a.kernel_stats, prog, a.sessions[0]))
        return
    ctx = engine.Context(0)
    if a.once:
        once(ctx, prog, a.once)
    elif a.intake_once:
        intake(ctx, prog, a.intake_once, 0, once_only=True)
    elif a.intake:
        for S in a.sessions:
            emit(intake(ctx, prog, S, a.reps))
    elif a.split_once:
        b = Batch(ctx, prog, a.split_once, np.zeros(prog.bytes, np.uint8))
        e = SplitEgress(ctx, prog, b, a.windows[0])
        for f in ("windows", "split"):
            print(f, [round(e.window(f), 4) for _ in range(3)], flush=True)
        e.close()
        b.close()
    elif a.egress and a.split:
        for S in a.sessions:
            for nw in a.windows:
                emit(egress_split(ctx, prog, S, a.reps, nw))
    elif a.egress:
        for S in a.sessions:
            emit(egress(ctx, prog, S, a.reps))
    else:
        for S in a.sessions:
            emit(measure(ctx, prog, S, a.reps, a.sample))
    ctx.close()


if __name__ == "__main__":
    main()
