"""Device random streams (gc_rand_*) beside what a host had to do before them, one JSON line per shape:

  garbler   S = 1 024 sessions, the two draws of circuit.Garbler for aes_128: 32 + 4 112 bytes each (gc_rand_fill_dev twice)
  gmw       S = 1, 16 MiB as tripleBatch's shares of a 2^20-word batch (gc_rand_gmw_shares_dev)
  bulk      S = 1 024, 1 MiB each (gc_rand_fill_dev)

Each draw is timed against two yardsticks, the three alternating in one process:
  upload    gc_dev_upload of the same number of bytes from pinned host memory: what the parent commit offers a host that has
            the bytes already (making them is not counted)
  garble    the gc_batch_garble_keyed pass of aes_128 x 1 024 under 32-byte keys that the first shape feeds (a hipGraph)

Method (as scripts/bench_batch_keyed.py): PREWARM untimed runs of every pass, then --reps rounds, each timing the passes one
after the other: a host clock around k calls between two gc_ctx_sync, k sized once so that a window lasts at least --window
seconds; ms per call = window / k, the median of the rounds is reported with every round beside it.  A draw cannot be part of
a captured graph (its position is a kernel argument), so the draws are plain calls through the ctypes binding: at the first
shape, whose kernels run for microseconds, the figure is the rate at which a Python host issues them.

  draw_bytes_per_s        bytes written per second of draw
  fraction_of_lds_bound   of the 1.2 TB/s the LDS look-ups allow AES-256 (76e9 blocks/s; README, derived, not measured here)
  draw_over_upload        draw_ms / upload_ms (below 1: the draw is faster than carrying the bytes over)
  draw_over_garble        draw_ms / garble_ms

--cursor measures the per-session cursors instead (gc_rand_*_cur*; rows "rand_cursor"), by the same protocol:
  fill      gc_rand_fill_cur_dev against gc_rand_fill_dev at the three shapes, the old call twice (fill_a, fill_b: an A/A pair
            that gives the run-to-run spread) and the cursor call, alternating.  The cursors are not reset between calls: every
            call goes on where the array stands, as a host loop would have it.
  scalars   gc_rand_scalars_cur_dev at (S, count, max) against gc_dev_upload of the same S * count * 32 bytes from pinned memory
  step      the captured step {fill_cur 32 -> d_keys, fill_cur 16 (1 + n) -> d_rnd, scalars_cur (N, 1) -> d_a, garble_keyed} of
            aes_128 x 1 024: one graph replay against the same four calls issued uncaptured with gc_rand_fill_dev standing in
            for the cursor fills
--once runs every cursor pass once and measures nothing: the run a kernel trace is taken of."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mpc_amd import engine, parse_file  # noqa: E402

PREWARM = 20
LDS_BOUND_BYTES_PER_S = 76e9 * 16  # README, round-1 table: AES-256 blocks per second the LDS array allows (derived)


def window(ctx, call, k):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(k):
        call()
    ctx.sync()
    return (time.perf_counter() - t0) / k * 1e3


def alternate(ctx, passes, reps, seconds):
    for call in passes.values():
        for _ in range(PREWARM):
            call()
    ks = {}
    for name, call in passes.items():
        ms = window(ctx, call, 5)
        ks[name] = max(5, int(seconds * 1e3 / max(ms, 1e-3)))
    out = {name: [] for name in passes}
    for _ in range(reps):
        for name, call in passes.items():
            out[name].append(window(ctx, call, ks[name]))
    return out, ks


P256_N = engine.P256_N


def emit(a, row):
    line = json.dumps(row)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def measure(a, ctx, passes):
    """-> (median ms per pass, every round, calls per window); with --once every pass runs once and the times are None"""
    if a.once:
        for call in passes.values():
            call()
        ctx.sync()
        return {k: None for k in passes}, {}, {}
    t, ks = alternate(ctx, passes, a.reps, a.window)
    return {k: statistics.median(v) for k, v in t.items()}, t, ks


def cursor_rows(a, ctx):
    rng = np.random.default_rng(7)
    c = parse_file(os.path.join(ROOT, "tests", "golden", "aes_128.gcf"))
    batch, nrnd = 1024, 16 * (1 + c.num_inputs)
    base = {"bench": "rand_cursor", "key_bytes": 32, "reps": a.reps, "window_s": a.window}
    h = engine.RandStreams(ctx, rng.integers(0, 256, (batch, 32), dtype=np.uint8))
    h1 = engine.RandStreams(ctx, rng.integers(0, 256, (1, 32), dtype=np.uint8))
    d_status = ctx.zeros(2, np.uint64)
    d_cur, d_cur1 = ctx.zeros(batch, np.uint64), ctx.zeros(1, np.uint64)
    d_keys, d_rnd, d_a = ctx.empty((batch, 32)), ctx.empty((batch, nrnd)), ctx.empty((batch, 32))

    # ---- fill against gc_rand_fill_dev ----
    d_bulk = ctx.empty((1024, 1 << 20))

    def old_garbler():
        h.fill(32, d_keys)
        h.fill(nrnd, d_rnd)

    def cur_garbler():
        h.fill_cur(d_cur, 32, d_keys, d_status)
        h.fill_cur(d_cur, nrnd, d_rnd, d_status)

    fills = {
        "garbler": (batch, 32 + nrnd, 2, old_garbler, cur_garbler),
        "one_stream": (1, 16 << 20, 1, lambda: h1.fill(16 << 20, d_bulk), lambda: h1.fill_cur(d_cur1, 16 << 20, d_bulk, d_status)),
        "bulk": (1024, 1 << 20, 1, lambda: h.fill(1 << 20, d_bulk), lambda: h.fill_cur(d_cur, 1 << 20, d_bulk, d_status)),
    }
    for name, (S, per, calls, old, new) in fills.items() if "fill" in a.kinds else ():
        h.seek(0)
        h1.seek(0)
        h.cur_set(d_cur, 0)
        h1.cur_set(d_cur1, 0)
        med, t, ks = measure(a, ctx, {"fill_a": old, "cursor": new, "fill_b": old})
        row = dict(base, kind="fill", shape=name, S=S, bytes_per_stream=per, total_bytes=S * per, calls_per_draw=calls,
                   calls_per_window=ks, fill_a_ms=med["fill_a"], fill_b_ms=med["fill_b"], cursor_ms=med["cursor"], ms_all=t)
        if not a.once:
            row.update(aa_ratio=med["fill_b"] / med["fill_a"], cursor_over_fill=med["cursor"] / min(med["fill_a"], med["fill_b"]),
                       cursor_bytes_per_s=S * per / (med["cursor"] * 1e-3))
        emit(a, row)
    d_bulk.close()

    # ---- scalars against an upload of the same bytes ----
    for S, count, mx, tag in ((1024, 1, P256_N, "N"), (1024, 128, P256_N, "N"), (1024, 1, (1 << 255) + 1, "2^255+1"),
                              (1024, 128, (1 << 255) + 1, "2^255+1"), (1, 131072, P256_N, "N"),
                              (1024, 128, 3, "3")) if "scalars" in a.kinds else ():
        hs, dc_ = (h, d_cur) if S == batch else (h1, d_cur1)
        total = S * count * 32
        d_out, d_up = ctx.empty(total), ctx.empty(total)
        pin = engine.PinnedArray(total, np.uint8)
        pin.a[:] = 0x5A
        hs.cur_set(dc_, 0)
        med, t, ks = measure(a, ctx, {"scalars": lambda: hs.scalars_cur(dc_, mx, count, d_out, d_status),
                                      "upload": lambda: d_up.upload(pin.a)})
        row = dict(base, kind="scalars", S=S, count=count, max=tag, total_bytes=total, calls_per_window=ks,
                   scalars_ms=med["scalars"], upload_ms=med["upload"], ms_all=t)
        if not a.once:
            row.update(scalars_over_upload=med["scalars"] / med["upload"], draws_per_s=S * count / (med["scalars"] * 1e-3))
        emit(a, row)
        pin.close()
        d_out.close()
        d_up.close()

    # ---- the captured step ----
    if "step" not in a.kinds:
        h.close()
        h1.close()
        return
    dc = engine.DeviceCircuit(ctx, c)
    gb = engine.Batch(dc, batch)
    assert gb.keyed_supported()
    gb.set_graph(True)

    def step_cursor():
        h.fill_cur(d_cur, 32, d_keys, d_status)
        h.fill_cur(d_cur, nrnd, d_rnd, d_status)
        h.scalars_cur(d_cur, P256_N, 1, d_a, d_status)
        gb.garble_keyed(d_keys, 32, d_rnd)

    def step_calls():
        h.fill(32, d_keys)
        h.fill(nrnd, d_rnd)
        h.scalars_cur(d_cur, P256_N, 1, d_a, d_status)
        gb.garble_keyed(d_keys, 32, d_rnd)

    h.seek(0)
    h.cur_set(d_cur, 0)
    step_cursor()
    ctx.sync()
    g = ctx.capture(step_cursor)
    med, t, ks = measure(a, ctx, {"replay": g.launch, "calls": step_calls})
    row = dict(base, kind="step", step="aes_128 x 1024: fill_cur 32, fill_cur 16 (1 + n), scalars_cur (N, 1), garble_keyed",
               calls_per_window=ks, replay_ms=med["replay"], calls_ms=med["calls"], ms_all=t)
    if not a.once:
        row.update(replay_over_calls=med["replay"] / med["calls"])
    emit(a, row)
    g.close()
    gb.close()
    dc.close()
    h.close()
    h1.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cursor", action="store_true", help="the rows of the per-session cursors instead")
    ap.add_argument("--once", action="store_true", help="with --cursor: run every pass once, measure nothing")
    ap.add_argument("--kinds", default="fill,scalars,step", help="with --cursor: which rows")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--shapes", default="garbler,gmw,bulk")
    a = ap.parse_args()
    ctx = engine.Context(0)
    if a.cursor:
        cursor_rows(a, ctx)
        ctx.close()
        return
    rng = np.random.default_rng(7)
    # the keyed garble pass of the headline batch, fed once by the draws it is compared with
    c = parse_file(os.path.join(ROOT, "tests", "golden", "aes_128.gcf"))
    batch, nrnd = 1024, 16 * (1 + c.num_inputs)
    dc = engine.DeviceCircuit(ctx, c)
    gb = engine.Batch(dc, batch)
    assert gb.keyed_supported()
    d_keys, d_rnd = ctx.empty((batch, 32)), ctx.empty((batch, nrnd))
    hg = engine.RandStreams(ctx, rng.integers(0, 256, (batch, 32), dtype=np.uint8))
    hg.draw_garbler(c.num_inputs, d_keys, d_rnd)
    gb.garble_keyed(d_keys, 32, d_rnd)
    ctx.sync()
    garble = ctx.capture(lambda: gb.garble_keyed(d_keys, 32, d_rnd))

    def garbler_draw():
        hg.seek(0)
        hg.draw_garbler(c.num_inputs, d_keys, d_rnd)

    shapes, handles = {}, [hg]
    if "garbler" in a.shapes:
        shapes["garbler"] = (batch, 32 + nrnd, 2, garbler_draw)
    if "gmw" in a.shapes:
        words = 1 << 20
        h1 = engine.RandStreams(ctx, rng.integers(0, 256, (1, 32), dtype=np.uint8))
        handles.append(h1)
        d_a, d_b = ctx.empty(words, np.uint64), ctx.empty(words, np.uint64)
        shapes["gmw"] = (1, 16 * words, 1, lambda: h1.gmw_shares(words, d_a, d_b))
    if "bulk" in a.shapes:
        hb = engine.RandStreams(ctx, rng.integers(0, 256, (1024, 32), dtype=np.uint8))
        handles.append(hb)
        d_bulk = ctx.empty((1024, 1 << 20))
        shapes["bulk"] = (1024, 1 << 20, 1, lambda: hb.fill(1 << 20, d_bulk))
    for name, (S, per, calls, draw) in shapes.items():
        total = S * per
        pin = engine.PinnedArray(total, np.uint8)
        pin.a[:] = 0x5A
        d_up = ctx.empty(total)
        t, ks = alternate(ctx, {"draw": draw, "upload": lambda: d_up.upload(pin.a), "garble": garble.launch}, a.reps, a.window)
        med = {k: statistics.median(v) for k, v in t.items()}
        row = {
            "bench": "rand", "shape": name, "S": S, "bytes_per_stream": per, "total_bytes": total, "key_bytes": 32,
            "calls_per_draw": calls, "reps": a.reps, "window_s": a.window, "calls_per_window": ks,
            "draw_ms": med["draw"], "upload_ms": med["upload"], "garble_ms": med["garble"],
            "draw_bytes_per_s": total / (med["draw"] * 1e-3), "upload_bytes_per_s": total / (med["upload"] * 1e-3),
            "fraction_of_lds_bound": total / (med["draw"] * 1e-3) / LDS_BOUND_BYTES_PER_S,
            "draw_over_upload": med["draw"] / med["upload"], "draw_over_garble": med["draw"] / med["garble"],
            "garble_pass": "aes_128 x 1024, gc_batch_garble_keyed, 32-byte keys", "ms_all": t,
        }
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        pin.close()
        d_up.close()
    garble.close()
    for h in handles:
        h.close()
    gb.close()
    dc.close()
    ctx.close()


if __name__ == "__main__":
    main()
