"""KOS check of the malicious IKNP variant, S sessions per call (gc_kos_multi_*_dev) beside the one-session calls: one JSON
line per (role, S, per), everything in HBM.  The protocol is scripts/bench_iknp_multi.py's: a host clock around k calls that
end in gc_ctx_sync, k sized once (after a warm-up) so that a window lasts at least --window seconds; per-call time =
window / k; median over --reps windows, every rep reported; the three rows of a role alternate in one process.

  multi        the multi _dev call: receiver (tags) and sender (check), S sessions of per + 256 labels
  single       ONE gc_kos_*_dev call over S * (per + 256) - 256 labels (plus its own 256 of the choice vector): the same
               number of multiplications under one key, spread over the whole grid.  The call allocates, copies its choice
               vector in and its sums out and waits, as it does for every caller
  sequential   what a caller does without the multi call: one gc_kos_*_dev call per session on slices of the session-major
               arrays, timed on at most --sample sessions and scaled to S

The sender's multi rows run the honest path (every session passes: delta = 0 and the receiver's tags over the same labels).
`single_spread` is (max - min) / median of single's repetitions: the margin of multi_over_single.  Bytes per label: 16 of
label and a choice bit; the kernel is bound by the AES block and the 128 x 128 carry-less multiply of every label
(DESIGN.md § 13), so ns_per_label is the figure to read."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mpc_amd import engine  # noqa: E402
from mpc_amd.circuit import LABEL  # noqa: E402
from scripts.bench_co import calls_for, timed  # noqa: E402

SHAPES = [(8, 128), (1024, 128), (1024, 127), (8192, 128), (1024, 512), (64, 16384)]


def shapes_of(text):
    return [tuple(int(v) for v in s.split("x")) for s in text.split(",") if s]


def labels(rng, shape):
    out = np.zeros(shape, LABEL)
    out["d0"] = rng.integers(0, 1 << 64, shape, dtype=np.uint64)
    out["d1"] = rng.integers(0, 1 << 64, shape, dtype=np.uint64)
    return out


def tup(l):
    return int(l["d0"]), int(l["d1"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join("%dx%d" % s for s in SHAPES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--sample", type=int, default=64, help="sessions the sequential rows are timed on")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    ctx = engine.Context(0)
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    rng = np.random.default_rng(13)
    for S, per in shapes_of(a.shapes):
        n = S * per
        total = S * (per + 256)  # labels multiplied by a multi call
        n_single = total - 256   # ... and the same number in one session: n_single + its choice vector
        row = 64 * -(-per // 512)
        sample = min(S, a.sample)
        seed2, delta, tags = labels(rng, S), labels(rng, S), labels(rng, (S, 3))
        cv, bcv = labels(rng, 256), rng.integers(0, 2, 256).astype(np.uint8)
        d_seed2, d_delta = ctx.to_device(seed2.view(np.uint8)), ctx.to_device(delta.view(np.uint8))
        d_res = ctx.random_u8((max(n, n_single), 16), seed=1)
        d_bytes = ctx.random_u8(max(n_single, 1), high=2, seed=2)  # one byte per OT: the one-session call's choices
        d_packed, d_bcvp = ctx.random_u8(S * row, seed=3), ctx.random_u8(S * 64, seed=4)
        d_cv = ctx.random_u8((S * 256, 16), seed=5)
        d_tags_in, d_tags = ctx.zeros((S * 3, 16)), ctx.zeros((S * 3, 16))
        d_ok, d_status = ctx.zeros(S), ctx.zeros(16)
        # the honest path for the multi sender: with delta = 0 the receiver's tags over the SAME labels are the sender's sums,
        # so every session passes and no status atomic is issued (the multiply by delta runs whatever delta holds)
        d_delta.zero()
        engine.kos_multi_receiver_tags_dev(ctx, d_seed2, d_res, d_packed, d_cv, d_bcvp, S, per, d_tags_in)
        ctx.sync()
        s0, dl0, x0, t00, t10 = tup(seed2[0]), tup(delta[0]), tup(tags[0, 0]), tup(tags[0, 1]), tup(tags[0, 2])

        def multi_receiver():
            engine.kos_multi_receiver_tags_dev(ctx, d_seed2, d_res, d_packed, d_cv, d_bcvp, S, per, d_tags)

        def multi_sender():
            engine.kos_multi_sender_check_dev(ctx, d_seed2, d_res, d_cv, d_delta, d_tags_in, S, per, d_ok, d_status)

        def seq_receiver():
            for s in range(sample):
                engine.kos_receiver_tags_dev(ctx, tup(seed2[s]), d_res.ptr + 16 * s * per, d_bytes.ptr + s * per, per, cv, bcv)

        def seq_sender():
            for s in range(sample):
                engine.kos_sender_check_dev(ctx, tup(seed2[s]), d_res.ptr + 16 * s * per, per, cv, tup(delta[s]), x0, t00, t10)

        calls = {
            "receiver": (multi_receiver, lambda: engine.kos_receiver_tags_dev(ctx, s0, d_res, d_bytes, n_single, cv, bcv),
                         seq_receiver),
            "sender": (multi_sender, lambda: engine.kos_sender_check_dev(ctx, s0, d_res, n_single, cv, dl0, x0, t00, t10),
                       seq_sender),
        }
        ks = {name: tuple(calls_for(ctx, fn, a.window) for fn in fns) for name, fns in calls.items()}
        times = {name: ([], [], []) for name in calls}
        for _ in range(a.reps):  # alternating
            for name, fns in calls.items():
                for side in range(3):
                    times[name][side].append(timed(ctx, fns[side], ks[name][side]))
        failed = [int(v) for v in d_status.download(np.uint64)]
        assert failed == [0, (1 << 64) - 1] and (d_ok.numpy() == 1).all(), failed
        for name in calls:
            multi, single, seq = (statistics.median(t) for t in times[name])
            seq_scaled = seq * S / sample
            spread = (max(times[name][1]) - min(times[name][1])) / single
            emit(dict(bench="kos_multi", role=name, S=S, per=per, labels=total, reps=a.reps, calls_per_window=list(ks[name]),
                      team="wave" if per + 256 <= 1024 else "workgroup",
                      multi_ms=round(multi * 1e3, 4), multi_ms_all=[round(t * 1e3, 4) for t in times[name][0]],
                      single_ms=round(single * 1e3, 4), single_ms_all=[round(t * 1e3, 4) for t in times[name][1]],
                      single_spread=round(spread, 3),
                      sequential_ms=round(seq_scaled * 1e3, 4), sequential_sample=sample,
                      sequential_sample_ms_all=[round(t * 1e3, 4) for t in times[name][2]],
                      failed_sessions=failed[0], multi_over_single=round(multi / single, 3), sequential_over_multi=round(seq_scaled / multi, 2),
                      ns_per_label=round(multi * 1e9 / total, 3)))
        for d in (d_seed2, d_delta, d_res, d_bytes, d_packed, d_bcvp, d_cv, d_tags_in, d_tags, d_ok, d_status):
            d.close()
    ctx.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
