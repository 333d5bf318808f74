"""Chou-Orlandi base OT, several sessions per call (gc_co_multi_*_dev) beside the one-session calls at the same total work:
one JSON line per (call, S, per), everything in HBM.  The protocol is scripts/bench_co.py's: a host clock around k calls that
end in gc_ctx_sync, k sized once (after a warm-up) so that a window lasts at least --window seconds; per-call time = window
/ k; median over --reps windows, every rep reported; the multi call and its one-session yardstick alternate in one process.

  multi_setup     gc_co_multi_sender_setup_dev, S sessions; yardstick: S x gc_co_sender_setup on the host (timed on a
                  sample of at most 64 sessions and scaled)
  multi_choices   gc_co_multi_receiver_choices_dev; yardstick: gc_co_base_choices_dev (G's table as well) at n = S * per
  multi_encrypt   gc_co_multi_sender_encrypt_dev;   yardstick: gc_co_sender_encrypt_dev at n = S * per
  multi_decrypt   gc_co_multi_receiver_decrypt_dev; yardstick: gc_co_receiver_decrypt_dev (the ladder) at n = S * per

The yardsticks do the same number of OTs with ONE session's constants, so `ratio` = multi / single is what per-lane
constants and the divergence of a wave that spans sessions cost.  With --sequential S (default 8) the script also times
what a caller without the multi calls does for S sessions of `per` OTs: S one-session sender sequences (host setup +
encrypt) and S gc_co_base receiver sequences (create + choices + decrypt + free), each ending in gc_ctx_sync.

With --base-shapes the script times the receiver handle over S sessions instead (gc_co_multi_base_*: per-session window tables
built on the device), by the same method and on the same buffers, the three calls alternating in one process:

  base_create     gc_co_multi_base_create_dev + gc_co_multi_base_free: the build of S tables, its allocations included
  base_decrypt    gc_co_multi_base_decrypt_dev through a handle that exists
  ladder_decrypt  gc_co_multi_receiver_decrypt_dev, the call the handle replaces

one line per shape, with `create_plus_decrypt_ms` and `speedup` = ladder / (create + decrypt): what a caller gains who builds
the tables for ONE decrypt, as ReceiveMultiHIP does."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mpc_amd import engine  # noqa: E402
from scripts.bench_co import calls_for, timed  # noqa: E402

SHAPES = [(8, 128), (1024, 128), (1024, 127), (131072, 1)]
BASE_SHAPES = [(8, 128), (1024, 128), (1024, 127), (8192, 128), (1024, 8), (1024, 16), (1024, 32), (1024, 64), (1024, 256)]


def shapes_of(text):
    return [tuple(int(v) for v in s.split("x")) for s in text.split(",") if s]


def bench_base(ctx, a, emit):
    """the rows of the receiver handle; the labels of the two decrypts are compared once per shape"""
    rng = np.random.default_rng(11)
    for S, per in shapes_of(a.base_shapes):
        n = S * per
        d_a = ctx.to_device(rng.integers(0, 256, (S, 32), dtype=np.uint8))
        d_A, d_ainv, d_st, d_st1 = ctx.zeros((S, 64)), ctx.zeros((S, 64)), ctx.zeros(4, np.uint64), ctx.zeros(4, np.uint64)
        d_sc, d_ch, d_ct = ctx.random_u8((n, 32), seed=1), ctx.random_u8(n, high=2, seed=2), ctx.random_u8((n, 32), seed=4)
        d_lab, d_lab1 = ctx.zeros((n, 16)), ctx.zeros((n, 16))
        engine.co_multi_sender_setup_dev(ctx, d_a, S, d_A, d_ainv, d_st)
        ctx.sync()
        h = engine.CoMultiBase(ctx, d_A, S)
        assert h.info() == (S, 0, None)

        def create():
            engine.CoMultiBase(ctx, d_A, S).close()

        fns = {"base_create": create,
               "base_decrypt": lambda: h.decrypt_dev(d_sc, d_ch, d_ct, per, 0, d_lab, d_st),
               "ladder_decrypt": lambda: engine.co_multi_receiver_decrypt_dev(ctx, d_A, d_sc, d_ch, d_ct, S, per, 0, d_lab1, d_st1)}
        ks = {name: calls_for(ctx, fn, a.window) for name, fn in fns.items()}
        times = {name: [] for name in fns}
        for _ in range(a.reps):  # alternating
            for name, fn in fns.items():
                times[name].append(timed(ctx, fn, ks[name]))
        clean = [0, (1 << 64) - 1, 0, (1 << 64) - 1]
        assert [int(v) for v in d_st.numpy()] == clean and [int(v) for v in d_st1.numpy()] == clean
        assert (d_lab.numpy() == d_lab1.numpy()).all(), "the handle's labels differ from the ladder's"
        med = {name: statistics.median(t) for name, t in times.items()}
        both = med["base_create"] + med["base_decrypt"]
        emit(dict(bench="co_multi_base", S=S, per=per, n=n, reps=a.reps, calls_per_window=ks,
                  create_ms=round(med["base_create"] * 1e3, 4), create_ms_all=[round(t * 1e3, 4) for t in times["base_create"]],
                  decrypt_ms=round(med["base_decrypt"] * 1e3, 4), decrypt_ms_all=[round(t * 1e3, 4) for t in times["base_decrypt"]],
                  ladder_ms=round(med["ladder_decrypt"] * 1e3, 4),
                  ladder_ms_all=[round(t * 1e3, 4) for t in times["ladder_decrypt"]],
                  create_plus_decrypt_ms=round(both * 1e3, 4), speedup=round(med["ladder_decrypt"] / both, 3),
                  decrypt_speedup=round(med["ladder_decrypt"] / med["base_decrypt"], 3),
                  create_us_per_session=round(med["base_create"] * 1e6 / S, 3), table_bytes=S * 61440))
        h.close()
        for d in (d_a, d_A, d_ainv, d_st, d_st1, d_sc, d_ch, d_ct, d_lab, d_lab1):
            d.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join("%dx%d" % s for s in SHAPES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--sequential", type=int, default=8, help="S of the sequential one-session comparison (0: skip)")
    ap.add_argument("--base-shapes", default=None, nargs="?", const=",".join("%dx%d" % s for s in BASE_SHAPES),
                    help="time the receiver handle (gc_co_multi_base_*) at these shapes INSTEAD of the rows above")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    ctx = engine.Context(0)
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    if a.base_shapes:
        bench_base(ctx, a, emit)
    rng = np.random.default_rng(7)
    for S, per in [] if a.base_shapes else shapes_of(a.shapes):
        n = S * per
        a_host = rng.integers(0, 256, (S, 32), dtype=np.uint8)
        d_a = ctx.to_device(a_host)
        d_A, d_ainv, d_st = ctx.zeros((S, 64)), ctx.zeros((S, 64)), ctx.zeros(4, np.uint64)
        d_sc, d_ch = ctx.random_u8((n, 32), seed=1), ctx.random_u8(n, high=2, seed=2)
        d_w = ctx.random_u8((n, 32), seed=3)
        d_pts, d_ct, d_lab = ctx.zeros((n, 64)), ctx.zeros((n, 32)), ctx.zeros((n, 16))
        d_pts1, d_ct1, d_lab1, d_st1 = ctx.zeros((n, 64)), ctx.zeros((n, 32)), ctx.zeros((n, 16)), ctx.zeros(2, np.uint64)
        engine.co_multi_sender_setup_dev(ctx, d_a, S, d_A, d_ainv, d_st)
        ctx.sync()
        a0 = bytes(a_host[0])
        A0, AaInv0 = engine.co_sender_setup(a0)
        assert bytes(d_A.numpy()[0]) == bytes(A0) and bytes(d_ainv.numpy()[0]) == bytes(AaInv0)
        base = engine.CoBase(ctx, A0)
        sample = min(S, 64)

        def host_setups():
            for s in range(sample):
                engine.co_sender_setup(bytes(a_host[s]))

        pairs = {
            "setup": (lambda: engine.co_multi_sender_setup_dev(ctx, d_a, S, d_A, d_ainv, d_st), host_setups),
            "choices": (lambda: engine.co_multi_receiver_choices_dev(ctx, d_A, d_sc, d_ch, S, per, d_pts, d_st),
                        lambda: base.choices_dev(d_sc, d_ch, n, d_pts1)),
            "encrypt": (lambda: engine.co_multi_sender_encrypt_dev(ctx, d_a, d_ainv, d_pts, d_w, S, per, 0, d_ct, d_st),
                        lambda: engine.co_sender_encrypt_dev(ctx, a0, AaInv0, d_pts1, d_w, n, 0, d_ct1, d_st1)),
            "decrypt": (lambda: engine.co_multi_receiver_decrypt_dev(ctx, d_A, d_sc, d_ch, d_ct, S, per, 0, d_lab, d_st),
                        lambda: engine.co_receiver_decrypt_dev(ctx, A0, d_sc, d_ch, d_ct1, n, 0, d_lab1)),
        }
        ks = {name: tuple(calls_for(ctx, fn, a.window) for fn in fns) for name, fns in pairs.items()}
        times = {name: ([], []) for name in pairs}
        for _ in range(a.reps):  # alternating
            for name, fns in pairs.items():
                for side in (0, 1):
                    times[name][side].append(timed(ctx, fns[side], ks[name][side]))
        assert [int(v) for v in d_st.numpy()] == [0, (1 << 64) - 1, 0, (1 << 64) - 1]
        for name in pairs:
            multi, single = statistics.median(times[name][0]), statistics.median(times[name][1])
            if name == "setup":
                single *= S / sample
            emit(dict(bench="co_multi", kernel="multi_" + name, S=S, per=per, n=n, reps=a.reps, calls_per_window=list(ks[name]),
                      ms=round(multi * 1e3, 4), ms_all=[round(t * 1e3, 4) for t in times[name][0]],
                      single_ms=round(single * 1e3, 4), single_ms_all=[round(t * 1e3, 4) for t in times[name][1]],
                      single="S x gc_co_sender_setup (host, scaled from %d)" % sample if name == "setup" else "one session of n OTs",
                      ratio=round(multi / single, 3), us_per_session=round(multi * 1e6 / S, 3)))
        if a.sequential and S == a.sequential:
            As, ainvs = d_A.numpy(), d_ainv.numpy()

            def sender_seq():
                for s in range(S):
                    _, ai = engine.co_sender_setup(bytes(a_host[s]))
                    o = s * per
                    engine.co_sender_encrypt_dev(ctx, bytes(a_host[s]), ai, d_pts.ptr + 64 * o, d_w.ptr + 32 * o, per, 0,
                                                 d_ct1.ptr + 32 * o, d_st1)
                    ctx.sync()

            def receiver_seq():
                for s in range(S):
                    o = s * per
                    h = engine.CoBase(ctx, As[s])
                    h.choices_dev(d_sc.ptr + 32 * o, d_ch.ptr + o, per, d_pts1.ptr + 64 * o)
                    ctx.sync()
                    h.decrypt_dev(d_sc.ptr + 32 * o, d_ch.ptr + o, d_ct.ptr + 32 * o, per, 0, d_lab1.ptr + 16 * o)
                    ctx.sync()
                    h.close()

            def sender_multi():
                engine.co_multi_sender_setup_dev(ctx, d_a, S, d_A, d_ainv, d_st)
                ctx.sync()
                engine.co_multi_sender_encrypt_dev(ctx, d_a, d_ainv, d_pts, d_w, S, per, 0, d_ct, d_st)
                ctx.sync()

            def receiver_multi():
                engine.co_multi_receiver_choices_dev(ctx, d_A, d_sc, d_ch, S, per, d_pts1, d_st)
                ctx.sync()
                engine.co_multi_receiver_decrypt_dev(ctx, d_A, d_sc, d_ch, d_ct, S, per, 0, d_lab, d_st)
                ctx.sync()

            seq = {"sender": (sender_multi, sender_seq), "receiver": (receiver_multi, receiver_seq)}
            ks = {name: tuple(calls_for(ctx, fn, a.window) for fn in fns) for name, fns in seq.items()}
            times = {name: ([], []) for name in seq}
            for _ in range(a.reps):
                for name, fns in seq.items():
                    for side in (0, 1):
                        times[name][side].append(timed(ctx, fns[side], ks[name][side]))
            assert (d_ainv.numpy() == ainvs).all()
            for name in seq:
                multi, single = statistics.median(times[name][0]), statistics.median(times[name][1])
                emit(dict(bench="co_multi", kernel=name + "_sessions", S=S, per=per, reps=a.reps, calls_per_window=list(ks[name]),
                          multi_ms=round(multi * 1e3, 4), multi_ms_all=[round(t * 1e3, 4) for t in times[name][0]],
                          sequential_ms=round(single * 1e3, 4), sequential_ms_all=[round(t * 1e3, 4) for t in times[name][1]],
                          sequential_ms_per_session=round(single * 1e3 / S, 4), speedup=round(single / multi, 2)))
        base.close()
        for d in (d_a, d_A, d_ainv, d_st, d_sc, d_ch, d_w, d_pts, d_ct, d_lab, d_pts1, d_ct1, d_lab1, d_st1):
            d.close()
    ctx.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
