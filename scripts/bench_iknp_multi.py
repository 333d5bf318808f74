"""IKNP extension and COT pads, S sessions per call (gc_iknp_multi_*_dev, gc_cot_multi_*_dev) beside the one-session calls:
one JSON line per (call, S, per), everything in HBM.  The protocol is scripts/bench_co_multi.py's: a host clock around k calls
that end in gc_ctx_sync, k sized once (after a warm-up) so that a window lasts at least --window seconds; per-call time =
window / k; median over --reps windows, every rep reported; the three rows of a call alternate in one process.

  multi           the multi _dev call: iknp_receive, iknp_send, cot_send, cot_receive
  single_same_n   the one-session _dev call at n = S * per with ONE session's constants: the ratio says what per-item keys
                  and the key schedule in the lane cost (and, for long sessions, where the one-session form wins)
  sequential      what a caller does today for S sessions: create + _dev call + gc_ctx_sync + free per session (the COT
                  calls have no handle: call + gc_ctx_sync), timed on at most --sample sessions and scaled to S

Bytes per OT (the model of DESIGN.md § 12): IKNP sender labels 16 + u 16 + keys 16 * 128 / per, receiver the same with two
keys per column; COT send 16 + 32 + 32, receive 16 + 32 + 1.  `hbm_fraction` = bytes / time / 8 TB/s."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mpc_amd import engine  # noqa: E402
from mpc_amd.circuit import LABEL, WIRE  # noqa: E402
from scripts.bench_co import calls_for, timed  # noqa: E402

SHAPES = [(8, 128), (1024, 128), (1024, 127), (8192, 128), (1024, 512), (64, 16384)]
HBM_BYTES_PER_S = 8e12


def shapes_of(text):
    return [tuple(int(v) for v in s.split("x")) for s in text.split(",") if s]


def labels(rng, shape):
    out = np.zeros(shape, LABEL)
    out["d0"] = rng.integers(0, 1 << 64, shape, dtype=np.uint64)
    out["d1"] = rng.integers(0, 1 << 64, shape, dtype=np.uint64)
    return out


def u_bytes(n):
    return int(engine.lib().gc_iknp_u_bytes(n))


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

    rng = np.random.default_rng(12)
    for S, per in shapes_of(a.shapes):
        n = S * per
        cps = -(-per // 512)
        ub = u_bytes(per)
        sample = min(S, a.sample)
        base = np.zeros((S, 128), WIRE)
        base["l0"], base["l1"] = labels(rng, (S, 128)), labels(rng, (S, 128))
        deltas, seeds, k0 = labels(rng, S), labels(rng, S), base["l0"].copy()
        d_choice = ctx.random_u8(max(S * cps * 64, -(-n // 512) * 64 + 16), seed=1)
        d_u = ctx.random_u8(max(S * ub, -(-n // 512) * 8192), seed=2)
        d_lab, d_lab1 = ctx.zeros((n, 16)), ctx.zeros((n, 16))
        d_wires, d_pads, d_flags = ctx.random_u8((n, 32), seed=3), ctx.zeros((n, 32)), ctx.random_u8(n, high=2, seed=4)
        d_seeds, d_deltas = ctx.to_device(seeds.view(np.uint8)), ctx.to_device(deltas.view(np.uint8))
        m_rcv, m_snd = engine.IKNPMultiReceiver(ctx, base), engine.IKNPMultiSender(ctx, deltas, k0)
        s_rcv, s_snd = engine.IKNPReceiver(ctx, base[0]), engine.IKNPSender(ctx, (int(deltas[0]["d0"]), int(deltas[0]["d1"])), k0[0])
        seed0, delta0 = (int(seeds[0]["d0"]), int(seeds[0]["d1"])), (int(deltas[0]["d0"]), int(deltas[0]["d1"]))

        def seq_iknp_receive():
            for s in range(sample):
                h = engine.IKNPReceiver(ctx, base[s])
                h.receive_dev(d_choice.ptr + s * cps * 64, per, d_u.ptr + s * ub, d_lab1.ptr + 16 * s * per)
                ctx.sync()
                h.close()

        def seq_iknp_send():
            for s in range(sample):
                h = engine.IKNPSender(ctx, (int(deltas[s]["d0"]), int(deltas[s]["d1"])), k0[s])
                h.send_dev(d_u.ptr + s * ub, per, d_lab1.ptr + 16 * s * per)
                ctx.sync()
                h.close()

        def seq_cot_send():
            for s in range(sample):
                o = s * per
                engine.cot_send_pads_dev(ctx, seed0, delta0, d_lab.ptr + 16 * o, d_wires.ptr + 32 * o, per, d_pads.ptr + 32 * o)
                ctx.sync()

        def seq_cot_receive():
            for s in range(sample):
                o = s * per
                engine.cot_receive_unpad_dev(ctx, seed0, d_flags.ptr + o, d_pads.ptr + 32 * o, d_lab1.ptr + 16 * o, per)
                ctx.sync()

        key_bytes = 16.0 * 128 / per
        calls = {
            "iknp_receive": (lambda: m_rcv.receive_dev(d_choice, per, d_u, d_lab),
                             lambda: s_rcv.receive_dev(d_choice, n, d_u, d_lab1), seq_iknp_receive, 32 + 2 * key_bytes),
            "iknp_send": (lambda: m_snd.send_dev(d_u, per, d_lab), lambda: s_snd.send_dev(d_u, n, d_lab1), seq_iknp_send,
                          32 + key_bytes),
            "cot_send": (lambda: engine.cot_multi_send_pads_dev(ctx, d_seeds, d_deltas, d_lab, d_wires, S, per, d_pads),
                         lambda: engine.cot_send_pads_dev(ctx, seed0, delta0, d_lab, d_wires, n, d_pads), seq_cot_send, 80),
            "cot_receive": (lambda: engine.cot_multi_receive_unpad_dev(ctx, d_seeds, d_flags, d_pads, d_lab, S, per),
                            lambda: engine.cot_receive_unpad_dev(ctx, seed0, d_flags, d_pads, d_lab1, n), seq_cot_receive, 49),
        }
        ks = {name: tuple(calls_for(ctx, fn, a.window) for fn in fns[:3]) for name, fns in calls.items()}
        times = {name: ([], [], []) for name in calls}
        for _ in range(a.reps):  # alternating
            for name, fns in calls.items():
                for side in range(3):
                    times[name][side].append(timed(ctx, fns[side], ks[name][side]))
        for name, fns in calls.items():
            multi, single, seq = (statistics.median(t) for t in times[name])
            seq_scaled = seq * S / sample
            emit(dict(bench="iknp_multi", call=name, S=S, per=per, n=n, reps=a.reps, calls_per_window=list(ks[name]),
                      multi_ms=round(multi * 1e3, 4), multi_ms_all=[round(t * 1e3, 4) for t in times[name][0]],
                      single_same_n_ms=round(single * 1e3, 4), single_same_n_ms_all=[round(t * 1e3, 4) for t in times[name][1]],
                      sequential_ms=round(seq_scaled * 1e3, 4), sequential_sample=sample,
                      sequential_sample_ms_all=[round(t * 1e3, 4) for t in times[name][2]],
                      multi_over_single=round(multi / single, 3), sequential_over_multi=round(seq_scaled / multi, 2),
                      ns_per_ot=round(multi * 1e9 / n, 3), bytes_per_ot=round(fns[3], 2),
                      hbm_fraction=round(fns[3] * n / multi / HBM_BYTES_PER_S, 4)))
        for h in (m_rcv, m_snd, s_rcv, s_snd):
            h.close()
        for d in (d_choice, d_u, d_lab, d_lab1, d_wires, d_pads, d_flags, d_seeds, d_deltas):
            d.close()
    ctx.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
