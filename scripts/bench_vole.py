"""Packed-IKNP VOLE throughput (gc_vole_*): one JSON line per (modulus, m), everything in HBM.

  sender    gc_vole_sender_mul_dev: per label one AES-128 key schedule, two AES-CTR blocks, the reduction of the pad (r),
            x * y mod p and one modular sum (PRODUCTS: the Montgomery products this takes per element)
  receiver  gc_vole_receiver_reduce_dev: one reduction per element
  pipeline  gc_iknp_receive_dev (all-false choices) -> gc_iknp_send_dev -> the two VOLE calls
  rot       the yardstick: gc_rot_send_dev at n = m (k_cot_dual<1, 2>: the same per-lane AES-128 key schedule and two
            blocks per element, then two XORs), timed in the same process, alternating with the sender

Timing: a host clock around k calls that end in gc_ctx_sync, k sized once (after a warm-up) so that a window lasts at least
--window seconds; per-call time = window / k; median over --reps windows, every rep reported.  m = 1 .. 1024 are the sizes
of vole/vole_bench_test.go; at those sizes the figures are launch and synchronisation cost, not kernel work.

Byte model per element: sender 16 (label) + 32 (x) + 32 (y) read, 32 (r) + 32 (u) written = 144 B; receiver 32 + 32 = 64 B;
rot 16 read + 32 written = 48 B.  frac_8TBps = bytes * m / time / 8e12.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mpc_amd import engine  # noqa: E402

HBM_BPS = 8e12
MODULI = {"p256": int("ffffffff00000001000000000000000000000000ffffffffffffffffffffffff", 16), "2^255-19": (1 << 255) - 19}
# Montgomery products per element (vole_mod.h): x * y mod p takes 2; a reduction takes 2 for p < 2^255 and none for
# p >= 2^255 (one conditional subtraction)
PRODUCTS = {"p256": {"sender": 2, "receiver": 0}, "2^255-19": {"sender": 4, "receiver": 2}}
SIZES = [1, 8, 64, 256, 1024, 1 << 16, 1 << 20, 1 << 24]
BYTES = {"sender": 144, "receiver": 64, "rot": 48}


def calls_for(ctx, fn, window):
    """k such that k calls + one sync last at least `window` seconds (after one warm-up call)"""
    fn()
    ctx.sync()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    dt = max(time.perf_counter() - t0, 1e-6)
    return max(1, math.ceil(window / dt))


def timed(ctx, fn, k):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=",".join(str(m) for m in SIZES))
    ap.add_argument("--modulus", default="p256", choices=sorted(MODULI))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    from tests.test_gpu_ot import base_setup
    ctx = engine.Context(0)
    base, delta, k0 = base_setup("bench-vole")
    seed = (0x0123456789ABCDEF, 0xFEDCBA9876543210)
    P = MODULI[a.modulus]
    lines = []
    for m in [int(x) for x in a.sizes.split(",")]:
        d_lab = ctx.random_u8((m, 16), seed=1)
        d_x, d_y = ctx.random_u8((m, 32), seed=2), ctx.random_u8((m, 32), seed=3)
        d_r, d_u, d_us, d_w = ctx.zeros((m, 32)), ctx.zeros((m, 32)), ctx.zeros((m, 32)), ctx.zeros((m, 32))
        chunks = (m + 511) // 512
        d_c, d_iu, d_lr, d_ls = ctx.zeros(chunks * 64), ctx.zeros(chunks * 8192), ctx.zeros((m, 16)), ctx.zeros((m, 16))
        rx, tx = engine.IKNPReceiver(ctx, base), engine.IKNPSender(ctx, delta, k0)

        def sender():
            engine.vole_sender_mul_dev(ctx, P, d_lab, d_x, d_y, m, d_r, d_u)

        def receiver():
            engine.vole_receiver_reduce_dev(ctx, P, d_u, m, d_us)

        def rot():
            engine.rot_send_dev(ctx, seed, delta, d_lab, m, d_w)

        def pipeline():
            rx.receive_dev(d_c, m, d_iu, d_lr)
            tx.send_dev(d_iu, m, d_ls)
            engine.vole_sender_mul_dev(ctx, P, d_ls, d_x, d_y, m, d_r, d_u)
            engine.vole_receiver_reduce_dev(ctx, P, d_u, m, d_us)

        fns = {"sender": sender, "rot": rot, "receiver": receiver, "pipeline": pipeline}
        ks = {name: calls_for(ctx, fn, a.window) for name, fn in fns.items()}
        times = {name: [] for name in fns}
        for _ in range(a.reps):  # alternating: sender, yardstick, receiver, pipeline
            for name, fn in fns.items():
                times[name].append(timed(ctx, fn, ks[name]))
        row = dict(bench="vole", modulus=a.modulus, m=m, mont_products_per_elem=PRODUCTS[a.modulus], reps=a.reps, calls_per_window=ks)
        for name in fns:
            med = statistics.median(times[name])
            row[name + "_ms"] = round(med * 1e3, 6)
            row[name + "_ms_all"] = [round(t * 1e3, 6) for t in times[name]]
            row[name + "_elems_per_s"] = round(m / med, 1)
            if name in BYTES:
                row[name + "_frac_8TBps"] = round(BYTES[name] * m / med / HBM_BPS, 4)
        row["sender_over_rot"] = round(row["sender_ms"] / row["rot_ms"], 3)
        row["bytes_per_elem"] = BYTES
        line = json.dumps(row)
        print(line, flush=True)
        lines.append(line)
        rx.close()
        tx.close()
        for d in (d_lab, d_x, d_y, d_r, d_u, d_us, d_w, d_c, d_iu, d_lr, d_ls):
            d.close()
    ctx.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
