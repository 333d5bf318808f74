"""Chou-Orlandi base OT throughput (gc_co_*_dev): one JSON line per (kernel, n), everything in HBM.

  choices   gc_co_receiver_choices_dev: B_i = b_i * G (+ A), one inversion, affine output
  encrypt   gc_co_sender_encrypt_dev: the on-curve check, S = a * B_i, T = S + AaInv, one shared inversion, two SHA-256
  decrypt   gc_co_receiver_decrypt_dev: b_i * A, one inversion, one SHA-256
  choices_tab, decrypt_tab   gc_co_base_choices_dev / gc_co_base_decrypt_dev: the same two loops with b_i * G and b_i * A
            summed from fixed-base window tables (mpc_amd/csrc/co_table.h) behind a session handle
  base_create   gc_co_base_create + gc_co_base_free of one session: A's table built on the host, uploaded, released (host
            clock; base_create_first is the first handle of the process, which also builds and uploads G's table)

The ladder rows are the yardstick of the table rows: same process, same buffers, alternating windows.  A `handle_vs_ladder`
line per n puts create + choices_tab + decrypt_tab beside choices + decrypt.

The points that encrypt reads are the ones choices wrote (seeded scalars), so every one is on the curve.

Timing: a host clock around k calls that end in gc_ctx_sync, k sized once (after a warm-up) so that a window lasts at least
--window seconds; per-call time = window / k; median over --reps windows, every rep reported.

Work model, from the code (mpc_amd/csrc/p256.h): Montgomery products per OT.  A doubling takes 8, a mixed addition 11, the
inversion 267 (255 squarings, 12 products), an affine conversion 6, the on-curve check 6.  The ladder is 256 doublings and
one addition per set bit of the scalar.  In encrypt the scalar is uniform: wt(a) additions for every lane.  In the receiver
kernels it is the lane's: a wave issues the addition on every step where ANY of its lanes has the bit set — all 256 for
random scalars — so `issued` counts 256 additions where `useful` counts 128.  The table forms make one addition per
window of w bits and no doubling: ceil(256 / w) additions issued (a wave skips one only if the digit is zero in all its
lanes), of which a lane's share 1 - 2^-w is useful; w = 4 for A, the library's kCoTabWidthG for G.  A product is 128 limb multiply-adds in the
CIOS form of vole_mont_mul (64 for a * b, 64 for q * p, of which the compiler folds the ones by the limbs 0 and 1 of p).
frac_mad_rate = issued products * 128 * n / time / (the card's v_mad_u64_u32 rate, measured in this run by
tools/mad_rate_ubench).
"""
import argparse
import json
import math
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mpc_amd import engine  # noqa: E402

SIZES = [1 << 10, 1 << 14, 1 << 17]
DBL, MADD, INV, AFFINE, ON_CURVE, LIMB_MADS = 8, 11, 267, 6, 6, 128
N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551


def tab_widths():
    """(w of G's table, w of A's table): the constexprs of mpc_amd/csrc/kernels.h that the library is built from"""
    text = open(os.path.join(ROOT, "mpc_amd", "csrc", "kernels.h")).read()
    return tuple(int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text).group(1))
                 for name in ("kCoTabWidthG", "kCoTabWidthA"))


def products(kernel, weight_a, widths=(4, 4)):
    """(useful, issued) Montgomery products per OT"""
    if kernel in ("choices_tab", "decrypt_tab"):
        w = widths[0] if kernel == "choices_tab" else widths[1]
        windows = -(-256 // w)
        tail = INV + AFFINE + (MADD if kernel == "choices_tab" else 0)
        return round(windows * MADD * (1 - 2.0 ** -w)) + tail, windows * MADD + tail
    if kernel == "encrypt":
        p = ON_CURVE + 256 * DBL + weight_a * MADD + MADD + 1 + INV + 2 + 2 * AFFINE
        return p, p
    tail = INV + AFFINE + (MADD if kernel == "choices" else 0)
    return 256 * DBL + 128 * MADD + tail, 256 * DBL + 256 * MADD + tail


def mad_rate():
    """lane-level 32 x 32 -> 64 multiply-adds per second of this card (tools/mad_rate_ubench.hip), measured now"""
    exe = os.path.join(ROOT, "tools", "mad_rate_ubench")
    if not os.path.exists(exe):
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "--offload-arch=gfx950", exe + ".hip", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout
    return json.loads(out.strip().splitlines()[-1])


def calls_for(ctx, fn, window):
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
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--create-reps", type=int, default=20)
    a = ap.parse_args()
    widths = tab_widths()
    rate = mad_rate()
    lines = [json.dumps(rate)]
    print(lines[0], flush=True)
    ctx = engine.Context(0)
    a_scalar = int.from_bytes(bytes(range(1, 33)), "big") % N
    weight_a = bin(a_scalar).count("1")
    A, AaInv = engine.co_sender_setup(a_scalar)
    t0 = time.perf_counter()
    base = engine.CoBase(ctx, A)  # the first handle of the process: G's table is built and uploaded here
    first_ms = (time.perf_counter() - t0) * 1e3

    def create():
        t0 = time.perf_counter()
        engine.CoBase(ctx, A).close()
        return time.perf_counter() - t0

    create()
    creates = [create() for _ in range(a.create_reps)]
    create_ms = statistics.median(creates) * 1e3
    for name, ms in (("base_create_first", first_ms), ("base_create", create_ms)):
        row = dict(bench="co", kernel=name, width_g=widths[0], width_a=widths[1], ms=round(ms, 4))
        if name == "base_create":
            row.update(reps=a.create_reps, ms_all=[round(t * 1e3, 4) for t in creates])
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    for n in [int(x) for x in a.sizes.split(",")]:
        d_sc, d_ch = ctx.random_u8((n, 32), seed=1), ctx.random_u8(n, high=2, seed=2)
        d_w = ctx.random_u8((n, 32), seed=3)
        d_pts, d_ct, d_lab, d_status = ctx.zeros((n, 64)), ctx.zeros((n, 32)), ctx.zeros((n, 16)), ctx.zeros(2, np.uint64)

        def choices():
            engine.co_receiver_choices_dev(ctx, A, d_sc, d_ch, n, d_pts)

        def encrypt():
            engine.co_sender_encrypt_dev(ctx, a_scalar, AaInv, d_pts, d_w, n, 0, d_ct, d_status)

        def decrypt():
            engine.co_receiver_decrypt_dev(ctx, A, d_sc, d_ch, d_ct, n, 0, d_lab)

        def choices_tab():
            base.choices_dev(d_sc, d_ch, n, d_pts)

        def decrypt_tab():
            base.decrypt_dev(d_sc, d_ch, d_ct, n, 0, d_lab)

        fns = {"choices": choices, "choices_tab": choices_tab, "encrypt": encrypt, "decrypt": decrypt, "decrypt_tab": decrypt_tab}
        ks = {name: calls_for(ctx, fn, a.window) for name, fn in fns.items()}
        times = {name: [] for name in fns}
        for _ in range(a.reps):  # alternating
            for name, fn in fns.items():
                times[name].append(timed(ctx, fn, ks[name]))
        assert int(d_status.numpy()[0]) == 0, "the choices kernel wrote a point that is not on the curve"
        meds = {}
        for name in fns:
            med = meds[name] = statistics.median(times[name])
            useful, issued = products(name, weight_a, widths)
            row = dict(bench="co", kernel=name, n=n, reps=a.reps, calls_per_window=ks[name], ms=round(med * 1e3, 4),
                       ms_all=[round(t * 1e3, 4) for t in times[name]], ot_per_s=round(n / med, 1),
                       mont_products_per_ot=useful, mont_products_issued_per_ot=issued, limb_mads_per_product=LIMB_MADS,
                       frac_mad_rate=round(issued * LIMB_MADS * n / med / rate["lane_mads_per_s"], 4))
            if name == "encrypt":
                row["weight_a"] = weight_a
            if name.endswith("_tab"):
                ladder = name[:-4]
                row.update(width=widths[0] if ladder == "choices" else widths[1], ladder_ms=round(meds[ladder] * 1e3, 4),
                           speedup=round(meds[ladder] / med, 3),
                           model_speedup=round(products(ladder, weight_a)[1] / issued, 3))
            line = json.dumps(row)
            print(line, flush=True)
            lines.append(line)
        ladder_ms = (meds["choices"] + meds["decrypt"]) * 1e3
        handle_ms = create_ms + (meds["choices_tab"] + meds["decrypt_tab"]) * 1e3
        lines.append(json.dumps(dict(bench="co", kernel="handle_vs_ladder", n=n, ladder_ms=round(ladder_ms, 4),
                                     handle_ms_with_create=round(handle_ms, 4), speedup=round(ladder_ms / handle_ms, 3))))
        print(lines[-1], flush=True)
        for d in (d_sc, d_ch, d_w, d_pts, d_ct, d_lab, d_status):
            d.close()
    base.close()
    ctx.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
