"""Bit-COT for S sessions per call (gc_iknp_multi_*_bits_dev) and a GMW triple batch over all peers (gc_gmw_triples_multi_*)
beside what a caller had before: one JSON line per row, everything in HBM.  The protocol is scripts/bench_iknp_multi.py's: a
host clock around k calls that end in one gc_ctx_sync, k sized once (after a warm-up) so that a window lasts at least
--window seconds; per-call time = window / k; median over --reps windows, every rep reported; the rows of a shape alternate
in one process.

Rows of bench = "iknp_multi_bits", per (call, S, per):
  multi        the multi _dev call: receive_bits (per-session choice rows, stride W), send_bits
  sequential   one one-session gc_iknp_receive_bits_dev / gc_iknp_send_bits_dev call per session on the same base labels,
               handles created and their workspaces grown before the clock starts: the path without this feature
Rows of bench = "gmw_triples_multi", per (P, words): every party's whole batch, all P parties on one device
  multi        per party: c = a & b, ONE receive-bits with the shared b (stride 0), ONE send-bits, u = a ^ Delta, the two
               folds — six launches whatever P is.  A party's sender reads the u-matrices where another party's receiver
               left them, [P - 1][u_bytes] as a block: which peer's bytes they are does not change the work, and the
               regrouping by peer is the transport's
  pairs        scripts/bench_gmw.py: time_triples' sequence, per ordered pair: two one-session bit-COT calls and three folds
The row at 2^20 words also carries bench_gmw.time_triples itself (one untimed-warm-up call and one timed, as bench_gmw
reports it).

Bytes per OT (the model of DESIGN.md § 14): receiver 16 of u out + 32 * 128 / per of keys + 2 / 8 (choice in, result out);
sender at most 3 / 8 (u column 0 in, result out, 16 / per of key).  `hbm_fraction` = bytes / time / 8 TB/s; `lds_fraction` for
the receiver = 256 AES blocks per 128 OTs x 200 table look-ups (160 of the rounds + 40 of the key schedule in the lane) over
the LDS array's rate of DESIGN.md § 4 (0.98 ns per wave-load per CU)."""
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

SHAPES = [(1, 8192), (4, 8192), (15, 8192), (1, 1 << 22), (4, 1 << 24), (1, 1 << 26)]
TRIPLES = [(2, 128), (5, 128), (2, 1 << 20)]
HBM_BYTES_PER_S = 8e12
LDS_LOOKUPS_PER_S = 256 * 64 / 0.98e-9  # 0.98 ns per wave-load per CU, 256 CUs


def pairs_of(text):
    return [tuple(int(v) for v in s.split("x")) for s in text.split(",") if s]


def labels(rng, shape):
    out = np.zeros(shape, LABEL)
    out["d0"] = rng.integers(0, 1 << 64, shape, dtype=np.uint64)
    out["d1"] = rng.integers(0, 1 << 64, shape, dtype=np.uint64)
    return out


def u_bytes(n):
    return int(engine.lib().gc_iknp_u_bytes(n))


def tup(l):
    return int(l["d0"]), int(l["d1"])


def sessions(rng, S):
    base = np.zeros((S, 128), WIRE)
    base["l0"], base["l1"] = labels(rng, (S, 128)), labels(rng, (S, 128))
    deltas = labels(rng, S)
    deltas["d0"] |= np.uint64(1)  # every sender session reads its u bytes: the dearer case
    return base, deltas, base["l1"].copy()  # (k0 need not follow delta for a timing)


def stats(ts):
    return round(statistics.median(ts) * 1e3, 4), [round(t * 1e3, 4) for t in ts]


def bench_calls(ctx, rng, S, per, a, emit):
    W, ub = -(-per // 64), u_bytes(per)
    base, deltas, k0 = sessions(rng, S)
    d_ch = ctx.random_u8(S * W * 8, seed=1)
    d_u = ctx.random_u8(S * ub, seed=2)
    d_res, d_res1 = ctx.zeros(S * W * 8), ctx.zeros(S * W * 8)
    m_rcv, m_snd = engine.IKNPMultiReceiver(ctx, base), engine.IKNPMultiSender(ctx, deltas, k0)
    s_rcv = [engine.IKNPReceiver(ctx, base[s]) for s in range(S)]
    s_snd = [engine.IKNPSender(ctx, tup(deltas[s]), k0[s]) for s in range(S)]

    def seq_receive():
        for s in range(S):
            s_rcv[s].receive_bits_dev(d_ch.ptr + 8 * s * W, per, d_u.ptr + s * ub, d_res1.ptr + 8 * s * W)

    def seq_send():
        for s in range(S):
            s_snd[s].send_bits_dev(d_u.ptr + s * ub, per, d_res1.ptr + 8 * s * W)

    n = S * per
    calls = {
        "receive_bits": (lambda: m_rcv.receive_bits_dev(d_ch, W, per, d_u, d_res), seq_receive, 16 + 32 * 128 / per + 2 / 8),
        "send_bits": (lambda: m_snd.send_bits_dev(d_u, per, d_res), seq_send, 2 / 8 + 16 / per),
    }
    ks = {name: tuple(calls_for(ctx, fn, a.window) for fn in fns[:2]) for name, fns in calls.items()}
    times = {name: ([], []) for name in calls}
    for _ in range(a.reps):  # alternating
        for name, fns in calls.items():
            for side in range(2):
                times[name][side].append(timed(ctx, fns[side], ks[name][side]))
    for name, fns in calls.items():
        (multi, multi_all), (seq, seq_all) = stats(times[name][0]), stats(times[name][1])
        row = dict(bench="iknp_multi_bits", call=name, S=S, per=per, n=n, reps=a.reps, calls_per_window=list(ks[name]),
                   multi_ms=multi, multi_ms_all=multi_all, sequential_ms=seq, sequential_ms_all=seq_all,
                   sequential_over_multi=round(seq / multi, 2), ns_per_ot=round(multi * 1e6 / n, 4),
                   bytes_per_ot=round(fns[2], 4), hbm_fraction=round(fns[2] * n / (multi * 1e-3) / HBM_BYTES_PER_S, 5))
        if name == "receive_bits":
            row["lds_fraction"] = round(n / 128 * 256 * 200 / (multi * 1e-3) / LDS_LOOKUPS_PER_S, 4)
        emit(row)
    for h in [m_rcv, m_snd] + s_rcv + s_snd:
        h.close()
    for d in (d_ch, d_u, d_res, d_res1):
        d.close()


def bench_triples(ctx, rng, P, words, a, emit):
    n, S = 64 * words, P - 1
    ub = u_bytes(n)
    d_a = [ctx.random_u8(words * 8, seed=1 + p) for p in range(P)]
    d_b = [ctx.random_u8(words * 8, seed=11 + p) for p in range(P)]
    d_c = [ctx.zeros(words * 8) for _ in range(P)]
    # multi: one handle per role and party over its P - 1 peers
    rcvs, snds = [], []
    for p in range(P):
        base, deltas, k0 = sessions(rng, S)
        rcvs.append(engine.IKNPMultiReceiver(ctx, base))
        snds.append(engine.IKNPMultiSender(ctx, deltas, k0))
    d_um = [ctx.zeros(S * ub) for _ in range(P)]
    d_r, d_s, d_uv = ctx.zeros(S * words * 8), ctx.zeros(S * words * 8), ctx.zeros(S * words * 8)
    d_v = ctx.random_u8(S * words * 8, seed=31)

    def multi():
        for p in range(P):
            engine.gmw_triples_local_dev(ctx, d_a[p], d_b[p], d_c[p], words)
            rcvs[p].receive_bits_dev(d_b[p], 0, n, d_um[p], d_r)
            engine.gmw_triples_multi_receiver_fold_dev(ctx, d_r, d_c[p], S, words)
        for p in range(P):
            snds[p].send_bits_dev(d_um[(p + 1) % P], n, d_s)
            engine.gmw_triples_multi_sender_u_dev(snds[p], d_a[p], d_uv, words)
            engine.gmw_triples_multi_sender_fold_dev(ctx, d_s, d_uv, d_v, d_c[p], S, words)

    # pairs: bench_gmw.time_triples' sequence on one-session handles
    d_u1 = ctx.zeros(ub)
    d_uv1, d_s1, d_r1 = ctx.zeros(words * 8), ctx.zeros(words * 8), ctx.zeros(words * 8)
    pairs = []
    for s in range(P):
        for r in range(P):
            if s != r:
                base, deltas, k0 = sessions(rng, 1)
                pairs.append((s, r, engine.IKNPReceiver(ctx, base[0]), engine.IKNPSender(ctx, tup(deltas[0]), k0[0])))

    def by_pairs():
        for p in range(P):
            engine.gmw_triples_local_dev(ctx, d_a[p], d_b[p], d_c[p], words)
        for s, r, rcv, snd in pairs:
            rcv.receive_bits_dev(d_b[r], n, d_u1, d_r1)
            snd.send_bits_dev(d_u1, n, d_s1)
            engine.gmw_triples_sender_u_dev(ctx, 1, d_a[s], d_uv1, words)
            engine.gmw_triples_sender_fold_dev(ctx, d_s1, d_uv1, d_b[r], d_c[s], words)
            engine.gmw_triples_receiver_fold_dev(ctx, d_r1, d_c[r], words)

    fns = (multi, by_pairs)
    ks = tuple(calls_for(ctx, fn, a.window) for fn in fns)
    times = ([], [])
    for _ in range(a.reps):
        for side in range(2):
            times[side].append(timed(ctx, fns[side], ks[side]))
    (m, m_all), (q, q_all) = stats(times[0]), stats(times[1])
    row = dict(bench="gmw_triples_multi", parties=P, words=words, reps=a.reps, calls_per_window=list(ks),
               multi_ms=m, multi_ms_all=m_all, pairs_ms=q, pairs_ms_all=q_all, pairs_over_multi=round(q / m, 2),
               multi_ms_per_party=round(m / P, 4), pairs_ms_per_party=round(q / P, 4),
               launches_per_party=dict(multi=6, pairs=1 + 8 * (P - 1)))
    if words >= 1 << 20:
        from scripts.bench_gmw import time_triples
        time_triples(ctx, P, words)  # its handles grow their workspaces in the first call
        row["bench_gmw_time_triples_ms"] = round(time_triples(ctx, P, words), 3)
    emit(row)
    for h in rcvs + snds + [x for pr in pairs for x in pr[2:]]:
        h.close()
    for d in d_a + d_b + d_c + d_um + [d_r, d_s, d_uv, d_v, d_u1, d_uv1, d_s1, d_r1]:
        d.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join("%dx%d" % s for s in SHAPES), help="S x per of the call rows")
    ap.add_argument("--triples", default=",".join("%dx%d" % s for s in TRIPLES), help="P x words of the batch rows")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    ctx = engine.Context(0)
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    rng = np.random.default_rng(14)
    for S, per in pairs_of(a.shapes):
        bench_calls(ctx, rng, S, per, a, emit)
    for P, words in pairs_of(a.triples):
        bench_triples(ctx, rng, P, words, a, emit)
    ctx.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
