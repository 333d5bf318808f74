"""GMW party engine throughput (gc_gmw_*): P = 2 and 3 parties of aes_128 in one process, one ctx each, on one device,
messages passed device-side.  One JSON line per (P, batch) config.

Online pass: every party steps round by round; after each round the host waits for every party's stream (the exchange) and
the messages are copied device-to-device into the next round's peer buffers.  pass_ms is the wall time of one whole pass of
all P parties (they share the device), median of --reps.  The online kernels do the same work whatever the triple values,
so the timed passes run on zero triples; triple generation (real bit-COT, gc_iknp_*_bits_dev, plus the four folds) is timed
on its own, on min(TW * batch, --cot-words) words per party, and reported as triples_ms_per_word.

Byte model per party per pass (u64 words, bw = ceil(batch / 64) instance words):
  shares   = 8 bw (reads + writes of slots): free gate 2 + 1 (INV 1 + 1), AND 2 reads (open) + 1 write (close),
             inputs 1 write, outputs 1 read
  triples  = 8 batch TW 5 (a, b on open; a, b, c on close)
  messages = 8 batch sum(w) 2 (4 written: own copy + msg_out; 2 + 2 npeers read on close)
  io       = 8 batch (ceil(ninputs/64) + ceil(noutputs/64))
"""
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
from mpc_amd.circuit import AND, INV, parse_file  # noqa: E402

HBM_BPS = 8e12


def byte_model(c, info, batch, P):
    bw = (batch + 63) // 64
    ops = c.Gates["op"]
    n_and = int((ops == AND).sum())
    n_inv = int((ops == INV).sum())
    n_free2 = len(ops) - n_and - n_inv
    slot_words = 3 * n_free2 + 2 * n_inv + 3 * n_and + c.num_inputs + c.num_outputs
    _, _, _, wl = engine.gmw_plan_describe(c.Gates, c.NumWires, c.num_inputs, c.num_outputs)
    sw = int(wl.sum())
    shares = 8 * bw * slot_words
    triples = 8 * batch * info.triple_words * 5
    messages = 8 * batch * sw * (4 + 2 + 2 * (P - 1))
    io = 8 * batch * ((c.num_inputs + 63) // 64 + (c.num_outputs + 63) // 64)
    return dict(shares=shares, triples=triples, messages=messages, io=io, total=shares + triples + messages + io)


def run_pass(parties, ctxs, d_in, d_t, xch, ws, batch):
    P = len(parties)
    for g, x, t in zip(parties, d_in, d_t):
        g.set_inputs_dev(x)
        g.set_triples_dev(*t)
    r = 0
    while True:
        w_prev = ws[r - 1] if r else 0
        w = ws[r] if r < len(ws) else 0
        src, dst = xch[(r + 1) & 1], xch[r & 1]
        for p, g in enumerate(parties):
            peers = (src + (p + 1) * 2 * w_prev * batch * 8) if w_prev else None
            g.step_dev(peers, (dst + p * 2 * w * batch * 8) if w else None)
        for cx in ctxs:
            cx.sync()  # the exchange: every party's message is out
        if not w:
            return
        slot = 2 * w * batch * 8
        for k in range(P - 1):
            dst.copy_from(dst + k * slot, slot, offset=(P + k) * slot)
        ctxs[0].sync()
        r += 1


def time_triples(ctx, P, words):
    """real bit-COT for every ordered pair + the folds, on `words` words per party; returns ms"""
    from tests.test_gpu_ot import base_setup
    import oracle
    n = 64 * words
    d_a = [ctx.random_u8(words * 8, seed=1 + p) for p in range(P)]
    d_b = [ctx.random_u8(words * 8, seed=11 + p) for p in range(P)]
    d_c = [ctx.zeros(words * 8) for _ in range(P)]
    d_u = ctx.zeros(((n + 511) // 512) * 8192)
    d_uv, d_s, d_r = ctx.zeros(words * 8), ctx.zeros(words * 8), ctx.zeros(words * 8)
    pairs = []
    for s in range(P):
        for r in range(P):
            if s != r:
                base, delta, k0 = base_setup("bench-gmw-%d-%d" % (s, r))
                pairs.append((s, r, engine.IKNPReceiver(ctx, base), engine.IKNPSender(ctx, delta, k0), oracle.label_bit(delta, 0)))
    ctx.sync()
    t0 = time.perf_counter()
    for p in range(P):
        engine.gmw_triples_local_dev(ctx, d_a[p], d_b[p], d_c[p], words)
    for s, r, rcv, snd, dbit in pairs:
        rcv.receive_bits_dev(d_b[r], n, d_u, d_r)
        snd.send_bits_dev(d_u, n, d_s)
        engine.gmw_triples_sender_u_dev(ctx, dbit, d_a[s], d_uv, words)
        engine.gmw_triples_sender_fold_dev(ctx, d_s, d_uv, d_b[r], d_c[s], words)
        engine.gmw_triples_receiver_fold_dev(ctx, d_r, d_c[r], words)
    ctx.sync()
    ms = (time.perf_counter() - t0) * 1e3
    for _, _, rcv, snd, _ in pairs:
        rcv.close()
        snd.close()
    for x in d_a + d_b + d_c + [d_u, d_uv, d_s, d_r]:
        x.close()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parties", default="2,3")
    ap.add_argument("--batches", default="1,64,4096,65536,1048576")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cot-words", type=int, default=1 << 20)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    c = parse_file(os.path.join(ROOT, "tests", "golden", "aes_128.gcf"))
    lines = []
    for P in [int(x) for x in a.parties.split(",")]:
        ctxs = [engine.Context(0) for _ in range(P)]
        for batch in [int(x) for x in a.batches.split(",")]:
            parties = [engine.Gmw(ctxs[p], c, P, p, batch) for p in range(P)]
            info = parties[0].info
            ws = [int(w) for w in engine.gmw_plan_describe(c.Gates, c.NumWires, c.num_inputs, c.num_outputs)[3] if w]
            in_bytes = ((c.num_inputs + 63) // 64) * batch * 8
            d_in = [ctxs[p].random_u8(in_bytes, seed=p) for p in range(P)]
            d_t = [[ctxs[p].zeros(info.triple_words * batch * 8) for _ in range(3)] for p in range(P)]
            xch = [ctxs[0].zeros((2 * P - 1) * 2 * max(ws) * batch * 8) for _ in range(2)]
            run_pass(parties, ctxs, d_in, d_t, xch, ws, batch)  # warm-up
            times = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                run_pass(parties, ctxs, d_in, d_t, xch, ws, batch)
                times.append((time.perf_counter() - t0) * 1e3)
            ms = statistics.median(times)
            bm = byte_model(c, info, batch, P)
            tw_words = min(info.triple_words * batch, a.cot_words)
            tms = time_triples(ctxs[0], P, tw_words)
            row = dict(bench="gmw_aes_128", parties=P, batch=batch, pass_ms=round(ms, 3), pass_ms_all=[round(t, 3) for t in times],
                       launches_per_pass=parties[0].last_launches, and_levels=info.n_and_levels,
                       bytes_per_party=bm, frac_8TBps=round(P * bm["total"] / (ms * 1e-3) / HBM_BPS, 4),
                       gate_inst_per_s_per_party=round(c.NumGates * batch / (ms * 1e-3), 1),
                       and_inst_per_s_per_party=round(info.n_and * batch / (ms * 1e-3), 1),
                       triples=dict(words_per_party=tw_words, ms=round(tms, 3), ms_per_mword=round(tms / tw_words * 1e6, 3)),
                       online_triples="zero words (data-independent work)")
            line = json.dumps(row)
            print(line, flush=True)
            lines.append(line)
            for g in parties:
                g.close()
            for x in d_in + [y for t in d_t for y in t] + xch:
                x.close()
        for cx in ctxs:
            cx.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
