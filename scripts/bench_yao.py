#!/usr/bin/env python
"""circuit.Garbler / circuit.Evaluator for S sessions per call (gc_yao_*_dev) on aes_128 with 32-byte keys: what the
messages cost next to the keyed passes, and M1 out / M1 in against the table egress / ingest the library had before.

The forms of a group alternate in one process, each with an untimed pass first; a timed window lies between two gc_ctx_sync
on the host clock and is repeated until it has lasted --window seconds; per form the median of --reps windows is reported,
and the windows themselves.

  send     gc_yao_garbler_send_dev: the keyed garble pass and M1 out
  garble   gc_batch_garble_keyed on the handle's batch: the pass alone         M1 out = send - garble, window by window
  egress   gc_batch_egress_tables on the same batch: the tables alone, no key, no labels (the call before this one)
  accept   gc_yao_evaluator_accept_dev: M1 in
  ingest   gc_batch_ingest_tables on the evaluator's batch, from the egress buffer
  eval     gc_yao_evaluator_eval_dev: the OT's labels in, the keyed eval pass, M2 out
  pass     gc_batch_set_input_range + gc_batch_eval_keyed on the same batch    M2 out = eval - pass
  result   gc_yao_garbler_result_dev: M2 in, M3 out
  parse    gc_yao_evaluator_result_dev: M3 in

The byte model of M1 out / M1 in is table bytes read (written) plus message bytes written (read), against 8 TB/s.  --trace
runs the six calls a few times at the first S and nothing else, for a kernel trace taken in a run of its own.  GC_YAO_TILE /
GC_YAO_PIECE choose another piece geometry; the row records what ran (profiles/yao_geometry.jsonl: --S 1024 --reps 3 --append).

    python scripts/bench_yao.py --S 64 256 1024 --out profiles/yao_bench.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mpc_amd import engine, parse_file  # noqa: E402

NG = NE = 128
KEYLEN = 32
HBM = 8e12


class Bench:
    def __init__(self, ctx, dc, S, seed=1):
        self.ctx, self.dc, self.S = ctx, dc, S
        rng = np.random.default_rng(seed)
        rb = lambda *shape: rng.integers(0, 256, shape, dtype=np.uint8)
        self.h = {"keys": rb(S, KEYLEN), "rnd": rb(S, 16 * (1 + NG + NE)), "gbits": rb(S, NG) & 1, "ebits": rb(S, NE) & 1}
        self.d = {k: ctx.to_device(v) for k, v in self.h.items()}
        self.gb, self.ev = engine.YaoGarbler(dc, NG, NE, KEYLEN, S), engine.YaoEvaluator(dc, NG, NE, KEYLEN, S)
        self.len, self.stride = self.gb.len, self.gb.stride
        z = ctx.zeros
        self.slots = [z(S * st) for st in self.stride]
        self.d_v, self.d_len3, self.d_gbits, self.d_ebits = z(4 * S), z(4 * S), z(S * self.gb.bits_bytes), z(S * self.gb.bits_bytes)
        self.d_wires, self.d_labels = z(32 * S * NE), z(16 * S * NE)
        self.wire_stride = (dc.tables_wire_bytes + 15) // 16 * 16
        self.d_wire, self.d_bad = z(S * self.wire_stride), z(16)

    def send(self):
        self.gb.send_dev(self.d["keys"], self.d["rnd"], self.d["gbits"], self.slots[0], self.stride[0])

    def garble(self):
        self.gb.batch.garble_keyed(self.d["keys"], KEYLEN, self.d["rnd"])

    def egress(self):
        self.gb.batch.egress_tables(self.d_wire, self.wire_stride)

    def accept(self):
        self.ev.accept_dev(self.slots[0], self.stride[0], self.d_v)

    def ingest(self):
        self.ev.batch.ingest_tables(self.d_wire, self.wire_stride, self.d_bad)

    def eval(self):
        self.ev.eval_dev(self.d_labels, self.slots[1], self.stride[1], self.d_v)

    def eval_pass(self):
        self.ev.batch.set_input_range(NG, NE, self.d_labels)
        self.ev.batch.eval_keyed(self.d["keys"], KEYLEN, self.ev.batch)

    def result(self):
        self.gb.result_dev(self.slots[1], self.stride[1], self.slots[2], self.stride[2], self.d_len3, self.d_gbits, self.d_v)

    def parse(self):
        self.ev.result_dev(self.slots[2], self.stride[2], self.d_ebits, self.d_v)

    def chain(self):
        """one whole session chain with the OT in the clear; checks the decoded bits against the plaintext circuit"""
        S = self.S
        self.send()
        self.gb.ot_wires_dev(self.d_wires)
        w = self.d_wires.download(engine.WIRE, (S, NE))
        self.d_labels.upload(np.where(self.h["ebits"].astype(bool), w["l1"], w["l0"]))
        self.accept()
        assert not self.d_v.download(np.uint32, (S,)).any()
        self.eval()
        self.result()
        assert not self.d_v.download(np.uint32, (S,)).any()
        self.parse()
        assert not self.d_v.download(np.uint32, (S,)).any()
        got = self.d_gbits.download(np.uint8, (S, self.gb.bits_bytes))
        assert (got == self.d_ebits.download(np.uint8, (S, self.gb.bits_bytes))).all()
        bits = np.concatenate([self.h["gbits"][0], self.h["ebits"][0]])
        want = self.dc.c.compute_bits(bits)[self.dc.c.NumWires - self.dc.c.num_outputs:]
        assert (np.unpackbits(got[0], bitorder="little")[:len(want)] == want).all(), "session 0 does not decode to the circuit's result"
        # the egress buffer for the ingest form, and the tables in M1 are those bytes
        self.egress()
        wire = self.d_wire.download(np.uint8, (S, self.wire_stride))[:, :self.dc.tables_wire_bytes]
        m1 = self.slots[0].download(np.uint8, (S, self.stride[0]))
        assert (m1[:, 4 + KEYLEN:4 + KEYLEN + wire.shape[1]] == wire).all(), "M1's tables differ from gc_batch_egress_tables"

    def close(self):
        self.gb.close(), self.ev.close()


def window_ms(ctx, fn, window):
    """the time of one fn() in ms, over a window of at least `window` seconds between two syncs (the calls take tens of
    microseconds: the stream is waited for, and the clock read, after every eighth)"""
    n = 0
    ctx.sync()
    t0 = time.perf_counter()
    while True:
        fn()
        n += 1
        if n % 8 == 0:
            ctx.sync()
            dt = time.perf_counter() - t0
            if dt >= window:
                return 1e3 * dt / n


def timed(ctx, fns, window, reps):
    """the forms alternate window by window; per form its `reps` windows"""
    per = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            per[k].append(window_ms(ctx, fn, window))
    return [np.array(w) for w in per]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add the rows to --out (a sweep over GC_YAO_TILE / GC_YAO_PIECE)")
    ap.add_argument("--trace", action="store_true", help="the six calls and the two parent calls alone, three times at the first S")
    args = ap.parse_args()
    circ = parse_file(os.path.join(ROOT, "tests", "golden", "aes_128.gcf"))
    ctx = engine.Context(0)
    dc = engine.DeviceCircuit(ctx, circ)
    tile, piece = engine.yao_kernel_shape()
    rows = []
    r4 = lambda a: [round(float(x), 4) for x in a]
    med = lambda a: round(float(np.median(a)), 4)
    for S in args.S:
        b = Bench(ctx, dc, S)
        b.chain()  # one untimed pass of everything, checked
        b.ingest(), b.eval_pass()
        ctx.sync()
        if args.trace:
            for _ in range(3):
                b.send(), b.egress(), b.accept(), b.ingest(), b.eval(), b.result(), b.parse()
            ctx.sync()
            print("trace pass done: S = %d" % S)
            b.close()
            break
        send, garble, egress = timed(ctx, (b.send, b.garble, b.egress), args.window, args.reps)
        b.send()
        garble_ms = b.gb.batch.last_ms
        accept, ingest = timed(ctx, (b.accept, b.ingest), args.window, args.reps)
        ev, ev_pass = timed(ctx, (b.eval, b.eval_pass), args.window, args.reps)
        eval_ms = b.ev.batch.last_ms
        result, parse = timed(ctx, (b.result, b.parse), args.window, args.reps)
        m1_out, m2_out = send - garble, ev - ev_pass
        table_bytes, len1 = 16 * dc.info.slab_rows * S, b.len[0]
        model = table_bytes + len1 * S
        frac = lambda ms: round(model / (ms * 1e-3) / HBM, 4)
        row = {"bench": "yao", "circuit": "aes_128", "keylen": KEYLEN, "S": S, "tile": tile, "piece_bytes": piece, "len1": len1,
               "m1_bytes_moved": model,
               "m1_out_ms": med(m1_out), "egress_ms": med(egress), "m1_out_windows_ms": r4(m1_out), "egress_windows_ms": r4(egress),
               "egress_spread_ms": round(float(egress.max() - egress.min()), 4), "m1_out_vs_egress": round(float(np.median(egress) / np.median(m1_out)), 2),
               "m1_out_hbm_fraction": frac(np.median(m1_out)), "egress_hbm_fraction": frac(np.median(egress)),
               "m1_in_ms": med(accept), "ingest_ms": med(ingest), "m1_in_windows_ms": r4(accept), "ingest_windows_ms": r4(ingest),
               "ingest_spread_ms": round(float(ingest.max() - ingest.min()), 4), "m1_in_vs_ingest": round(float(np.median(ingest) / np.median(accept)), 2),
               "m1_in_hbm_fraction": frac(np.median(accept)), "ingest_hbm_fraction": frac(np.median(ingest)),
               "send_ms": med(send), "garble_ms": med(garble), "garble_last_ms": round(garble_ms, 4),
               "send_share_not_garbling": round(1 - float(np.median(garble) / np.median(send)), 3),
               "accept_eval_ms": round(med(accept) + med(ev), 4), "eval_pass_ms": med(ev_pass), "eval_last_ms": round(eval_ms, 4),
               "accept_eval_share_not_evaluating": round(1 - float(np.median(ev_pass) / (np.median(accept) + np.median(ev))), 3),
               "m2_out_us": round(1e3 * med(m2_out), 1), "result_us": round(1e3 * med(result), 1), "parse_us": round(1e3 * med(parse), 1),
               "window_s": args.window, "reps": args.reps}
        rows.append(row)
        print(json.dumps(row), flush=True)
        b.close()
    if args.out and rows:
        with open(args.out, "a" if args.append else "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    dc.close()
    ctx.close()


if __name__ == "__main__":
    main()
