#!/usr/bin/env python
"""The four sha2pc rounds for S sessions per call (gc_sha2pc_*_dev) against the best route without them, on sha256xor.

Two forms alternate in one process, each with an untimed pass first; a timed window lies between two gc_ctx_sync on the
host clock and is repeated until it has lasted --window seconds; the median of --reps windows is reported per call.

  dev   the round as one gc_sha2pc_*_dev call on device slots
  b     the same round through gc_co_multi_*_dev, the keyed batch, the dense table egress / ingest and read-backs, with the
        payloads spliced and parsed on the host (numpy) and the choice points decompressed on the host with PYTHON INTEGERS
        standing in for math/big (pow(t, (p + 1) // 4, p) per point): what a caller of the library had before

Both forms produce the same bytes; the script checks that before it times anything.  --trace runs Round 3 and Round 4 of the
dev form a few times at one S and nothing else, for a kernel trace taken in a run of its own.

    python scripts/bench_sha2pc.py --S 64 256 1024 --out profiles/sha2pc_bench.jsonl
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

P = 0xFFFFFFFF00000001000000000000000000000000FFFFFFFFFFFFFFFFFFFFFFFF
B = 0x5AC635D8AA3A93E7B3EBBD55769886BC651D06B0CC53B0F63BCE3C3E27D2604B
NG = NE = NOUT = 256
CHUNK = np.frombuffer(b"\x05P-256", np.uint8)


def label_bytes(lab):
    """LABEL [...] -> u8 [..., 16]: BE(D0) || BE(D1)"""
    out = np.empty(lab.shape + (2,), ">u8")
    out[..., 0], out[..., 1] = lab["d0"], lab["d1"]
    return out.view(np.uint8).reshape(lab.shape + (16,))


def bytes_label(raw):
    be = np.ascontiguousarray(raw).view(">u8").reshape(raw.shape[:-1] + (2,))
    out = np.zeros(raw.shape[:-1], engine.LABEL)
    out["d0"], out["d1"] = be[..., 0], be[..., 1]
    return out


class Bench:
    def __init__(self, ctx, dc, S, seed=1):
        self.ctx, self.dc, self.S = ctx, dc, S
        self.rows = dc.info.slab_rows
        rng = np.random.default_rng(seed)
        rb = lambda *shape: rng.integers(0, 256, shape, dtype=np.uint8)
        self.h = {"a": rb(S, 32), "sid": rb(S, 8), "scalars": rb(S, NE, 32), "ebits": rb(S, NE) & 1, "gbits": rb(S, NG) & 1,
                  "keys": rb(S, 32), "rnd": rb(S, 16 * (1 + NG + NE))}
        self.h["a"][:, 0] &= 0x7F  # below N, not zero
        self.d = {k: ctx.to_device(v) for k, v in self.h.items()}
        self.gb, self.ev = engine.Sha2pcGarbler(dc, NG, NE, S), engine.Sha2pcEvaluator(dc, NG, NE, S)
        self.len, self.lead, self.stride = self.gb.len, self.gb.lead, self.gb.stride
        z = ctx.zeros
        self.slots = [z(S * st) for st in self.stride]
        self.d_v, self.d_A, self.d_ainv, self.d_A2, self.d_sid2 = z(4 * S), z(64 * S), z(64 * S), z(64 * S), z(8 * S)
        self.d_digest = z(32 * S)
        # form b: its own batches and arrays
        self.bg, self.be = engine.Batch(dc, S), engine.Batch(dc, S)
        self.bstride = self.bg.stride
        self.d_status, self.d_points, self.d_ct = z(32), z(64 * S * NE), z(32 * S * NE)
        self.d_wires, self.d_ew, self.d_outs = z(32 * S * NG), z(32 * S * NE), z(16 * NOUT * self.bstride)
        self.d_tables, self.d_labels, self.d_el = z(16 * self.rows * S), z(16 * S * NG), z(16 * S * NE)
        self.d_A_b, self.d_ainv_b, self.d_keys_b = z(64 * S), z(64 * S), z(32 * S)

    # ---- dev form ----
    def dev1(self):
        self.gb.round1_dev(self.d["a"], self.d["sid"], self.d_A, self.d_ainv, self.slots[0], self.stride[0], self.d_v)

    def dev2(self):
        self.ev.round2_dev(self.slots[0], self.stride[0], self.d["scalars"], self.d["ebits"], self.d_A2, self.d_sid2,
                           self.slots[1], self.stride[1], self.d_v)

    def dev3(self):
        self.gb.round3_dev(self.d["a"], self.d_ainv, self.d["sid"], self.slots[1], self.stride[1], self.d["keys"],
                           self.d["rnd"], self.d["gbits"], self.slots[2], self.stride[2], self.d_v)

    def dev4(self):
        self.ev.round4_dev(self.d_A2, self.d_sid2, self.d["scalars"], self.d["ebits"], self.slots[2], self.stride[2],
                           self.d_digest, self.d_v)

    def payloads(self, k):
        raw = self.slots[k].download(np.uint8, (self.S, self.stride[k]))
        return raw[:, self.lead[k]:self.lead[k] + self.len[k]]

    # ---- form b: every function returns what the dev form leaves on the device, as host arrays ----
    def b1(self):
        S = self.S
        engine.co_multi_sender_setup_dev(self.ctx, self.d["a"], S, self.d_A_b, self.d_ainv_b, self.d_status)
        A = self.d_A_b.download(np.uint8, (S, 64))
        r1 = np.empty((S, 80), np.uint8)
        r1[:, :2], r1[:, 2:10], r1[:, 10:16], r1[:, 16:] = (0x52, 0x31), self.h["sid"], CHUNK, A
        return r1

    def b2(self, r1):
        S = self.S
        assert (r1[:, :2] == (0x52, 0x31)).all() and (r1[:, 10:16] == CHUNK).all()
        A = self.ctx.to_device(np.ascontiguousarray(r1[:, 16:]))
        engine.co_multi_receiver_choices_dev(self.ctx, A, self.d["scalars"], self.d["ebits"], S, NE, self.d_points, self.d_status)
        pts = self.d_points.download(np.uint8, (S, NE, 64))
        r2 = np.empty((S, self.len[1]), np.uint8)
        r2[:, :2], r2[:, 2:10], r2[:, 10:16] = (0x52, 0x32), r1[:, 2:10], CHUNK
        r2[:, 16:16 + 32 * NE] = pts[:, :, :32].reshape(S, -1)
        r2[:, 16 + 32 * NE:] = np.packbits(pts[:, :, 63] & 1, axis=1, bitorder="little")
        return r2

    def decompress(self, r2):
        """decodePoints on the host: one square root mod p per OT, with Python integers"""
        S = self.S
        signs = np.unpackbits(r2[:, 16 + 32 * NE:], axis=1, bitorder="little")
        out = bytearray(64 * S * NE)
        exp = (P + 1) // 4
        for s in range(S):
            row = r2[s, 16:16 + 32 * NE].tobytes()
            for j in range(NE):
                x = int.from_bytes(row[32 * j:32 * j + 32], "big")
                t = (x * x * x - 3 * x + B) % P
                y = pow(t, exp, P)
                assert x < P and y * y % P == t
                if (y & 1) != signs[s, j]:
                    y = P - y
                o = 64 * (s * NE + j)
                out[o:o + 32], out[o + 32:o + 64] = row[32 * j:32 * j + 32], y.to_bytes(32, "big")
        return np.frombuffer(bytes(out), np.uint8)

    def b3(self, r2):
        S, rows = self.S, self.rows
        assert (r2[:, 2:10] == self.h["sid"]).all()
        self.d_points.upload(self.decompress(r2))
        self.bg.garble_keyed(self.d["keys"], 32, self.d["rnd"])
        self.bg.gather_input_wires(0, NG, self.d_wires)
        self.bg.gather_input_wires(NG, NE, self.d_ew)
        engine.co_multi_sender_encrypt_dev(self.ctx, self.d["a"], self.d_ainv_b, self.d_points, self.d_ew, S, NE, 0, self.d_ct, self.d_status)
        self.bg.egress_tables_dense(self.d_tables, 16 * rows)
        self.bg.gather_outputs(self.d_outs)
        g = self.d_wires.download(engine.WIRE, (S, NG))
        outs = self.d_outs.download(engine.LABEL, (NOUT, self.bstride))[:, :S].T
        R = self.bg.read_r()[:S]
        r3 = np.empty((S, self.len[2]), np.uint8)
        r3[:, :2], r3[:, 2:10], r3[:, 10:42] = (0x52, 0x33), self.h["sid"], self.h["keys"]
        o = 42
        r3[:, o:o + 16 * rows] = self.d_tables.download(np.uint8, (S, 16 * rows))
        o += 16 * rows
        sel = np.where(self.h["gbits"].astype(bool), g["l1"], g["l0"])
        r3[:, o:o + 16 * NG] = label_bytes(sel).reshape(S, -1)
        o += 16 * NG
        l1 = np.zeros_like(outs)
        l1["d0"], l1["d1"] = outs["d0"] ^ R["d0"][:, None], outs["d1"] ^ R["d1"][:, None]
        r3[:, o:o + 32 * NOUT] = np.stack([label_bytes(outs), label_bytes(l1)], 2).reshape(S, -1)
        o += 32 * NOUT
        r3[:, o:] = self.d_ct.download(np.uint8, (S, 32 * NE))
        return r3

    def b4(self, r1, r3):
        S, rows = self.S, self.rows
        assert (r3[:, :2] == (0x52, 0x33)).all() and (r3[:, 2:10] == r1[:, 2:10]).all()
        o = 42
        self.d_keys_b.upload(np.ascontiguousarray(r3[:, 10:42]))
        self.d_tables.upload(np.ascontiguousarray(r3[:, o:o + 16 * rows]))
        o += 16 * rows
        self.d_labels.upload(bytes_label(np.ascontiguousarray(r3[:, o:o + 16 * NG]).reshape(S, NG, 16)))
        o += 16 * NG
        hints = np.ascontiguousarray(r3[:, o:o + 32 * NOUT]).reshape(S, NOUT, 2, 16)
        o += 32 * NOUT
        self.d_ct.upload(np.ascontiguousarray(r3[:, o:]))
        A = self.ctx.to_device(np.ascontiguousarray(r1[:, 16:]))
        self.be.ingest_tables_dense(self.d_tables, 16 * rows)
        engine.co_multi_receiver_decrypt_dev(self.ctx, A, self.d["scalars"], self.d["ebits"], self.d_ct, S, NE, 0, self.d_el, self.d_status)
        self.be.set_input_range(0, NG, self.d_labels)
        self.be.set_input_range(NG, NE, self.d_el)
        self.be.eval_keyed(self.d_keys_b, 32, self.be)
        self.be.gather_outputs(self.d_outs)
        outs = label_bytes(self.d_outs.download(engine.LABEL, (NOUT, self.bstride))[:, :S].T)
        is0, is1 = (outs == hints[:, :, 0]).all(2), (outs == hints[:, :, 1]).all(2)
        assert (is0 | is1).all()
        return np.packbits(~is0 & is1, axis=1, bitorder="little")


def window_ms(ctx, fn, window):
    """the time of one fn() in ms, over a window of at least `window` seconds between two syncs"""
    n = 0
    ctx.sync()
    t0 = time.perf_counter()
    while True:
        fn()
        n += 1
        ctx.sync()
        dt = time.perf_counter() - t0
        if dt >= window:
            return 1e3 * dt / n


def timed(ctx, fns, window, reps):
    """the forms alternate window by window; per form the median of `reps` windows, and the windows"""
    per = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            per[k].append(window_ms(ctx, fn, window))
    return [(float(np.median(w)), w) for w in per]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="Round 3 and Round 4 of the dev form alone, three times at the first S")
    args = ap.parse_args()
    circ = parse_file(os.path.join(ROOT, "tests", "golden", "sha256xor.gcf"))
    ctx = engine.Context(0)
    dc = engine.DeviceCircuit(ctx, circ)
    rows = []
    for S in args.S:
        b = Bench(ctx, dc, S)
        # one untimed pass of each form, and both give the same bytes
        b.dev1(), b.dev2(), b.dev3(), b.dev4()
        ctx.sync()
        r1, r2, r3 = (b.payloads(k).copy() for k in range(3))
        digest = b.d_digest.download(np.uint8, (S, 32))
        assert not b.d_v.download(np.uint32, (S,)).any()
        if args.trace:
            for _ in range(3):
                b.dev3(), b.dev4()
            ctx.sync()
            print("trace pass done: S = %d" % S)
            b.gb.close(), b.ev.close()  # before the circuit and the ctx
            break
        h1 = b.b1()
        h2 = b.b2(h1)
        h3 = b.b3(h2)
        h4 = b.b4(h1, h3)
        assert (h1 == r1).all() and (h2 == r2).all() and (h3 == r3).all() and (h4 == digest).all(), "the forms differ"
        forms = {"round1": (b.dev1, b.b1), "round2": (b.dev2, lambda: b.b2(h1)), "round3": (b.dev3, lambda: b.b3(h2)),
                 "round4": (b.dev4, lambda: b.b4(h1, h3))}
        for name, (dev, base) in forms.items():
            (t_dev, w_dev), (t_b, w_b) = timed(ctx, (dev, base), args.window, args.reps)
            row = {"bench": "sha2pc", "circuit": "sha256xor", "S": S, "call": name, "dev_ms": round(t_dev, 4),
                   "b_ms": round(t_b, 4), "dev_faster": t_dev < t_b, "speedup": round(t_b / t_dev, 2),
                   "dev_windows_ms": [round(x, 4) for x in w_dev], "b_windows_ms": [round(x, 4) for x in w_b],
                   "window_s": args.window, "reps": args.reps,
                   "b": "gc_co_multi_*_dev + keyed batch + dense egress / ingest + read-backs; payloads spliced with numpy, "
                        "points decompressed with Python integers standing in for math/big"}
            rows.append(row)
            print(json.dumps(row), flush=True)
        b.gb.close(), b.ev.close()
    if args.out and rows:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    dc.close()
    ctx.close()


if __name__ == "__main__":
    main()
