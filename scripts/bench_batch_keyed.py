"""One AES key per instance (gc_batch_garble_keyed / gc_batch_eval_keyed) beside the one-key batch calls: aes_128 x 1 024 and
sha256xor x 256 under 32-byte keys, everything in HBM, one JSON line per circuit.

Method: the one-key form and the keyed form alternate in one process.  Each of the four passes (garble and eval of either
form) is recorded once in a hipGraph; PREWARM untimed launches of the step bring the card to its sustained clocks, as bench.py
warms its headline; then --reps rounds, each timing the four passes one after the other: a host clock around k launches that end
in gc_ctx_sync, k sized once so that a window lasts at least --window seconds.  ms per pass = window / k; the median of the
rounds is reported with every round beside it.

  garble_ms / eval_ms            the one-key passes (gc_batch_garble / gc_batch_eval)
  keyed_garble_ms / ..eval_ms    the keyed passes; the garbler's includes k_expand_keys (it is part of the call)
  keyed_over_one_key             their ratios, garble, eval and the sum
  expand_ms                      what the key expansion adds to a pass: keyed minus one-key garble of a ONE-GATE circuit at the
                                 same batch (expansion kernel + the load of the LDS key table; the hashing is nothing there)
  one_instance_batches_ms        what a caller with per-session keys had to do before: one batch of ONE instance per session,
                                 garble + eval under its own key, timed on at most --sample sessions and scaled to the batch
  keyed_over_one_instance        keyed garble + eval against that

--hbm: the keyed kernels with the wires in HBM (path 2 of gc_batch_keyed_path) instead, same protocol, two lines:
  (a) the synthetic levelised circuit of bench.py's `synthetic` row (131 072 gates, W = 1 024, f = 0.17) x 1 024, whose wires
      are in HBM: the one-key HBM-wire pass against keyed path 2;
  (b) aes_128 x 1 024: keyed path 1 (wires in LDS) against path 2 forced with gc_batch_set_keyed_path — what the fall-back
      costs a batch that could run in LDS; the one-key pass beside them.
--form F (with --hbm): gc_batch_set_keyed_hbm_form on the path-2 batches, 0 the rule, 1 the plain form, 2 the split form (hash
waves and free waves on wide levels); the line's `form` is what gc_batch_keyed_hbm_form then reports, `form_setting` is F.
--hsweep (with --hbm): the synthetic row only, split form, the hash waves of every split level fixed at H = 4 .. 15 for both
roles (gc_batch_debug_keyed_hbm_hash_waves), the plain form and the rule beside them: one text line per setting."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mpc_amd import circuit, engine, parse_file  # noqa: E402

PREWARM = 100  # untimed launches ahead of the windows (bench.py: PREWARM_STEPS)
CASES = [("aes_128", 1024), ("sha256xor", 256)]


def window(ctx, launch, k):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(k):
        launch()
    ctx.sync()
    return (time.perf_counter() - t0) / k * 1e3


def alternate(ctx, passes, reps, seconds):
    """{name: [ms per launch, one per round]} of graphs / callables timed round-robin"""
    for launch in passes.values():
        for _ in range(PREWARM):
            launch()
    ks = {}
    for name, launch in passes.items():
        ms = window(ctx, launch, 20)
        ks[name] = max(20, int(seconds * 1e3 / max(ms, 1e-3)))
    out = {name: [] for name in passes}
    for _ in range(reps):
        for name, launch in passes.items():
            out[name].append(window(ctx, launch, ks[name]))
    return out


def graphs_of(ctx, gb, ev, d_bits, garble, evaluate):
    """the two passes run once directly (key upload, allocations), then as one hipGraph each"""
    garble()
    ev.select_inputs(gb, d_bits)
    evaluate()
    ctx.sync()
    return ctx.capture(garble), ctx.capture(evaluate)


def measure(ctx, c, batch, reps, seconds, sample):
    rng = np.random.default_rng(7)
    dc = engine.DeviceCircuit(ctx, c)
    gb, ev = engine.Batch(dc, batch), engine.Batch(dc, batch)
    assert gb.keyed_supported() and ev.keyed_supported()
    d_rnd = ctx.random_u8((batch, c.num_inputs + 1, 16), 256, seed=1234)
    d_bits = ctx.random_u8((batch, c.num_inputs), 2, seed=4321)
    keys = rng.integers(0, 256, (batch, 32), dtype=np.uint8)
    d_keys = ctx.to_device(keys)
    key = keys[0].tobytes()
    g1, e1 = graphs_of(ctx, gb, ev, d_bits, lambda: gb.garble(key, d_rnd), lambda: ev.eval(key, gb))
    gk, ek = graphs_of(ctx, gb, ev, d_bits, lambda: gb.garble_keyed(d_keys, 32, d_rnd), lambda: ev.eval_keyed(d_keys, 32, gb))
    t = alternate(ctx, {"garble": g1.launch, "keyed_garble": gk.launch, "eval": e1.launch, "keyed_eval": ek.launch}, reps, seconds)
    # the expansion alone: a one-gate circuit at the same batch
    tiny = circuit.and_chain(1)
    dct = engine.DeviceCircuit(ctx, tiny)
    tb = engine.Batch(dct, batch)
    d_trnd = ctx.random_u8((batch, tiny.num_inputs + 1, 16), 256, seed=99)
    tb.garble(key, d_trnd)
    tb.garble_keyed(d_keys, 32, d_trnd)
    ctx.sync()
    t1, tk = ctx.capture(lambda: tb.garble(key, d_trnd)), ctx.capture(lambda: tb.garble_keyed(d_keys, 32, d_trnd))
    tt = alternate(ctx, {"tiny": t1.launch, "tiny_keyed": tk.launch}, reps, seconds / 4)
    # one batch of one instance per session: what per-session keys cost a caller without the keyed calls
    n1 = min(sample, batch)
    singles = []
    for i in range(n1):
        a, b = engine.Batch(dc, 1), engine.Batch(dc, 1)
        singles.append((a, b, keys[i].tobytes(), ctx.random_u8((1, c.num_inputs + 1, 16), 256, seed=i)))

    def sessions():
        for a, b, k, r in singles:
            a.garble(k, r)
            b.select_inputs(a, d_bits)
            b.eval(k, a)

    sessions()
    ts = [window(ctx, sessions, 3) * batch / n1 for _ in range(reps)]
    med = {k: statistics.median(v) for k, v in list(t.items()) + list(tt.items())}
    one, keyed = med["garble"] + med["eval"], med["keyed_garble"] + med["keyed_eval"]
    row = {
        "bench": "batch_keyed", "circuit": c.name, "batch": batch, "key_bytes": 32, "tile_instances": gb.tile_instances,
        "and_gates": dc.info.n_and, "reps": reps, "window_s": seconds,
        "garble_ms": med["garble"], "eval_ms": med["eval"], "keyed_garble_ms": med["keyed_garble"],
        "keyed_eval_ms": med["keyed_eval"],
        "keyed_over_one_key": {"garble": med["keyed_garble"] / med["garble"], "eval": med["keyed_eval"] / med["eval"],
                               "garble_plus_eval": keyed / one},
        "expand_ms": med["tiny_keyed"] - med["tiny"], "one_gate_garble_ms": med["tiny"], "one_gate_keyed_garble_ms": med["tiny_keyed"],
        "one_instance_batches_ms": statistics.median(ts), "one_instance_batches_timed": n1,
        "keyed_over_one_instance": keyed / statistics.median(ts),
        "keyed_and_gates_per_s": dc.info.n_and * batch / (keyed * 1e-3),
        "one_key_and_gates_per_s": dc.info.n_and * batch / (one * 1e-3),
        "ms_all": {k: v for k, v in list(t.items()) + list(tt.items())}, "one_instance_batches_ms_all": ts,
    }
    for g in (g1, e1, gk, ek, t1, tk):
        g.close()
    for a, b, _, _ in singles:
        a.close()
        b.close()
    for b in (gb, ev, tb):
        b.close()
    dct.close()
    dc.close()
    return row


def measure_hbm(ctx, c, batch, reps, seconds, forced, form=0):
    """forced = False: one key against keyed path 2 on a batch whose wires are in HBM; True: one key, keyed path 1 and keyed
    path 2 (a second pair of batches sent there) on a batch whose wires are in LDS"""
    rng = np.random.default_rng(7)
    dc = engine.DeviceCircuit(ctx, c)
    gb, ev = engine.Batch(dc, batch), engine.Batch(dc, batch)
    assert gb.keyed_path == ev.keyed_path == (1 if forced else 2) and gb.lds_wires == forced
    d_rnd = ctx.random_u8((batch, c.num_inputs + 1, 16), 256, seed=1234)
    d_bits = ctx.random_u8((batch, c.num_inputs), 2, seed=4321)
    keys = rng.integers(0, 256, (batch, 32), dtype=np.uint8)
    d_keys = ctx.to_device(keys)
    key = keys[0].tobytes()
    if not forced:
        for b in (gb, ev):
            b.set_keyed_hbm_form(form)
    g1, e1 = graphs_of(ctx, gb, ev, d_bits, lambda: gb.garble(key, d_rnd), lambda: ev.eval(key, gb))
    gk, ek = graphs_of(ctx, gb, ev, d_bits, lambda: gb.garble_keyed(d_keys, 32, d_rnd), lambda: ev.eval_keyed(d_keys, 32, gb))
    passes = {"garble": g1.launch, "eval": e1.launch}
    graphs, batches = [g1, e1, gk, ek], [gb, ev]
    if forced:
        gb2, ev2 = engine.Batch(dc, batch), engine.Batch(dc, batch)
        for b in (gb2, ev2):
            b.set_keyed_path(2)
            b.set_keyed_hbm_form(form)
        g2, e2 = graphs_of(ctx, gb2, ev2, d_bits, lambda: gb2.garble_keyed(d_keys, 32, d_rnd), lambda: ev2.eval_keyed(d_keys, 32, gb2))
        passes.update({"path1_garble": gk.launch, "path1_eval": ek.launch, "path2_garble": g2.launch, "path2_eval": e2.launch})
        graphs += [g2, e2]
        batches += [gb2, ev2]
    else:
        passes.update({"path2_garble": gk.launch, "path2_eval": ek.launch})
    t = alternate(ctx, passes, reps, seconds)
    med = {k: statistics.median(v) for k, v in t.items()}
    base = "path1" if forced else ""
    bg, be = (med["path1_garble"], med["path1_eval"]) if forced else (med["garble"], med["eval"])
    row = {
        "bench": "batch_keyed_hbm", "circuit": c.name, "batch": batch, "key_bytes": 32, "tile_instances": gb.tile_instances,
        "gates": int(dc.info.ngates), "and_gates": int(dc.info.n_and), "levels": int(dc.info.nlevels), "reps": reps,
        "window_s": seconds, "wires_in_lds_under_one_key": bool(forced),
        "form": batches[-1].keyed_hbm_form, "form_setting": form,
        "one_key_garble_ms": med["garble"], "one_key_eval_ms": med["eval"],
        "path2_garble_ms": med["path2_garble"], "path2_eval_ms": med["path2_eval"],
        "path2_over": "keyed path 1" if forced else "the one-key HBM-wire pass",
        "path2_over_base": {"garble": med["path2_garble"] / bg, "eval": med["path2_eval"] / be,
                            "garble_plus_eval": (med["path2_garble"] + med["path2_eval"]) / (bg + be)},
        "path2_and_gates_per_s": dc.info.n_and * batch / ((med["path2_garble"] + med["path2_eval"]) * 1e-3),
        "ms_all": t,
    }
    if forced:
        row["path1_garble_ms"], row["path1_eval_ms"] = med["path1_garble"], med["path1_eval"]
    for g in graphs:
        g.close()
    for b in batches:
        b.close()
    dc.close()
    return row


def main_hsweep(ctx, c, batch, reps, seconds, out):
    """the synthetic row under the split form with H fixed for both roles, the plain form and the rule beside them"""
    rng = np.random.default_rng(7)
    dc = engine.DeviceCircuit(ctx, c)
    gb, ev = engine.Batch(dc, batch), engine.Batch(dc, batch)
    assert gb.keyed_path == ev.keyed_path == 2
    d_rnd = ctx.random_u8((batch, c.num_inputs + 1, 16), 256, seed=1234)
    d_bits = ctx.random_u8((batch, c.num_inputs), 2, seed=4321)
    d_keys = ctx.to_device(rng.integers(0, 256, (batch, 32), dtype=np.uint8))
    settings = [("plain", 1, 0)] + [("H=%d" % h, 2, h) for h in range(4, 16)] + [("rule", 0, 0), ("plain", 1, 0)]
    head = "# %s x %d, tiles of %d, 32-byte keys; ms per pass, median of %d windows of %.2f s (all windows in brackets)" % (
        c.name, batch, gb.tile_instances, reps, seconds)
    lines = [head]
    print(head, flush=True)
    for name, form, h in settings:
        for b in (gb, ev):
            b.set_keyed_hbm_form(form)
            b.debug_keyed_hbm_hash_waves(h, h)
        gk, ek = graphs_of(ctx, gb, ev, d_bits, lambda: gb.garble_keyed(d_keys, 32, d_rnd), lambda: ev.eval_keyed(d_keys, 32, gb))
        t = alternate(ctx, {"garble": gk.launch, "eval": ek.launch}, reps, seconds)
        line = "%-6s form %d  garble %.3f ms %s  eval %.3f ms %s" % (
            name, gb.keyed_hbm_form, statistics.median(t["garble"]), ["%.3f" % v for v in t["garble"]],
            statistics.median(t["eval"]), ["%.3f" % v for v in t["eval"]])
        print(line, flush=True)
        lines.append(line)
        gk.close()
        ek.close()
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")
    gb.close()
    ev.close()
    dc.close()


def main_hbm(ctx, a):
    w, frac = a.synthetic_width, a.synthetic_frac  # scripts/sweep_synthetic.py: the (1 024, 0.17) row by default
    syn = circuit.synthetic_levelised(131072 // w, w, frac, seed=101, ninputs=256)
    syn.name = "synthetic_w%d_f%g" % (w, frac)
    if a.hsweep:
        main_hsweep(ctx, syn, a.batch, a.reps, a.window, a.out)
        return
    aes = parse_file(os.path.join(ROOT, "tests", "golden", "aes_128.gcf"))
    aes.name = "aes_128"
    for c, forced in ((syn, False), (aes, True))[: 2 if (w, frac, a.batch) == (1024, 0.17, 1024) else 1]:
        line = json.dumps(measure_hbm(ctx, c, a.batch, a.reps, a.window, forced, a.form))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hbm", action="store_true", help="the keyed HBM-wire kernels (path 2) instead: see the module docstring")
    ap.add_argument("--form", type=int, default=0, choices=[0, 1, 2], help="with --hbm: the form of the path-2 kernels (0 the rule)")
    ap.add_argument("--synthetic-width", type=int, default=1024, help="with --hbm: gates per level of the synthetic row (131 072 in all)")
    ap.add_argument("--synthetic-frac", type=float, default=0.17, help="with --hbm: AND fraction of the synthetic row")
    ap.add_argument("--batch", type=int, default=1024, help="with --hbm: instances (another shape than the default one drops the aes_128 row)")
    ap.add_argument("--hsweep", action="store_true", help="with --hbm: the synthetic row with the hash waves fixed at 4 .. 15")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--sample", type=int, default=64, help="one-instance batches the sequential row is timed on")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    ctx = engine.Context(0)
    if a.hbm:
        main_hbm(ctx, a)
        ctx.close()
        return
    for name, batch in CASES:
        c = parse_file(os.path.join(ROOT, "tests", "golden", name + ".gcf"))
        c.name = name
        line = json.dumps(measure(ctx, c, batch, a.reps, a.window, a.sample))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
