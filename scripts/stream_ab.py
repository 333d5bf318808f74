"""A/B of two builds of libgcengine.so on the streamed programs (scripts/bench_stream.py): rates, the host's stage cycles
(GC_TRACE=1) and every scheduling count of both sides (gc_stream_stats, *_fuse_stats, *_wait_stats, *_deep_stats), one child
process per run (GC_LIB selects the library), the two builds alternating.  Made for refactors of the streaming engine's host
side: "same decisions, same speed" against the parent commit's build.

  stream_ab.py run PLAN --base-lib PATH [--base-driver PATH] [--out FILE]   PLAN: timing | controls | stats | trace | view | native
  stream_ab.py report FILE...
  (--base-driver: tools/stream_driver linked against the base library, for the plan `native`)

A child that fails ends the run.  Every child runs under a time limit of its own."""
import argparse
import hashlib
import json
import os
import re
import statistics as st
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def one(name, window, reps, flags):
    """one library, one program, a fixed sequence of passes: garbler (bytes copied, then in place), evaluator block by block
    and over read buffers; the first pass of each kind warms the plans"""
    import bench_stream as bs
    from mpc_amd import engine
    key = bytes(range(32))
    steps, prim = bs.PROGRAMS[name]()
    rnd = bs.stream_rnd(name, len(prim))
    gates = sum(c.NumGates for c, _, _ in steps)
    want = bs.golden_sha(name, key)
    ctx = engine.Context(0)
    passes, ev_stats = [], []
    close0 = engine.StreamEval.close

    def close(self):  # (bench_stream closes its evaluators itself: their counts are read on the way)
        ev_stats.append({"fuse": list(self.fuse_stats()), "waiting": self.wait_stats(), "deep": list(self.deep_stats()),
                         "parsed_matched": list(self.stats()), "dev": list(self.dev_stats())})
        return close0(self)
    engine.StreamEval.close = close

    def gstats(g, stats):
        return {"groups": stats[0], "grouped_steps": stats[1], "big_steps": stats[2], "fuse": list(g.fuse_stats()),
                "waiting": g.wait_stats(), "deep": list(g.deep_stats())}
    last = None
    for rep in range(1 + reps):
        stream, sizes, dt, stats, g = bs.garble_program(ctx, key, steps, prim, rnd, window, True, False)
        sha = hashlib.sha256(memoryview(stream)).hexdigest()
        if want is not None and sha != want:
            raise AssertionError("%s: stream SHA-256 %s != oracle's %s" % (name, sha, want))
        passes.append({"phase": "garble_copied", "rep": rep, "s": dt, "gates_per_s": gates / dt, "stats": gstats(g, stats)})
        if last is not None:
            last.close()
        last = g
    if "noview" not in flags:
        for rep in range(max(reps, 1)):
            _, _, dt, stats, gv = bs.garble_program(ctx, key, steps, prim, rnd, window, True, True)
            passes.append({"phase": "garble_view", "rep": rep, "s": dt, "gates_per_s": gates / dt, "stats": gstats(gv, stats)})
            gv.close()
    if "noeval" not in flags:
        for rep in range(1 + reps):
            dt, _ = bs.eval_program(ctx, key, steps, prim, g, stream, sizes)
            passes.append({"phase": "eval_circuit", "rep": rep, "s": dt, "gates_per_s": gates / dt, "stats": ev_stats[-1]})
        for rep in range(1 + reps):
            dt, _, _ = bs.eval_program_blocks(ctx, key, steps, prim, g, stream, sizes)
            passes.append({"phase": "eval_blocks", "rep": rep, "s": dt, "gates_per_s": gates / dt, "stats": ev_stats[-1]})
    g.close()
    ctx.close()
    print(json.dumps({"program": name, "window": window, "steps": len(steps), "gates": gates, "sha256_ok": want is not None,
                      "env": {k: os.environ[k] for k in os.environ if k.startswith("GC_STREAM")}, "passes": passes}), flush=True)


def native(name, window, driver):
    import bench_stream as bs
    bs.NATIVE = driver
    print(json.dumps(bs.run_native(name, window=window)), flush=True)


def run(plan, libs, drivers, out):
    def child(label, argv, env_extra, timeout=420):
        env = dict(os.environ, GC_LIB=libs[label], **env_extra)
        t0 = time.time()
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
        if r.returncode != 0:
            sys.exit("child failed (%d): %s\n%s" % (r.returncode, " ".join(argv), r.stderr[-3000:]))
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        rec.update({"plan": plan, "lib": label, "wall_s": round(time.time() - t0, 1), "env_extra": env_extra,
                    "trace": [l for l in r.stderr.splitlines() if "host cycles per step" in l]})
        with open(out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print("%s %s %s: %.0f s" % (plan, label, " ".join(argv), rec["wall_s"]), flush=True)
    both = ("base", "new")
    if plan == "timing":  # 3 processes per build, 2 timed passes each behind a warm one
        for _ in range(3):
            for label in both:
                child(label, ["one", "ed25519like", "1024", "2"], {})
    elif plan == "controls":
        for _ in range(3):
            for label in both:
                child(label, ["one", "ssa23", "64", "2", "noview"], {})
                child(label, ["one", "mixed", "64", "2", "noview"], {})
    elif plan == "stats":  # the base three times, the new build once: which counts are a function of the program alone?
        for prog, win, env in (("ed25519like", "1", {}), ("ed25519like", "1", {"GC_STREAM_NO_FUSE": "1"}), ("uniform512", "64", {}),
                               ("uniform4096", "64", {}), ("big130", "4", {})):
            for label in ("base", "base", "base", "new"):
                child(label, ["one", prog, win, "0", "noview"], env, timeout=600)
    elif plan == "trace":
        for _ in range(5):
            for label in both:
                child(label, ["one", "ed25519like", "1024", "1", "noview"], {"GC_TRACE": "1"})
    elif plan == "view":  # the garbler alone, bytes handed out in place, with its stage cycles
        for _ in range(5):
            for label in both:
                child(label, ["one", "ed25519like", "1024", "2", "noeval"], {"GC_TRACE": "1"})
    elif plan == "native":
        for env in ({}, {}, {}, {}, {}, {"GC_TRACE": "1"}, {"GC_TRACE": "1"}, {"GC_TRACE": "1"}):
            for label in both:
                child(label, ["native", "ed25519like", "1024", drivers[label]], env, timeout=300)
    else:
        sys.exit("unknown plan " + plan)


def flat(d, pre=""):
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(flat(v, pre + k + "."))
        elif isinstance(v, list):
            out.update({"%s%s[%d]" % (pre, k, i): x for i, x in enumerate(v)})
        else:
            out[pre + k] = v
    return out


def report(files):
    recs = [json.loads(l) for p in files for l in open(p) if l.strip()]
    for r in recs:
        r["lib"] = "base" if r["lib"] in ("base", "parent") else "new"
    rates, counts, cyc = {}, {}, {}
    for r in recs:
        if "passes" in r:
            envk = ",".join("%s=%s" % kv for kv in sorted(r["env"].items()))
            for p in r["passes"]:
                if r["plan"].startswith(("timing", "controls", "view")) and (p["rep"] or p["phase"] == "garble_view"):
                    rates.setdefault((r["program"], r["window"], p["phase"]), {}).setdefault(r["lib"], []).append(p["gates_per_s"])
                for k, v in flat(p["stats"]).items():
                    counts.setdefault((r["program"], r["window"], envk, r["plan"], p["phase"], p["rep"], k), {}).setdefault(r["lib"], []).append(v)
        elif not r["env_extra"]:
            for k in r:
                if k.endswith("gates_per_s") and r[k] and "steady" not in k:
                    rates.setdefault((r["program"], r["window"], "C host " + k), {}).setdefault(r["lib"], []).append(r[k])
        seen = {}
        for l in r.get("trace", []):
            m = re.search(r"\] (\w+): host cycles per step \((\d+) steps\):(.*)\|", l)
            d = dict(zip(m.group(3).split()[0::2], map(float, m.group(3).split()[1::2])))
            nth = seen[m.group(1)] = seen.get(m.group(1), -1) + 1  # (streams are freed in the order of the passes)
            cyc.setdefault((r["plan"], m.group(1), "stream %d" % nth), {}).setdefault(r["lib"], []).append(d["place"] + d["queue"] + d["mark"])
    print("== rates, gates/s: row | base n min median max | new n min median max | new median >= base min")
    for key in sorted(rates):
        a, b = rates[key].get("base", []), rates[key].get("new", [])
        if a and b:
            print("%-55s | %d %.3e %.3e %.3e | %d %.3e %.3e %.3e | %s" % (" ".join(map(str, key)), len(a), min(a), st.median(a), max(a), len(b),
                                                                          min(b), st.median(b), max(b), "ok" if st.median(b) >= min(a) else "BELOW"))
    print("== host cycles per step, place + queue + mark: stream | base n min median max | new n min median max | new median <= base max")
    for key in sorted(cyc):
        a, b = cyc[key].get("base", []), cyc[key].get("new", [])
        if a and b:
            print("%-35s | %d %.0f %.0f %.0f | %d %.0f %.0f %.0f | %s" % (" ".join(key), len(a), min(a), st.median(a), max(a), len(b), min(b), st.median(b),
                                                                        max(b), "ok" if st.median(b) <= max(a) else "ABOVE"))
    print("== scheduling counts, pass by pass")
    n = {"equal": 0, "in range": 0, "DIFFERS": 0, "outside": 0}
    for key in sorted(counts):
        a, b = counts[key].get("base", []), counts[key].get("new", [])
        if not a or not b:
            continue
        const = len(set(a)) == 1
        ok = all(x == a[0] for x in b) if const else all(min(a) <= x <= max(a) for x in b)
        what = ("equal" if ok else "DIFFERS") if const else ("in range" if ok else "outside")
        n[what] += 1
        if what != "equal":
            print("  %-8s %s: base %s -> new %s" % (what, " ".join(map(str, key)), a, b))
    print("the base's runs agree and the new build equals them: %(equal)d counts; they agree and it DIFFERS: %(DIFFERS)d; "
          "they vary and it lies inside / outside their range: %(in range)d / %(outside)d" % n)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "one":
        one(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5:])
    elif len(sys.argv) > 1 and sys.argv[1] == "native":
        native(sys.argv[2], int(sys.argv[3]), sys.argv[4])
    else:
        ap = argparse.ArgumentParser()
        ap.add_argument("cmd", choices=["run", "report"])
        ap.add_argument("args", nargs="+")
        ap.add_argument("--base-lib")
        ap.add_argument("--base-driver")
        ap.add_argument("--out", default="stream_ab.jsonl")
        a = ap.parse_args()
        if a.cmd == "report":
            report(a.args)
        else:
            run(a.args[0], {"base": os.path.abspath(a.base_lib), "new": os.path.join(ROOT, "mpc_amd", "csrc", "libgcengine.so")},
                {"base": a.base_driver and os.path.abspath(a.base_driver), "new": os.path.join(ROOT, "tools", "stream_driver")}, a.out)
