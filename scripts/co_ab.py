"""A/B of two builds of libgcengine.so on the Chou-Orlandi benchmarks: scripts/bench_co.py, scripts/bench_co_multi.py (with
and without --base-shapes) at their default shapes and, with --headline, python bench.py.  One child process per run (GC_LIB
selects the library), the two builds alternating, every JSON line of a child kept with `side`, `run` and `script` added.
Made for refactors of the CO kernels and their host side: "same speed" against the parent commit's build, judged by the
spread the parent shows against itself in the same session.

  co_ab.py run --base-lib PATH [--runs 2] [--headline] --out FILE
  co_ab.py report FILE

A child that fails ends the run.  Every child runs under a time limit of its own."""
import argparse
import json
import os
import statistics as st
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = (("bench_co", ["scripts/bench_co.py"], 240), ("bench_co_multi", ["scripts/bench_co_multi.py"], 300),
           ("bench_co_multi_base", ["scripts/bench_co_multi.py", "--base-shapes"], 300))
HEADLINE = ("bench", ["bench.py"], 600)


def child(side, lib, run, name, argv, limit, out):
    env = dict(os.environ)
    if lib:
        env["GC_LIB"] = lib
    r = subprocess.run([sys.executable] + argv, cwd=ROOT, env=env, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.exit("%s on side %s failed (%d):\n%s" % (name, side, r.returncode, r.stderr[-2000:]))
    with open(out, "a") as f:
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                f.write(json.dumps(dict(side=side, run=run, script=name, **json.loads(line))) + "\n")
    print("%s %s run %d done" % (side, name, run), flush=True)


def key(row):
    return tuple(str(row.get(k)) for k in ("script", "bench", "kernel", "call", "n", "S", "per"))


def report(path):
    """per row and timing (every `*ms_all` list of a line): the base's median run by run, the span of all its repetitions,
    and whether the new build's median lies within that span"""
    rows = {}
    for line in open(path):
        row = json.loads(line)
        for f, v in row.items():
            if f.endswith("ms_all"):
                rows.setdefault(key(row) + (f[:-4],), {}).setdefault(row["side"], []).append(v)
        if row["script"] == "bench" and "value" in row:
            print("bench.py %s: %s %s" % (row["side"], row["value"], row.get("unit", "")))
    worst = None
    for k, sides in sorted(rows.items()):
        if "base" not in sides or "new" not in sides:
            continue
        b, n = sum(sides["base"], []), sum(sides["new"], [])
        med, rel = st.median(n), st.median(n) / st.median(b) - 1
        name = " ".join(x for x in k if x != "None")
        print("%-56s base runs %s span %.4f .. %.4f  new runs %s  %+.2f%%  %s"
              % (name, ["%.4f" % st.median(r) for r in sides["base"]], min(b), max(b),
                 ["%.4f" % st.median(r) for r in sides["new"]], rel * 100, "inside" if min(b) <= med <= max(b) else "OUTSIDE"))
        if worst is None or rel > worst[0]:
            worst = (rel, name)
    if worst:
        print("worst row: %s %+.2f%%" % (worst[1], worst[0] * 100))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "report"])
    ap.add_argument("file", nargs="?")
    ap.add_argument("--base-lib")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--headline", action="store_true", help="python bench.py once per side as well")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.mode == "report":
        if not a.file:
            ap.error("report needs the FILE of a run")
        return report(a.file)
    if not a.base_lib or not os.path.exists(a.base_lib) or not a.out:
        ap.error("run needs --base-lib (an existing library of the parent commit) and --out")
    for run in range(a.runs):
        for name, argv, limit in SCRIPTS:
            for side, lib in (("base", a.base_lib), ("new", None)):
                child(side, lib, run, name, argv, limit, a.out)
    if a.headline:
        for side, lib in (("base", a.base_lib), ("new", None)):
            child(side, lib, 0, *HEADLINE, a.out)


if __name__ == "__main__":
    main()
