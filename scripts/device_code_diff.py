#!/usr/bin/env python3
"""device_code_diff.py <tree A> <tree B>: is the device code of two checkouts the same?

Every .hip file under mpc_amd/csrc is compiled to gfx950 assembly in both trees (device pass only, the flags of the
tests/test_*_kernel_resources.py files), the output is cut at the kernel symbols, and per file the script reports whether
  * the sets of .amdhsa_kernel names are equal, and
  * every kernel's text (its label up to its .Lfunc_end) and its .amdhsa_kernel block are equal.
Kernels are compared by NAME: a host-side change may reorder the template instantiations.  Not compared: .ident, comments
(they carry file paths and block numbers) and the numbers of local labels (.LBB<function>_<block>, .Lfunc_end<function>,
.Ltmp<n>), which count functions in the order of the file: they are renumbered per kernel in order of appearance.

Prints one line per file and exits 0 only if every file is identical.  A host refactor is checked with
    git worktree add ../parent HEAD~1 && python scripts/device_code_diff.py ../parent .
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S"]
LOCAL_LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)*")


def assembly(tree, name, out):
    src = os.path.join(tree, "mpc_amd", "csrc", name)
    r = subprocess.run([HIPCC] + FLAGS + [src, "-o", out], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s: hipcc failed\n%s" % (src, r.stderr[-4000:]))
    with open(out) as f:
        return f.read().splitlines()


def normalise(lines):
    """drop .ident and comments; renumber local labels in order of appearance"""
    seen = {}
    out = []
    for line in lines:
        s = line.split(";")[0].strip()
        if not s or s.startswith(".ident"):
            continue
        out.append(LOCAL_LABEL.sub(lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), s))
    return out


def kernels(lines):
    """{kernel name: normalised text + descriptor block}"""
    names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    found = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        d0 = next(i for i, l in enumerate(lines) if l.strip() == ".amdhsa_kernel " + name)
        d1 = next(i for i in range(d0, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        found[name] = normalise(lines[start:end + 1]) + normalise(lines[d0:d1 + 1])
    return found


def compare(job):
    a, b, name, tmp = job
    if not (os.path.exists(os.path.join(a, "mpc_amd", "csrc", name)) and os.path.exists(os.path.join(b, "mpc_amd", "csrc", name))):
        return name, False, "DIFFERENT: the file is in one tree only"
    ka = kernels(assembly(a, name, os.path.join(tmp, "a_" + name + ".s")))
    kb = kernels(assembly(b, name, os.path.join(tmp, "b_" + name + ".s")))
    if set(ka) != set(kb):
        only = sorted(set(ka) ^ set(kb))
        return name, False, "DIFFERENT: %d / %d kernels, in one tree only: %s" % (len(ka), len(kb), " ".join(only[:8]))
    changed = sorted(k for k in ka if ka[k] != kb[k])
    if changed:
        return name, False, "DIFFERENT: %d of %d kernels differ: %s" % (len(changed), len(ka), " ".join(changed[:8]))
    return name, True, "identical, %d kernels in A, %d in B" % (len(ka), len(kb))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1), help="compilations at a time")
    args = ap.parse_args()
    names = sorted({n for t in (args.tree_a, args.tree_b) for n in os.listdir(os.path.join(t, "mpc_amd", "csrc")) if n.endswith(".hip")})
    print("device code, A against B: hipcc %s, kernels compared by name" % " ".join(FLAGS))
    ok = True
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(args.j) as pool:
        for name, same, text in pool.map(compare, [(args.tree_a, args.tree_b, n, tmp) for n in names]):
            ok &= same
            print("%-40s %s" % (name, text), flush=True)
    print("ALL IDENTICAL: %d files" % len(names) if ok else "NOT IDENTICAL")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
