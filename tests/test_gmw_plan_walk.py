"""Host walk of the GMW plan (mpc_amd/csrc/gmw_plan.cpp) on the CPU.  tests/cpp/gmw_plan_walk.cpp is compiled with the host
compiler together with gmw_plan.cpp itself and walks gc::GmwPlan as the kernels do (input load; per round the close of the
previous AND level, the free gates sub-round by sub-round, the open of the round's AND level, the outputs last).  What it
prints — every party's messages with their padding bits, (level, words) per round, the output shares — is compared bit for
bit with the restated reference (tests/py_gmw_reference.py: run_parties), and the XOR of the output shares with the plaintext
in the bucketed order.  While walking it enforces what k_gmw_step relies on between two workgroup barriers: every slot is
below nslots and written once per pass, every read is of a slot written in a strictly earlier phase, and the rounds, sub-round
offsets and slot lists are laid out as gmw_engine.cpp indexes them.  No GPU needed."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import gmw_cases as G
from tests import py_gmw_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_amd", "csrc")
WALK = os.path.join(ROOT, "tests", "cpp", "gmw_plan_walk.cpp")
HIP_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")  # gmw.h includes hip/hip_runtime.h


def _case_bytes(c, P, n, shares, trip):
    tw = R.triple_words(c)[2]
    parts = [struct.pack("<7I", c.NumGates, c.NumWires, c.num_inputs, c.num_outputs, P, n, tw), np.ascontiguousarray(c.Gates).tobytes()]
    for p in range(P):
        parts.append(np.ascontiguousarray(shares[p], np.uint64).tobytes())
        for t in trip[p]:
            parts.append(np.ascontiguousarray(t, np.uint64).tobytes())
    return b"".join(parts)


def _parse(text):
    """[dict(rc, plan, rounds=[(level, words)], msgs={q: [words]}, outs={q: words}, bad=[text], nbad)] per case"""
    cases = []
    for line in text.splitlines():
        t = line.split()
        if t[0] == "case":
            assert int(t[1]) == len(cases)
            cases.append(dict(rc=int(t[3]), plan=None, rounds=[], msgs={}, outs={}, bad=[], nbad=None))
            continue
        cur = cases[-1]
        if t[0] == "plan":
            cur["plan"] = tuple(int(x) for x in t[1:])
        elif t[0] == "round":
            assert int(t[1]) == len(cur["rounds"])
            cur["rounds"].append((int(t[2]), int(t[3])))
        elif t[0] == "msg":
            cur["msgs"].setdefault(int(t[1]), []).append(np.array([int(x, 16) for x in t[2:]], np.uint64))
        elif t[0] == "out":
            cur["outs"][int(t[1])] = np.array([int(x, 16) for x in t[2:]], np.uint64)
        elif t[0] == "bad":
            cur["bad"].append(line)
        elif t[0] == "end":
            assert int(t[1]) == len(cases) - 1
            cur["nbad"] = int(t[2])
        else:
            raise AssertionError("unknown line: " + line)
    return cases


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    d = tmp_path_factory.mktemp("gmw_plan_walk")
    exe = d / "gmw_plan_walk"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-isystem",
                        HIP_INCLUDE, WALK, os.path.join(CSRC, "gmw_plan.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    count = [0]

    def go(blobs, *extra, expect_clean=True):
        count[0] += 1
        f = d / ("cases_%d.bin" % count[0])
        f.write_bytes(b"".join(blobs))
        r = subprocess.run([str(exe), str(f)] + list(extra), capture_output=True, text=True, timeout=300)
        assert r.returncode in (0, 1), r.stderr
        cases = _parse(r.stdout)
        assert len(cases) == len(blobs)
        if expect_clean:
            assert r.returncode == 0, [c["bad"] for c in cases if c["bad"]][:3]
        return cases

    return go


def _check(c, P, n, bits, shares, trip, got, what):
    """one walked case against the restated reference, every instance"""
    assert got["rc"] == 0 and got["nbad"] == 0 and not got["bad"], (what, got["rc"], got["bad"][:5])
    ands, _ = R.buckets(c)
    n_and_levels = sum(1 for a in ands if a)
    assert got["plan"] == (c.num_inputs + c.NumGates, n_and_levels + 1, len(ands), n_and_levels), what
    ref_msgs, ref_outs = R.run_parties(c, shares, trip)
    want_rounds = [(lv, m.shape[1]) for lv, m in ref_msgs[0]] + [(len(ands), 0)]  # the closing round: nlevels, no words
    assert got["rounds"] == want_rounds, what
    for p in range(P):
        msgs = got["msgs"][p]
        assert len(msgs) == len(want_rounds) and msgs[-1].size == 0, what
        for (lv, rm), m in zip(ref_msgs[p], msgs):
            assert m.size == rm.size and (m.reshape(rm.shape) == rm).all(), "%s: party %d level %d: message differs" % (what, p, lv)
        assert (got["outs"][p].reshape(ref_outs[p].shape) == ref_outs[p]).all(), "%s: party %d: output shares differ" % (what, p)
    x = np.bitwise_xor.reduce(np.stack([got["outs"][p].reshape(ref_outs[p].shape) for p in range(P)]), axis=0)
    ob = R.unpack(x, c.num_outputs)
    for i in range(n):
        assert (ob[:, i] == R.plain_bucketed(c, bits[i])).all(), "%s: instance %d: plaintext differs" % (what, i)
    assert (G.plain_bucketed_batch(c, bits) == ob).all(), what  # the batched restatement the GPU tests use agrees


FUZZ_CHUNK = 100
INSTANCES = (1, 2, 3, 5)  # and 64, a full slot word, for one seed in twenty


@pytest.mark.parametrize("first", range(0, G.N_FUZZ, FUZZ_CHUNK))
def test_fuzz_circuits(walk, first):
    """1 000 seeded circuits, 100 per process: P 2 .. 5, reuse 0 .. 0.6, p_and 0 .. 0.9, 1 / 2 / 3 / 5 / 64 instances"""
    cases, blobs = [], []
    for seed in range(first, first + FUZZ_CHUNK):
        c, P = G.fuzz_case(seed)
        n = 64 if seed % 20 == 7 else INSTANCES[(seed // 5) % 4]
        bits, shares, trip = G.pass_data(c, P, n, 9000 + seed)
        cases.append((c, P, n, bits, shares, trip))
        blobs.append(_case_bytes(c, P, n, shares, trip))
    for seed, case, got in zip(range(first, first + FUZZ_CHUNK), cases, walk(blobs)):
        _check(*case, got, "fuzz seed %d" % seed)


def test_fuzz_parameters_cover_the_grid():
    seen = set()
    for seed in range(80):
        seen.add((2 + seed % 4, G.REUSE[(seed // 4) % 4], G.P_AND[(seed // 16) % 5]))
    assert len(seen) == 80 and G.N_FUZZ >= 1000


def test_shipped_circuits(walk, aes_circ, add64_circ):
    cases, blobs = [], []
    for k, (c, P, n) in enumerate(((aes_circ, 2, 3), (aes_circ, 5, 2), (add64_circ, 2, 64), (add64_circ, 3, 2))):
        bits, shares, trip = G.pass_data(c, P, n, 300 + k)
        cases.append((c, P, n, bits, shares, trip))
        blobs.append(_case_bytes(c, P, n, shares, trip))
    for k, (case, got) in enumerate(zip(cases, walk(blobs))):
        _check(*case, got, "shipped %d" % k)
        c, bits = case[0], case[3]
        x = np.bitwise_xor.reduce(np.stack([got["outs"][p] for p in range(case[1])]), axis=0).reshape(-1, case[2])
        ob = R.unpack(x, c.num_outputs)  # no wire reuse here: circuit order gives the same result
        assert (ob[:, 0] == c.compute_bits(bits[0])[c.NumWires - c.num_outputs:]).all()


@pytest.mark.parametrize("n", [1, 64])
def test_directed_circuits(walk, n):
    cases, blobs = [], []
    for k, (c, status) in enumerate(G.directed()):
        P = G.directed_parties(k)
        bits, shares, trip = G.pass_data(c, P, n, 500 + k)
        cases.append((c, P, n, bits, shares, trip, status))
        blobs.append(_case_bytes(c, P, n, shares, trip))
    names = set()
    for case, got in zip(cases, walk(blobs)):
        c, status = case[0], case[6]
        names.add(c.name)
        if status:
            assert got["rc"] == status and got["plan"] is None, c.name
        else:
            _check(*case[:6], got, c.name)
    assert len(names) == len(cases) >= 15


def test_directed_circuits_pin_what_they_say():
    """the two reuse circuits differ between the bucketed order and circuit order on some input, so a planner that renamed
    along circuit order would fail them; the level shapes are the ones named"""
    by_name = {c.name: c for c, _ in G.directed()}
    for name in ("free_gate_before_and_of_its_level", "ands_read_before_they_write"):
        c = by_name[name]
        diff = 0
        for v in range(1 << c.num_inputs):
            bits = [(v >> i) & 1 for i in range(c.num_inputs)]
            diff += int((R.plain_bucketed(c, bits) != c.compute_bits(bits)[c.NumWires - c.num_outputs:]).any())
        assert diff, name
    for n in (64, 65, 128):
        ands, _ = R.buckets(by_name["one_level_%d_ands" % n])
        assert [len(a) for a in ands] == [n, 0]
    ands, rest = R.buckets(by_name["and_on_last_level"])
    assert [len(a) for a in ands] == [1, 0] and [len(x) for x in rest] == [1, 0]
    ands, rest = R.buckets(by_name["ands_only"])
    assert [len(a) for a in ands] == [2, 1, 0] and not any(rest)
    ands, rest = R.buckets(by_name["ands_read_before_they_write"])
    assert [len(a) for a in ands] == [2, 0] and [len(x) for x in rest] == [1, 1]
    assert [by_name["noutputs_%d" % k].num_outputs for k in (0, 64, 65)] == [0, 64, 65]


def test_the_checks_fire_on_a_spoilt_plan(walk, aes_circ):
    """the walker's own switch folds the second sub-round of every round into the first (a dropped barrier): the hazard check
    must report reads in the phase that writes, on aes_128 and on a reuse circuit"""
    blobs = []
    for k, (c, P) in enumerate(((aes_circ, 2), G.fuzz_case(40))):
        _, shares, trip = G.pass_data(c, P, 2, 700 + k)
        blobs.append(_case_bytes(c, P, 2, shares, trip))
    for got in walk(blobs, "merge-sub-rounds", expect_clean=False):
        assert got["rc"] == 0 and got["nbad"] > 0
        assert any("the phase that writes it" in b for b in got["bad"])
