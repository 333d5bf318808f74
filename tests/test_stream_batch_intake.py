"""CPU check of mpc_amd/csrc/stream_batch_intake.h, the framing state behind gc_stream_eval_batch_in_* (DESIGN.md §20): what is
held of an unfinished message, where the next one starts, what a feed of n bytes does, the cap on the carry, the stop in front
of an op that is not OpCircuit, and the four counters.  The header is compiled alone into
tests/cpp/stream_batch_intake_check.cpp with the host compiler under AddressSanitizer and UBSan (the pattern of
tests/test_stream_batch_windows.py; nothing is loaded into Python) and replays scripts of messages and chunk lengths; every
line it prints — the outcome of the feed, the counters, the carry and every message it evaluated, by stream offset — is
compared with the model below, which works on stream offsets alone and holds no buffer."""
import os
import random
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")

HEADER = 20
GC_E_ROWS = -4


class Model:
    """items: ("M", len, numGates) / ("F", op, len).  A feed sees the stream from the start of the open message to pos + n"""

    def __init__(self, cap, items):
        self.cap, self.items, self.at_start = cap, [], {}
        off = 0
        for k, it in enumerate(items):
            n = it[1] if it[0] == "M" else it[2]
            self.items.append((it[0], off, n, it[1] if it[0] == "F" else 1, it[2] if it[0] == "M" else 0, k))
            self.at_start[off] = self.items[-1]
            off += n
        self.total, self.pos, self.held = off, 0, 0
        self.steps = self.bytes = self.uploads = self.carried = 0
        self.reported = []

    def feed(self, n):
        n = min(n, self.total - self.pos)
        if n == 0:
            return "c end"
        lo, hi = self.pos - self.held, self.pos + n
        at, msgs, rc, op, stop = lo, [], 0, 1, None
        while True:
            it, avail = self.at_start.get(at), hi - at
            if it is None or avail < 4:
                break
            if it[0] == "F":
                op, stop = it[3], it
                break
            if avail < HEADER:
                break
            if 5 * it[4] + HEADER > self.cap:
                rc, stop = GC_E_ROWS, it
                break
            if avail < it[2]:
                break
            msgs.append(it)
            at += it[2]
        if stop is None and hi - at > self.cap:
            rc, stop = GC_E_ROWS, self.at_start[at]
        if stop is None:
            taken, carry = n, hi - at
        else:
            taken, carry = max(at - self.pos, 0), 0
        self.steps += len(msgs)
        self.bytes += at - lo
        self.uploads += 1
        self.carried += carry
        self.held = carry
        self.pos += taken
        if stop is not None:
            self.pos = stop[1] + stop[2]
        self.reported += [m[5] for m in msgs]
        return "%d %d %d %d | %d %d %d %d |%s" % (rc, taken, op, carry, self.steps, self.bytes, self.uploads, self.carried,
                                                  "".join(" %d:%d:%d" % (m[1], m[2], m[5]) for m in msgs))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("stream_batch_intake") / "stream_batch_intake_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(CPP, "stream_batch_intake_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def replay(program, runs):
    """runs: [(cap, items, chunk lengths or a function() -> next chunk length)]; every printed line must be the model's.
    Returns [(model, lines)]"""
    script, want, out = [], [], []
    for cap, items, chunks in runs:
        m = Model(cap, items)
        script.append("i %d" % cap)
        want.append("i ok")
        script += ["%s %d %d" % it for it in items]
        mine = []
        if callable(chunks):
            while m.pos < m.total:
                n = chunks()
                script.append("c %d" % n)
                mine.append(m.feed(n))
        else:
            for n in chunks:
                script.append("c %d" % n)
                mine.append(m.feed(n))
        want += mine
        out.append((m, mine))
    r = subprocess.run([program], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "line %d: the intake says %r, the model %r" % (k, g, w)
    return out


def test_the_header_makes_no_hip_call():
    text = open(os.path.join(CSRC, "stream_batch_intake.h")).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert "hip" not in code.lower()
    assert re.findall(r'#include "([^"]+)"', code) == ["../../include/gcengine.h"]


def test_a_cap_below_one_header_is_refused(program):
    r = subprocess.run([program], input="i 19\ni 0\ni 20\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.splitlines() == ["i refused", "i refused", "i ok"]


def test_directed_cuts(program):
    """three messages and an OpReturn behind them: whole; byte by byte; a cut at every position of the first two messages"""
    items = [("M", 24, 0), ("M", 300, 3), ("M", 20, 0), ("F", 2, 44), ("M", 77, 1)]
    total = 24 + 300 + 20 + 44 + 77
    runs = [(5000, items, [total, total]), (5000, items, [1] * total)]
    runs += [(5000, items, [cut, total, total]) for cut in range(1, 24 + 300 + 1)]
    out = replay(program, runs)
    for m, lines in out:
        assert m.reported == [0, 1, 2, 4] and m.pos == m.total and m.steps == 4 and m.bytes == total - 44
    whole = out[0][1]
    assert whole[0].startswith("0 344 2 0 | 3 344 1 0 | 0:24:0 24:300:1 324:20:2")  # stops in front of the word
    assert whole[1].startswith("0 77 1 0 | 4 421 2 0 | 388:77:4")                 # ... and goes on at a fresh OpCircuit
    bytewise = [ln for ln in out[1][1] if ln != "c end"]
    assert sum(1 for ln in bytewise if ln.split()[2] == "2") == 1 and out[1][0].uploads == total - 44 + 4
    # the op word of the OpReturn across two chunks: the second feed takes nothing and reports the op
    m, lines = replay(program, [(5000, items, [346, 100, 100])])[0]
    assert lines[0].startswith("0 346 1 2 |") and lines[1].startswith("0 0 2 0 |") and lines[2].startswith("0 77 1 0 |")


def test_the_cap(program):
    """a message longer than the cap is refused when its carry would pass the cap, not before; a header that claims more gates
    than the cap holds is refused as soon as it is complete; the stream goes on behind either"""
    items = [("M", 100, 0), ("M", 3000, 0), ("M", 50, 0), ("M", 60, 200), ("M", 40, 0)]
    m, lines = replay(program, [(1000, items, [600, 500, 1, 5000, 5000, 5000])])[0]
    assert lines[0].startswith("0 600 1 500 | 1 100 1 500 | 0:100:0")
    assert lines[1].startswith("0 500 1 1000 | 1 100 2 1500 |")      # exactly the cap: still held
    assert lines[2].startswith("%d 0 1 0 | 1 100 3 1500 |" % GC_E_ROWS)  # one byte more
    assert lines[3].startswith("%d 50 1 0 | 2 150 4 1500 | 3100:50:2" % GC_E_ROWS)  # 5 * 200 + 20 > 1000
    assert lines[4].startswith("0 40 1 0 | 3 190 5 1500 | 3210:40:4") and m.reported == [0, 2, 4]


def test_ten_thousand_random_sequences(program):
    rng = random.Random(20)
    runs = []
    for _ in range(10000):
        cap = rng.choice((5000, 5000, 8192, 1 << 20, 2000, 600, 100))
        items = []
        for _ in range(rng.randrange(1, 9)):
            if rng.random() < 0.15:
                items.append(("F", rng.choice((0, 2, 2, 3, 7, 0xFFFFFFFF, 0x01000000)), rng.randrange(4, 200)))
            else:
                n = rng.choice((HEADER, 24, 25, 5000)) if rng.random() < 0.2 else rng.randrange(24, 5001)
                items.append(("M", n, rng.choice((0, 0, 0, 1, 17, 99, 400, 5000, 0xFFFFFFFF))))
        style = rng.random()
        if style < 0.02:
            chunks = lambda: 1  # noqa: E731
        elif style < 0.1:
            k = rng.randrange(2, 64)
            chunks = lambda k=k: k  # noqa: E731
        else:
            chunks = lambda: rng.choice((1, 3, 4, 19, 20, 21, 4096, 8192)) if rng.random() < 0.3 else rng.randrange(1, 8193)  # noqa: E731
        runs.append((cap, items, chunks))
    out = replay(program, runs)
    lines = [ln for _, mine in out for ln in mine]
    rows = sum(1 for ln in lines if ln.startswith("%d " % GC_E_ROWS))
    stops = sum(1 for ln in lines if ln.split()[2] != "1")
    straddled = sum(1 for ln in lines if ln.split()[2] != "1" and ln.split()[1] == "0")
    carried = sum(1 for ln in lines if ln.split()[3] != "0")
    assert len(lines) > 100000 and rows > 1000 and stops > 1000 and straddled > 20 and carried > 50000
    for m, _ in out:  # every message that is not refused is reported once and in order, and nothing is left over
        ok = [it[5] for it in m.items if it[0] == "M" and 5 * it[4] + HEADER <= m.cap]
        assert m.pos == m.total and m.reported == sorted(m.reported) and set(m.reported) <= set(ok)
        assert len(m.reported) == len(set(m.reported)) == m.steps
        if m.cap >= 5000:
            assert m.reported == ok
