"""CPU check of the split rule of mpc_amd/csrc/stream_batch_windows.h (plan_split / commit_split), the ring state
behind gc_stream_batch_out_create_split: a step goes behind what the filling window holds and on into the windows after it, every
window that becomes full is sealed, none is sealed short and none grows.  The header is compiled alone into
tests/cpp/stream_batch_split_check.cpp with the host compiler under AddressSanitizer and UBSan (the pattern of
tests/test_stream_batch_windows.py; nothing is loaded into Python) and replays scripts of step(n) / flush / next / release; every
line it prints, the outcome of the event and the whole ring state, is compared with the model below.  (The first row of a piece
is found on the device, k_sb_serialise_range: there is no host table to check here.)"""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")

STEPS = (2552, 11526, 4158)  # the program of the GPU tests
HEADER = 20
WINDOWS = (4096, 5000, 1000, 18236)


class SplitModel:
    """the windows are used in index order and all have one size; a step of k bytes lies in ceil((off + k) / cap) windows from
    the filling one on, which must all be free; the ones it fills are sealed at cap bytes; windows come back in sealing order"""

    def __init__(self, window_bytes, n):
        self.c, self.n = (window_bytes + 15) // 16 * 16, n
        self.fill, self.off, self.sealed, self.out = 0, 0, [], []
        self.n_sealed = self.total = self.busy = self.split_steps = self.segments = 0

    def busy_windows(self):
        return len(self.sealed) + len(self.out)

    def seal(self):
        self.sealed.append((self.fill, self.off))
        self.n_sealed += 1
        self.fill, self.off = (self.fill + 1) % self.n, 0
        return "(%d %d)" % self.sealed[-1]

    def windows_of(self, k):
        return (self.off + k + self.c - 1) // self.c

    def step(self, k):
        if k > (self.n - 1) * self.c:
            return "s large"
        nwin = self.windows_of(k)
        if self.busy_windows() + nwin > self.n:
            self.busy += 1
            return "s busy"
        w, at, seals, left = self.fill, self.off, [], k
        for _ in range(nwin):
            take = min(left, self.c - self.off)
            self.off += take
            left -= take
            if self.off == self.c:
                seals.append(self.seal())
        assert left == 0
        self.total += k
        self.segments += nwin
        self.split_steps += nwin > 1
        return " ".join(["s ok %d %d %d" % (w, at, nwin)] + seals)

    def flush(self):
        return "f " + (self.seal() if self.busy_windows() < self.n and self.off else "none")

    def next(self):
        if not self.sealed:
            return "n none"
        self.out.append(self.sealed.pop(0))
        return "n (%d %d)" % self.out[-1]

    def release(self):
        return "r %d" % self.out.pop(0)[0] if self.out else "r none"

    def state(self):
        lens = [0] * self.n
        for w, k in self.sealed + self.out:
            lens[w] = k
        return " | %d %d %d %d | %d %d %d %d | %s | %s" % (
            self.fill if self.busy_windows() < self.n else -1, self.off, len(self.out), len(self.sealed), self.n_sealed, self.total,
            0, self.busy, " ".join([str(self.c)] * self.n), " ".join(map(str, lens)))

    def event(self, ev):
        head = {"f": self.flush, "n": self.next, "r": self.release}
        return (self.step(int(ev[2:])) if ev[0] == "s" else head[ev[0]]()) + self.state()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("stream_batch_split") / "stream_batch_split_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(CPP, "stream_batch_split_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def replay(program, runs):
    """runs: [(window_bytes, nwindows, [events])]; every printed line must be the model's"""
    script, want = [], []
    for wb, n, events in runs:
        m = SplitModel(wb, n)
        script.append("i %d %d" % (wb, n))
        want.append("i ok" + m.state())
        for ev in events:
            script.append(ev)
            want.append(m.event(ev))
    r = subprocess.run([program], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "event %d (%s): the ring says %r, the model %r" % (k, script[k], g, w)
    return want


def unchanged_but_busy(was, now, busy_more):
    """two state lines: windows, offset, sizes, lengths and every counter but `busy` are the same"""
    was, now = was.split("|"), now.split("|")
    assert now[1] == was[1] and now[3:] == was[3:]
    assert now[2].split()[:3] == was[2].split()[:3] and int(now[2].split()[3]) == int(was[2].split()[3]) + busy_more


def smallest_ring(window_bytes, largest_step):
    """the fewest windows with which a step of largest_step bytes is never refused as too large"""
    cap = (window_bytes + 15) // 16 * 16
    return max(2, (largest_step + cap - 1) // cap + 1)


@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("window_bytes", WINDOWS)
def test_the_program_of_the_gpu_tests(program, window_bytes, extra):
    """the three steps behind their headers, twice over, with a consumer that takes and returns a window whenever the garbler
    is told BUSY: every window but the flushed one is cap bytes long, and nothing grows"""
    n = smallest_ring(window_bytes, max(STEPS) + HEADER) + extra
    m, events = SplitModel(window_bytes, n), []

    def do(ev):
        events.append(ev)
        return m.event(ev)

    lens = []
    for k in list(STEPS) * 2:
        while do("s %d" % (k + HEADER)).startswith("s busy"):
            line = do("n")
            assert line.startswith("n (") and not do("r").startswith("r none")
            lens.append(int(line.split()[2].rstrip(")")))
    flushed = do("f")
    while True:
        line = do("n")
        if line.startswith("n none"):
            break
        lens.append(int(line.split()[2].rstrip(")")))
        do("r")
    total = 2 * sum(k + HEADER for k in STEPS)
    assert sum(lens) == total and all(x == m.c for x in lens[:-1])
    assert lens[-1] == (total % m.c or m.c) and flushed.startswith("f none") == (total % m.c == 0)
    if window_bytes < 18236:
        assert m.split_steps > 0
    if window_bytes == 1000:
        assert m.c == 1008 and n == 13 + extra  # the middle step lies in 12 windows
    replay(program, [(window_bytes, n, events)])


def test_directed_edges(program):
    cap, n = 4096, 4
    events = ["s 4096",            # 1: fills the window exactly: one window, sealed, no empty window touched
              "s 100", "s 12188",  # 2, 3: ends exactly at the end of the third window from here: all three sealed, no fourth
              "s 1",               # 4: every window is sealed: busy
              "n", "r", "n", "r", "n", "r", "n", "r",  # 5 - 12
              "s 12288",           # 13: (nwindows - 1) * cap: accepted, three windows
              "s 12289",           # 14: one more: too large
              "n", "r",            # 15, 16
              "s 12289",           # 17: ... whatever is free
              "s 10", "s 8182",    # 18, 19: windows 3 and 0, both exactly full
              "n", "r",            # 20, 21
              "s 8182",            # 22: window 1 is free and empty, window 2 is not: busy
              "s 4096",            # 23
              "f"]                 # 24: nothing to flush
    lines = replay(program, [(cap, n, events)])  # lines[k] is the outcome of events[k - 1]
    assert lines[1].startswith("s ok 0 0 1 (0 4096) | 1 0 ")
    assert lines[2].startswith("s ok 1 0 1 | 1 100 ")
    assert lines[3].startswith("s ok 1 100 3 (1 4096) (2 4096) (3 4096) | -1 0 ")
    assert lines[4].startswith("s busy")
    unchanged_but_busy(lines[3], lines[4], 1)
    assert lines[13].startswith("s ok 0 0 3 (0 4096) (1 4096) (2 4096) | 3 0 ")
    for k in (14, 17):
        assert lines[k].startswith("s large"), k
        unchanged_but_busy(lines[k - 1], lines[k], 0)
    assert lines[18].startswith("s ok 3 0 1 | 3 10 ")
    assert lines[19].startswith("s ok 3 10 2 (3 4096) (0 4096) | -1 0 ")
    assert lines[22].startswith("s busy")
    unchanged_but_busy(lines[21], lines[22], 1)
    assert lines[23].startswith("s ok 1 0 1 (1 4096) | -1 0 ") and lines[24].startswith("f none")


def test_busy_with_exactly_k_minus_1_windows_free(program):
    """a step of k windows with the filling one and k - 2 behind it free: busy, nothing but the counter moves, and the step that
    needs one window fewer is exact"""
    n = 5
    events = ["s 1008", "s 1008", "s 8",  # 1 - 3: windows 0, 1 sealed; window 2 fills; 3 and 4 free
              "n",                        # 4: window 0 handed out
              "s 2017",                   # 5: 8 + 2017 = 2 * 1008 + 9: windows 2, 3, 4
              "s 1000",                   # 6: window 4 holds 9: 1 009 bytes need window 0 too, which is handed out: busy
              "s 999",                    # 7: ... but 999 fill window 4 exactly
              "s 1",                      # 8: no filling window: busy
              "r", "s 1",                 # 9, 10: window 0 fills
              "n", "r",                   # 11, 12: window 1 is free as well
              "s 2016",                   # 13: 1 + 2016 bytes lie in three windows, two are free: busy
              "s 2015"]                   # 14: two windows, both exactly full
    lines = replay(program, [(1000, n, events)])
    assert lines[5].startswith("s ok 2 8 3 (2 1008) (3 1008) | 4 9 ")
    assert lines[7].startswith("s ok 4 9 1 (4 1008) | -1 0 ")
    assert lines[10].startswith("s ok 0 0 1 | 0 1 ")
    for k in (6, 8, 13):
        assert lines[k].startswith("s busy"), k
        unchanged_but_busy(lines[k - 1], lines[k], 1)
    assert lines[14].startswith("s ok 0 1 2 (0 1008) (1 1008) | -1 0 ")


def test_fewer_than_two_windows_are_refused(program):
    r = subprocess.run([program], input="i 4096 1\ni 4096 0\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.splitlines() == ["i refused", "i refused"]


def test_ten_thousand_random_sequences(program):
    rng = random.Random(21)
    runs = []
    for _ in range(10000):
        cap = rng.choice(WINDOWS + (16, 64, 4097))
        n = rng.choice((2, 2, 3, 3, 4, 7, 13))
        real = (cap + 15) // 16 * 16
        sizes = (1, 15, 16, real // 2, real - 1, real, real + 1, 3 * real, (n - 1) * real, (n - 1) * real + 1, STEPS[0] + HEADER,
                 STEPS[1] + HEADER, STEPS[2] + HEADER)
        events = []
        for _ in range(rng.randrange(5, 40)):
            x = rng.random()
            events.append("s %d" % (rng.choice(sizes) if rng.random() < 0.7 else rng.randrange(1, 2 * real + 2)) if x < 0.5
                          else "f" if x < 0.6 else "n" if x < 0.8 else "r")
        runs.append((cap, n, events))
    lines = replay(program, runs)
    text = "\n".join(lines)
    assert len(lines) > 200000
    for word in ("s busy", "s large", "r none", "n none", "f none"):
        assert word in text, word
    ok = [ln.split() for ln in lines if ln.startswith("s ok")]
    assert sum(1 for f in ok if int(f[4]) > 1) > 1000  # steps were cut, often
    assert all(ln.split("|")[2].split()[2] == "0" for ln in lines if "|" in ln)  # grown stays 0
