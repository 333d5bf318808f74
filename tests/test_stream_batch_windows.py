"""CPU check of mpc_amd/csrc/stream_batch_windows.h, the ring state behind gc_stream_batch_out_* (DESIGN.md §18): which window
fills and where, what a step of n bytes does, sealed / handed-out / free, growth and the four counters.  The header is compiled
alone into tests/cpp/stream_batch_windows_check.cpp with the host compiler under AddressSanitizer and UBSan (the pattern of
tests/test_host_staging.py; nothing is loaded into Python) and replays scripts of step(n) / flush / next / release; every line it
prints — the outcome of the event and the whole ring state — is compared with the model below.  A second test checks that the
bindings and the header agree on the new prototypes."""
import os
import random
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")

STEPS = (2552, 11526, 4158)  # tests/test_stream_batch_host.STEP_BYTES[0]: the program of the GPU tests
HEADER = 20                  # the OpCircuit header the GPU tests put in front of every step
CAPS = (18236, 14078, 11526, 4096)


class Model:
    """the windows are used in index order; a step goes behind what the filling window holds, else into the next one, which
    must be free; only an empty window grows; windows come back in the order they were sealed"""

    def __init__(self, window_bytes, n):
        self.cap, self.n = [(window_bytes + 15) // 16 * 16] * n, n
        self.fill, self.off, self.sealed, self.out = 0, 0, [], []
        self.n_sealed = self.total = self.grown = self.busy = 0

    def busy_windows(self):
        return len(self.sealed) + len(self.out)

    def seal(self):
        self.sealed.append((self.fill, self.off))
        self.n_sealed += 1
        self.fill, self.off = (self.fill + 1) % self.n, 0
        return "(%d %d)" % self.sealed[-1]

    def step(self, k):
        moves = self.off != 0 and self.off + k > self.cap[self.fill]
        if self.busy_windows() + (1 if moves else 0) >= self.n:
            self.busy += 1
            return "s busy"
        seals = [self.seal()] if moves else []
        grow = 0
        if k > self.cap[self.fill]:
            assert self.off == 0
            grow = self.cap[self.fill] = (k + 4095) // 4096 * 4096
            self.grown += 1
        w, at = self.fill, self.off
        self.off += k
        self.total += k
        if self.off == self.cap[w]:
            seals.append(self.seal())
        return " ".join(["s ok %d %d %d" % (w, at, grow)] + seals)

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
            self.grown, self.busy, " ".join(map(str, self.cap)), " ".join(map(str, lens)))

    def event(self, ev):
        head = {"s": self.step, "f": lambda: self.flush(), "n": lambda: self.next(), "r": lambda: self.release()}
        return (self.step(int(ev[2:])) if ev[0] == "s" else head[ev[0]]()) + self.state()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("stream_batch_windows") / "stream_batch_windows_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(CPP, "stream_batch_windows_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def replay(program, runs):
    """runs: [(window_bytes, nwindows, [events])]; every printed line must be the model's"""
    script, want = [], []
    for wb, n, events in runs:
        m = Model(wb, n)
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


def test_the_header_makes_no_hip_call():
    text = open(os.path.join(CSRC, "stream_batch_windows.h")).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert "hip" not in code and "#include \"" not in code


@pytest.mark.parametrize("nwindows", [2, 3])
@pytest.mark.parametrize("cap", CAPS)
def test_the_program_of_the_gpu_tests(program, cap, nwindows):
    """the three steps behind their headers, twice over, with a consumer that takes and returns a window whenever the garbler
    is told BUSY; then the directed edges: a step of cap exactly, of cap + 1, flush on an empty window, release with nothing out"""
    m, events = Model(cap, nwindows), []

    def do(ev):
        events.append(ev)
        return m.event(ev)

    for k in list(STEPS) * 2:
        while do("s %d" % (k + HEADER)).startswith("s busy"):
            assert do("n").startswith("n (") and not do("r").startswith("r none")
    do("f")
    while not do("n").startswith("n none"):
        do("r")
    assert do("r").startswith("r none")        # release with nothing out
    assert do("f").startswith("f none")        # flush on an empty window
    w, c = m.fill, m.cap[m.fill]
    assert do("s %d" % c).startswith("s ok %d 0 0 (%d %d)" % (w, w, c))  # exactly full: sealed, not grown
    before, w, k = m.grown, m.fill, m.cap[m.fill] + 1
    line = do("s %d" % k)                      # one byte more than an empty window: it grows, to a multiple of 4 096
    assert line.startswith("s ok %d 0 %d" % (w, (k + 4095) // 4096 * 4096)) and m.grown == before + 1
    do("s 1"), do("f"), do("n"), do("n"), do("r"), do("r"), do("r")
    want = replay(program, [(cap, nwindows, events)])
    if cap == 4096:  # steps 1 and 2 exceed the window, header included, and each lands on a fresh empty window
        first_pass = [w for w in want[1:] if w.startswith("s ok")][:3]
        assert [int(w.split()[4]) for w in first_pass] == [0, 12288, 8192]


def test_busy_changes_nothing_but_its_counter(program):
    events = ["s 4096", "s 4096", "s 1", "s 5000", "n", "s 1", "r", "s 1", "s 4096", "n", "n", "r", "r", "r", "f"]
    lines = replay(program, [(4096, 2, events)])  # lines[0] is the new ring, lines[k] the outcome of events[k - 1]
    for k in (3, 4, 6, 9):
        assert lines[k].startswith("s busy"), k
        was, now = lines[k - 1].split("|"), lines[k].split("|")
        assert now[1] == was[1] and now[3:] == was[3:]                      # windows, offset, sizes and lengths: unchanged
        assert now[2].split()[:3] == was[2].split()[:3] and int(now[2].split()[3]) == int(was[2].split()[3]) + 1
    # a partly filled window and no free one behind it: BUSY, and the byte stays where it is until flush seals it
    assert lines[8].startswith("s ok 0 0 0") and lines[15].startswith("f (0 1)")
    assert lines[13].startswith("r none") and lines[11].startswith("n none")


def test_fewer_than_two_windows_are_refused(program):
    r = subprocess.run([program], input="i 4096 1\ni 4096 0\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.splitlines() == ["i refused", "i refused"]


def test_ten_thousand_random_sequences(program):
    rng = random.Random(18)
    runs = []
    for _ in range(10000):
        cap = rng.choice(CAPS + (16, 64, 1000, 4097))
        n = rng.choice((2, 2, 3, 3, 4, 7))
        real = (cap + 15) // 16 * 16
        sizes = (1, 15, 16, real // 2, real - 1, real, real + 1, 3 * real, STEPS[0] + HEADER, STEPS[1] + HEADER, STEPS[2] + HEADER)
        events = []
        for _ in range(rng.randrange(5, 40)):
            x = rng.random()
            events.append("s %d" % (rng.choice(sizes) if rng.random() < 0.7 else rng.randrange(1, 2 * real + 2)) if x < 0.5
                          else "f" if x < 0.6 else "n" if x < 0.8 else "r")
        runs.append((cap, n, events))
    lines = replay(program, runs)
    text = "\n".join(lines)
    assert len(lines) > 200000 and "s busy" in text and "r none" in text and "n none" in text and "f none" in text
    assert sum(1 for ln in lines if ln.startswith("s ok") and ln.split()[4] != "0") > 1000  # growth happened, often


def _protos(names):
    text = open(os.path.join(ROOT, "include", "gcengine.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(gc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        if m.group(1) in names:
            out[m.group(1)] = ["ptr" if "*" in p else "scalar" for p in m.group(2).split(",")]
    return out


NEW = ("gc_stream_batch_select_labels_dev", "gc_stream_batch_decode_dev", "gc_stream_batch_select_labels", "gc_stream_batch_decode",
       "gc_stream_batch_out_create", "gc_stream_batch_out_free", "gc_stream_batch_out_garble", "gc_stream_batch_out_flush",
       "gc_stream_batch_out_next", "gc_stream_batch_out_release", "gc_stream_batch_out_stats", "gc_stream_eval_batch_circuit_host",
       "gc_stream_eval_batch_uploads_wait", "gc_stream_eval_batch_bad")


def test_bindings_and_header_agree_on_the_new_prototypes():
    """every new entry point is declared, exported, bound in Python with as many arguments of the same kind (pointer or scalar)
    as the header gives it, named by the C++ wrapper and called from the Go stub; GC_E_BUSY is -10 everywhere"""
    import ctypes as C

    from mpc_amd import engine
    protos = _protos(NEW)
    assert sorted(protos) == sorted(NEW)
    L = engine.lib()
    for name, kinds in protos.items():
        fn = getattr(L, name)
        assert len(fn.argtypes) == len(kinds), name
        for k, (t, kind) in enumerate(zip(fn.argtypes, kinds)):
            is_ptr = t is C.c_void_p or t is C.c_char_p or hasattr(t, "contents")
            assert is_ptr == (kind == "ptr"), "%s argument %d" % (name, k + 1)
    assert engine.GC_E_BUSY == -10 and "window" in L.gc_strerror(engine.GC_E_BUSY).decode()
    header = open(os.path.join(ROOT, "include", "gcengine.h")).read()
    assert re.search(r"GC_E_BUSY\s*=\s*-10\b", header) and re.search(r"#define GC_ABI_VERSION 2\b", header)
    hpp = open(os.path.join(ROOT, "include", "mpc_host.hpp")).read()
    go = open(os.path.join(ROOT, "go", "circuit", "stream_batch_hip.go")).read()
    for name in NEW:
        assert name + "(" in hpp, "include/mpc_host.hpp does not call %s" % name
        assert "C." + name + "(" in go, "go/circuit/stream_batch_hip.go does not call %s" % name
    for method in ("select_labels", "decode", "out"):
        assert hasattr(engine.StreamBatch, method)
    for method in ("circuit_host", "uploads_wait", "bad"):
        assert hasattr(engine.StreamEvalBatch, method)
