"""CPU check of the device-side build of the per-session window tables of the multi-session Chou-Orlandi receiver
(mpc_amd/csrc/co_multi_table.h: co_multi_tab_bases and co_multi_tab_rows_lane, the lane bodies of k_co_multi_tab_bases and
k_co_multi_tab_rows with their index arithmetic).  The header is compiled into a small stand-alone C++ program with the host
compiler, as tests/test_co_multi_host.py does with co_multi.h, and the two bodies run for every lane of 3 sessions (G itself
and two seeded points, so that the s * 960 offsets matter) as the launches do: all sessions through the bases body, then the
rows body per chunk of 2 sessions, over a grid rounded up to whole workgroups, with a workspace that holds ONE chunk.  Every
array is a vector of exactly the size the library allocates.

  * each session's 61 440 bytes are memcmp-equal to co_tab_build<4> of that point, the host builder the one-session handle
    uses;
  * the entries are d * 2^(4i) * P of the restatement (tests/py_co_reference.py), by Python additions;
  * a point that is not on the curve is reported bad and nothing is written for it, by either body;
  * the same program built with -fsanitize=address,undefined exits 0: the index arithmetic, before a device sees it.  The
    binary stands alone; nothing sanitized is loaded into python."""
import os
import random
import subprocess

import pytest

from tests import py_co_reference as co
from tests.test_co_table_host import expected_table

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpc_amd", "csrc")
G, N, P = co.G, co.N, co.P

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <vector>

#define GC_CO_TABLE_BUILD 1
#include "co_multi_table.h"

using namespace gc;

constexpr int kWidth = 4;         // kCoTabWidthA of kernels.h (which needs HIP types and is not included here)
constexpr size_t kChunk = 2;      // sessions per rows launch: 3 sessions make a full chunk and a ragged one
constexpr size_t kThreads = 256;  // lanes of a workgroup: the grid of a launch is rounded up to it
constexpr size_t kWindows = co_tab_windows(kWidth), kEntries = co_tab_entries(kWidth);

static Fe hex32(const char *s) {
    uint8_t b[32] = {0};
    for (int i = 0; i < 32; i++) {
        unsigned v = 0;
        std::sscanf(s + 2 * i, "%2x", &v);
        b[i] = (uint8_t)v;
    }
    Fe f;
    vole_load_be(b, f.v);
    return f;
}
static void put(const uint32_t *mont) {
    Fe f;
    for (int j = 0; j < kVoleLimbs; j++) f.v[j] = mont[j];
    const Fe plain = fe_from_mont(f);
    uint8_t b[32];
    vole_store_be(plain.v, b);
    for (int i = 0; i < 32; i++) std::printf("%02x", b[i]);
}
struct HostMem {
    Fe ld(const uint32_t *p) const {
        Fe f;
        for (int j = 0; j < kVoleLimbs; j++) f.v[j] = p[j];
        return f;
    }
    void st(uint32_t *p, const Fe &f) const {
        for (int j = 0; j < kVoleLimbs; j++) p[j] = f.v[j];
    }
};

// the build as co_engine.cpp launches it.  x, y: plain coordinates of the S points
static void build(const std::vector<Fe> &x, const std::vector<Fe> &y, std::vector<uint32_t> &good, std::vector<CoTabEntry> &tabs,
                  std::vector<CoTabBase> &bases, std::vector<CoTabZ> &zs) {
    const size_t S = x.size();
    for (size_t s = 0; s < (S + 63) / 64 * 64; s++) {
        if (s >= S) continue;
        good[s] = co_multi_tab_bases<kWidth>(x[s], y[s], s, bases.data(), HostMem()) ? 1u : 0u;
    }
    for (size_t s0 = 0; s0 < S; s0 += kChunk) {
        const size_t count = S - s0 < kChunk ? S - s0 : kChunk;
        const size_t lanes = (count * kWindows + kThreads - 1) / kThreads * kThreads;
        for (size_t l = 0; l < lanes; l++)
            co_multi_tab_rows_lane<kWidth>(l, s0, count, good.data(), bases.data(), tabs.data(), zs.data(), HostMem());
    }
}

// argv: x y of each session's point (plain hex).  Prints "equal <s> <0|1>" per session, then every entry "x y" (plain hex),
// then "bad <0|1>" for a point off the curve whose arrays stayed untouched
int main(int argc, char **argv) {
    static_assert(sizeof(CoTabEntry) == 64 && sizeof(CoTabBase) == 96 && sizeof(CoTabZ) == 64, "the sizes the library allocates");
    if (argc < 3 || argc % 2 != 1) return 2;
    const size_t S = (size_t)(argc - 1) / 2;
    std::vector<Fe> x(S), y(S);
    for (size_t s = 0; s < S; s++) {
        x[s] = hex32(argv[1 + 2 * s]);
        y[s] = hex32(argv[2 + 2 * s]);
    }
    std::vector<uint32_t> good(S, 7u);
    std::vector<CoTabEntry> tabs(S * kEntries);
    std::vector<CoTabBase> bases(S * kWindows);
    std::vector<CoTabZ> zs((S < kChunk ? S : kChunk) * kEntries);
    build(x, y, good, tabs, bases, zs);
    for (size_t s = 0; s < S; s++) {
        if (good[s] != 1u) return 3;
        Aff a;
        if (!pt_on_curve(x[s], y[s], a)) return 4;
        std::vector<CoTabEntry> want(kEntries);
        co_tab_build<kWidth>(a, want.data());
        std::printf("equal %zu %d\n", s, std::memcmp(want.data(), tabs.data() + s * kEntries, kEntries * sizeof(CoTabEntry)) == 0);
    }
    for (const CoTabEntry &e : tabs) {
        put(e.x);
        std::printf(" ");
        put(e.y);
        std::printf("\n");
    }
    // a bad session: (x, y + 1) of the first point
    std::vector<Fe> bx(1, x[0]), by(1, y[0]);
    by[0].v[0] ^= 1u;
    std::vector<uint32_t> bgood(1, 7u);
    std::vector<CoTabEntry> btabs(kEntries);
    std::vector<CoTabBase> bbases(kWindows);
    std::vector<CoTabZ> bzs(kEntries);
    std::memset(btabs.data(), 0xA5, kEntries * sizeof(CoTabEntry));
    std::memset(bbases.data(), 0xA5, kWindows * sizeof(CoTabBase));
    std::memset(bzs.data(), 0xA5, kEntries * sizeof(CoTabZ));
    build(bx, by, bgood, btabs, bbases, bzs);
    bool untouched = bgood[0] == 0u;
    const uint8_t *p[3] = {(const uint8_t *)btabs.data(), (const uint8_t *)bbases.data(), (const uint8_t *)bzs.data()};
    const size_t n[3] = {kEntries * sizeof(CoTabEntry), kWindows * sizeof(CoTabBase), kEntries * sizeof(CoTabZ)};
    for (int k = 0; k < 3; k++)
        for (size_t i = 0; i < n[k]; i++) untouched = untouched && p[k][i] == 0xA5;
    std::printf("bad %d\n", untouched ? 1 : 0);
    return 0;
}
"""


def h(v):
    return "%064x" % v


def seeded(tag):
    return co.mul(G, int.from_bytes(random.Random("co_multi_table/" + tag).randbytes(32), "big") % N)


POINTS = [G, seeded("a1"), seeded("a2")]
ARGS = [h(c) for pt in POINTS for c in pt]


def compile_program(d, name, flags):
    src, out = d / (name + ".cpp"), d / name
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, str(src), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = compile_program(tmp_path_factory.mktemp("co_multi_table_host"), "co_multi_table_check", ["-O2"])
    r = subprocess.run([exe] + ARGS, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr)
    got = r.stdout.splitlines()
    assert len(got) == len(POINTS) + len(POINTS) * 960 + 1
    return got


def test_the_constants_are_the_library_s():
    from tests.util import kernel_constants
    assert kernel_constants("kCoTabWidthA") == 4
    assert kernel_constants("kCoMultiTabRowThreads") == 256 and kernel_constants("kCoMultiTabBaseThreads") == 64


def test_each_session_equals_the_host_builder(lines):
    assert len(set(POINTS)) == 3 and all(co.valid_point(p) for p in POINTS)
    assert lines[:len(POINTS)] == ["equal %d 1" % s for s in range(len(POINTS))]


def test_entries_equal_the_restatement(lines):
    for s, pt in enumerate(POINTS):
        windows, digits, table = expected_table(pt, 4)
        assert (windows, digits) == (64, 15) and len(table) * 64 == 61440
        got = lines[len(POINTS) + s * 960:len(POINTS) + (s + 1) * 960]
        bad = [i for i in range(960) if got[i] != "%s %s" % (h(table[i][0]), h(table[i][1]))]
        assert not bad, "session %d: entry (window %d, digit %d) is not d * 2^(4i) * P" % (s, bad[0] // 15, bad[0] % 15 + 1)


def test_a_bad_session_writes_nothing(lines):
    assert not co.valid_point((G[0], G[1] ^ 1))
    assert lines[-1] == "bad 1"


def test_sanitized_build_exits_clean(tmp_path, lines):
    exe = compile_program(tmp_path, "co_multi_table_check_san",
                          ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([exe] + ARGS, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    assert r.stdout.splitlines() == lines
