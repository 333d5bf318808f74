"""CPU check of the fixed-base window tables of the Chou-Orlandi receiver (mpc_amd/csrc/co_table.h): the header is compiled
into a small C++ program with the host compiler, as tests/test_p256_host.py does with p256.h, and every result is compared
with Python integers (tests/py_co_reference.py).

  * every entry of a table is d * 2^(w * i) * P, for G at the widths the library can be built with and for a seeded A at the
    session width;
  * pt_mul_tab equals the restatement's scalar multiplication on the edge scalars of the header's argument (every power of
    the window base, the values just below, N minus them, alternating all-ones / all-zero windows, 0, 1, N - 1 and the
    scalars at and above N whose raw digits would be wrong) and on 200 random ones;
  * a counter that only this host build has shows that no plain addition met equal x coordinates with both operands finite:
    the argument for pt_madd<false> in the header, observed."""
import os
import random
import subprocess

import pytest

from tests import py_co_reference as co

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpc_amd", "csrc")
P, N, G = co.P, co.N, co.G
TOP = 1 << 256
WIDTHS = (4, 5, 8)  # the session width, one that does not divide 256, the generator's width

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define GC_CO_TABLE_COUNT 1
#define GC_CO_TABLE_BUILD 1
#include "co_table.h"

using namespace gc;

static Fe hex32(const std::string &s) {
    uint8_t b[32] = {0};
    for (int i = 0; i < 32 && 2 * i + 1 < (int)s.size(); i++) {
        unsigned v = 0;
        std::sscanf(s.c_str() + 2 * i, "%2x", &v);
        b[i] = (uint8_t)v;
    }
    Fe f;
    vole_load_be(b, f.v);
    return f;
}
static void put(const Fe &f) {
    uint8_t b[32];
    vole_store_be(f.v, b);
    for (int i = 0; i < 32; i++) std::printf("%02x", b[i]);
}
static CoTabEntry copy_entry(const CoTabEntry *e) { return *e; }

template <int W>
static void run(const Aff &base, const std::vector<std::string> &scalars) {
    static_assert(sizeof(CoTabEntry) == 64 && alignof(CoTabEntry) == 16, "an entry is four 16-byte loads");
    std::vector<CoTabEntry> tab(co_tab_entries(W));
    co_tab_build<W>(base, tab.data());
    std::printf("%d %d\n", co_tab_windows(W), co_tab_digits(W));
    for (const CoTabEntry &e : tab) {
        Fe x, y;
        for (int j = 0; j < 8; j++) {
            x.v[j] = e.x[j];
            y.v[j] = e.y[j];
        }
        put(fe_from_mont(x));
        std::printf(" ");
        put(fe_from_mont(y));
        std::printf("\n");
    }
    co_tab_exceptional() = 0;
    for (const std::string &k : scalars) {
        const Jac p = pt_mul_tab<W>(hex32(k), tab.data(), copy_entry);
        Fe x, y;
        pt_to_affine(p, fe_inv(p.z), x, y);
        put(x);
        std::printf(" ");
        put(y);
        std::printf("\n");
    }
    std::printf("%llu\n", co_tab_exceptional());
}

// argv: width, x, y of the base (plain hex); the scalars on stdin, one per line
int main(int argc, char **argv) {
    if (argc != 4) return 2;
    Aff base;
    if (!pt_on_curve(hex32(argv[2]), hex32(argv[3]), base)) return 3;
    std::vector<std::string> scalars;
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        line[std::strcspn(line, "\n")] = 0;
        if (line[0]) scalars.push_back(line);
    }
    const int w = std::atoi(argv[1]);
    if (w == 4) run<4>(base, scalars);
    else if (w == 5) run<5>(base, scalars);
    else if (w == 8) run<8>(base, scalars);
    else return 4;
    return 0;
}
"""


def h(v):
    return "%064x" % v


def hp(pt):
    return "%s %s" % (h(pt[0]), h(pt[1]))


def edge_scalars():
    ks = [0, 1, N - 1, N, N + 1, TOP - 1]
    for j in range(64):
        ks += [1 << (4 * j), (1 << (4 * j)) - 1, N - (1 << (4 * j))]
    ks += [int("0f" * 32, 16), int("f0" * 32, 16)]
    r = random.Random("co_table/scalars")
    ks += [r.randrange(N, TOP) for _ in range(12)]  # (a uniform 256-bit value is at or above N once in 2^32)
    return ks + [r.getrandbits(256) for _ in range(200)]


SCALARS = edge_scalars()
BASES = {"G": G, "A": co.mul(G, int.from_bytes(random.Random("co_table/a").randbytes(32), "big") % N)}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("co_table_host")
    src, out = d / "co_table_check.cpp", d / "co_table_check"
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


@pytest.fixture(scope="module")
def products():
    """k * P of the restatement for every scalar of the list, once per base"""
    return {name: [co.mul(base, k) for k in SCALARS] for name, base in BASES.items()}


def expected_table(base, w):
    windows, digits = -(-256 // w), (1 << w) - 1
    out, b = [], base
    for _ in range(windows):
        e = b
        for _ in range(digits):
            out.append(e)
            e = co.add(e, b)
        b = e  # 2^w * b
    return windows, digits, out


@pytest.mark.parametrize("name,w", [("G", w) for w in WIDTHS] + [("A", 4)])
def test_table_entries_and_windowed_product(exe, products, name, w):
    base = BASES[name]
    r = subprocess.run([exe, str(w), h(base[0]), h(base[1])], input="".join(h(k) + "\n" for k in SCALARS), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    windows, digits, table = expected_table(base, w)
    assert table[digits] == co.mul(base, 1 << w) and table[-1] == co.mul(base, digits << (w * (windows - 1)))
    assert co.INF not in table
    assert lines[0] == "%d %d" % (windows, digits)
    n = windows * digits
    if w == 4:
        assert n * 64 == 61440
    assert len(lines) == 1 + n + len(SCALARS) + 1
    got = lines[1:1 + n]
    bad = [i for i in range(n) if got[i] != hp(table[i])]
    assert not bad, "entry (window %d, digit %d) is not d * 2^(w * i) * P" % (bad[0] // digits, bad[0] % digits + 1)
    got = lines[1 + n:1 + n + len(SCALARS)]
    bad = [h(k) for k, g, want in zip(SCALARS, got, products[name]) if g != hp(want)]
    assert not bad, "pt_mul_tab differs at %d scalars, the first %s" % (len(bad), bad[0])
    assert lines[-1] == "0", "%s plain additions met h = 0 with both operands finite" % lines[-1]


def test_the_scalar_list_holds_the_cases_that_break_unreduced_digits():
    assert {N, N + 1, TOP - 1} <= set(SCALARS) and sum(1 for k in SCALARS if k >= N) >= 15
    assert co.mul(G, N) == co.INF and co.mul(G, N + 1) == G
