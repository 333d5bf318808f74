"""CPU check of the sender's per-session setup of the multi-session Chou-Orlandi calls (mpc_amd/csrc/co_multi.h:
co_multi_setup_session, the routine k_co_multi_setup runs with one lane per session).  The header is compiled into a small
C++ program with the host compiler, with a host-built table of G as tests/test_co_table_host.py has it, and A and AaInv are
compared with the restatement's sender_setup (tests/py_co_reference.py):

  * A = a * G and AaInv = -(a^2 mod N) * G for the scalars where the square wraps or meets its edges (1, 2, N - 1 whose
    square is 1, N + 1, 2^256 - 1, 2^255) and for 40 seeded ones;
  * the counter that only a host build has shows that no plain addition of the two table walks met equal x coordinates
    with both operands finite: the digits of a^2 mod N are those of a value below N, as co_table.h asks;
  * a = 0 and a = N report a bad session, with zero outputs."""
import os
import subprocess

import pytest

from tests import py_co_reference as co
from tests.util import drbg

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpc_amd", "csrc")
N = co.N
TOP = 1 << 256

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define GC_CO_TABLE_COUNT 1
#define GC_CO_TABLE_BUILD 1
#include "co_multi.h"

using namespace gc;

constexpr int kWidth = 8;  // kCoTabWidthG of kernels.h (which needs HIP types and is not included here)

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
static void put(const Fe &f) {
    uint8_t b[32];
    vole_store_be(f.v, b);
    for (int i = 0; i < 32; i++) std::printf("%02x", b[i]);
}
static CoTabEntry copy_entry(const CoTabEntry *e) { return *e; }

// the scalars on stdin, one per line: "<good> Ax Ay AaInvx AaInvy" each, then the count of exceptional plain additions
int main() {
    Aff g;
    g.x = fe_to_mont(p256_gx());
    g.y = fe_to_mont(p256_gy());
    g.inf = 0;
    std::vector<CoTabEntry> tab(co_tab_entries(kWidth));
    co_tab_build<kWidth>(g, tab.data());
    uint8_t n_be[32];
    vole_store_be(p256_n().v, n_be);
    VoleMod modn;
    if (!vole_mod_init(n_be, &modn)) return 3;
    co_tab_exceptional() = 0;
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        if (std::strlen(line) < 64) continue;
        Fe ax, ay, tx, ty;
        const bool good = co_multi_setup_session<kWidth>(hex32(line), modn, tab.data(), copy_entry, ax, ay, tx, ty);
        std::printf("%d ", good ? 1 : 0);
        put(ax);
        std::printf(" ");
        put(ay);
        std::printf(" ");
        put(tx);
        std::printf(" ");
        put(ty);
        std::printf("\n");
    }
    std::printf("%llu\n", co_tab_exceptional());
    return 0;
}
"""

GOOD = [1, 2, N - 1, N + 1, TOP - 1, 1 << 255] + [int.from_bytes(drbg("co_multi/host/a%d" % i, 32), "big") for i in range(40)]
BAD = [0, N]


def h(v):
    return "%064x" % v


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("co_multi_host")
    src, out = d / "co_multi_check.cpp", d / "co_multi_check"
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(out)], input="".join(h(a) + "\n" for a in GOOD + BAD), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    got = r.stdout.splitlines()
    assert len(got) == len(GOOD) + len(BAD) + 1
    return got


def test_the_table_width_is_the_library_s():
    from tests.util import kernel_constants
    assert kernel_constants("kCoTabWidthG") == 8


def test_setup_equals_the_restatement(lines):
    assert all(a % N for a in GOOD) and pow(N - 1, 2, N) == 1 and any(a >= N for a in GOOD)
    for a, line in zip(GOOD, lines):
        A, AaInv = co.sender_setup(a)
        assert AaInv == co.neg(co.mul(co.G, a * a % N))
        assert line == "1 %s %s %s %s" % (h(A[0]), h(A[1]), h(AaInv[0]), h(AaInv[1])), "a = %s" % h(a)


def test_no_exceptional_plain_addition(lines):
    assert lines[-1] == "0", "%s plain additions met h = 0 with both operands finite" % lines[-1]


def test_zero_scalars_are_bad_sessions(lines):
    for a, line in zip(BAD, lines[len(GOOD):]):
        assert a % N == 0
        assert line == "0 " + " ".join([h(0)] * 4), "a = %s" % h(a)
