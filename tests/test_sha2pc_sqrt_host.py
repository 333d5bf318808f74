"""CPU check of the square root mod p and the point decompression of the sha2pc Round 2 decode
(mpc_amd/csrc/p256_sqrt.h): the header is plain C++ on p256.h, compiled here into a stand-alone program with the host
compiler under AddressSanitizer and UBSan, run directly, and compared with Python integers: y = pow(t, (p + 1) // 4, p),
accepted when y * y = t."""
import os
import random
import subprocess

import pytest

from tests import go_transcript as gt

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpc_amd", "csrc")
P, B, G = gt.P, gt.B, gt.G

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <string>

#include "p256_sqrt.h"

using namespace gc;

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
// lines "X odd" (X: 64 hex digits, any value below 2^256) -> "ok x y | ok root" : the decompression, and fe_sqrt of X itself
// taken mod p (root: the plain value, 0 when X is no square)
int main() {
    char hex[80];
    int odd;
    while (std::scanf("%64s %d", hex, &odd) == 2) {
        const Fe X = hex32(hex);
        Fe x, y;
        const bool ok = pt_decompress(X, odd != 0, x, y);
        std::printf("%d ", ok ? 1 : 0);
        put(x);
        std::printf(" ");
        put(y);
        Fe r;
        const Fe t = fe_to_mont(X);
        const bool sq = fe_sqrt(t, r);
        std::printf(" %d ", sq ? 1 : 0);
        put(sq ? fe_from_mont(r) : fe_zero());
        std::printf("\n");
    }
    return 0;
}
"""


def py_decompress(x, odd):
    if x >= P:
        return None
    t = (x * x * x - 3 * x + B) % P
    y = pow(t, (P + 1) // 4, P)
    if y * y % P != t:
        return None
    return (x, y if (y & 1) == odd else (-y) % P)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("sha2pc_sqrt")
    src, exe = d / "sqrt_check.cpp", d / "sqrt_check"
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(exe)


def run(program, cases):
    text = "".join("%064x %d\n" % c for c in cases)
    r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    return [l.split() for l in lines]


def check(cases, rows):
    for (X, odd), (ok, x, y, sq, root) in zip(cases, rows):
        want = py_decompress(X, odd)
        assert int(ok) == (want is not None), hex(X)
        assert (int(x, 16), int(y, 16)) == (want or (0, 0)), hex(X)
        t = X % P
        r = pow(t, (P + 1) // 4, P)
        is_sq = r * r % P == t
        assert int(sq) == is_sq, hex(X)
        if is_sq:  # the chain gives t^((p + 1) / 4) itself, not its negative
            assert int(root, 16) == r, hex(X)


def test_generator_and_edges(program):
    cases = [(G[0], 0), (G[0], 1), (0, 0), (0, 1), (P - 1, 0), (P - 1, 1), (P, 0), (P, 1), (2 ** 256 - 1, 0), (2 ** 256 - 1, 1),
             (P + 5, 0), (1, 0), (2, 1)]
    rows = run(program, cases)
    check(cases, rows)
    got = {c: r for c, r in zip(cases, rows)}
    assert (int(got[(G[0], G[1] & 1)][2], 16), int(got[(G[0], 1 - (G[1] & 1))][2], 16)) == (G[1], P - G[1])
    for X in (P, 2 ** 256 - 1, P + 5):  # refused, not reduced
        assert got[(X, 0)][:3] == ["0", "0" * 64, "0" * 64]
    assert got[(0, 0)][0] == "1" and got[(P - 1, 0)][0] == ("1" if py_decompress(P - 1, 0) else "0")


def test_seeded_values(program):
    """2 000 seeded x: x^3 - 3x + b is a non-residue for about half of them (1 013 of 2 000 with this seed; the test asks
    for 900 .. 1 100, five standard deviations of a fair coin around 1 000)"""
    rng = random.Random("sha2pc-sqrt")
    cases = [(rng.randrange(P), rng.randrange(2)) for _ in range(2000)]
    non = sum(py_decompress(*c) is None for c in cases)
    print("non-residues: %d of %d" % (non, len(cases)))
    assert 900 <= non <= 1100, non
    check(cases, run(program, cases))
