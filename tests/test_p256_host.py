"""CPU check of the Chou-Orlandi kernels' arithmetic (mpc_amd/csrc/p256.h, co_sha256.h): both headers are compiled into a
small C++ program with the host compiler — they are plain C++, as vole_mod.h — and every result is compared with Python
integers (the P-256 of tests/go_transcript.py, which the Go tests' round hashes pin) and with hashlib."""
import hashlib
import os
import random
import subprocess

import pytest

from tests import py_co_reference as co

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpc_amd", "csrc")
P, N, G = co.P, co.N, co.G
TOP = 1 << 256

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "co_sha256.h"

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
// a point given as plain x, y (0, 0: infinity) -> Montgomery affine
static Aff aff(const Fe &x, const Fe &y) {
    Aff q;
    q.x = fe_to_mont(x);
    q.y = fe_to_mont(y);
    q.inf = fe_is_zero(x) && fe_is_zero(y);
    return q;
}
// the same point as (x z^2, y z^3, z) for a plain z != 0
static Jac jac(const Aff &q, const Fe &z) {
    if (q.inf) return pt_infinity();
    const Fe zm = fe_to_mont(z), z2 = fe_sqr(zm);
    return Jac{fe_mul(q.x, z2), fe_mul(q.y, fe_mul(z2, zm)), zm};
}
static void put_point(const Jac &p) {
    Fe x, y;
    pt_to_affine(p, fe_inv(p.z), x, y);
    put(x);
    std::printf(" ");
    put(y);
}

int main() {
    char line[1024];
    while (std::fgets(line, sizeof line, stdin)) {
        std::vector<std::string> a;
        for (char *t = std::strtok(line, " \n"); t; t = std::strtok(nullptr, " \n")) a.push_back(t);
        if (a.empty()) continue;
        const std::string &op = a[0];
        if (op == "const") {  // the constants of p against vole_mod_init, and 1 in Montgomery form
            uint8_t pb[32];
            const VoleMod f = p256_field();
            Fe p;
            for (int j = 0; j < 8; j++) p.v[j] = f.p[j];
            vole_store_be(p.v, pb);
            VoleMod m;
            bool ok = vole_mod_init(pb, &m) && m.n0 == f.n0;
            for (int j = 0; j < 8; j++) ok = ok && m.p[j] == f.p[j] && m.r2[j] == f.r2[j];
            ok = ok && fe_eq(fe_to_mont(fe_plain_one()), fe_one());
            put(p);
            std::printf(" %d\n", ok ? 1 : 0);
        } else if (op == "mul") {
            put(fe_from_mont(fe_mul(fe_to_mont(hex32(a[1])), fe_to_mont(hex32(a[2])))));
            std::printf("\n");
        } else if (op == "sqr") {
            put(fe_from_mont(fe_sqr(fe_to_mont(hex32(a[1])))));
            std::printf("\n");
        } else if (op == "inv") {
            put(fe_from_mont(fe_inv(fe_to_mont(hex32(a[1])))));
            std::printf("\n");
        } else if (op == "sub") {
            put(fe_sub(hex32(a[1]), hex32(a[2])));
            std::printf("\n");
        } else if (op == "dbl") {  // x y z
            put_point(pt_dbl(jac(aff(hex32(a[1]), hex32(a[2])), hex32(a[3]))));
            std::printf("\n");
        } else if (op == "madd" || op == "cadd") {  // x1 y1 z1 x2 y2
            const Jac p = jac(aff(hex32(a[1]), hex32(a[2])), hex32(a[3]));
            const Aff q = aff(hex32(a[4]), hex32(a[5]));
            put_point(op == "cadd" ? pt_madd<true>(p, q) : pt_madd<false>(p, q));
            std::printf("\n");
        } else if (op == "smul") {  // k x y
            put_point(pt_mul(sc_reduce(hex32(a[1])), aff(hex32(a[2]), hex32(a[3]))));
            std::printf("\n");
        } else if (op == "red") {
            put(sc_reduce(hex32(a[1])));
            std::printf("\n");
        } else if (op == "curve") {  // x y
            Aff q;
            std::printf("%d\n", pt_on_curve(hex32(a[1]), hex32(a[2]), q) ? 1 : 0);
        } else if (op == "sha") {  // len, the message as 144 hex digits (zero beyond len)
            const unsigned len = (unsigned)std::atoi(a[1].c_str());
            uint32_t m[18], st[8];
            for (int j = 0; j < 18; j++) {
                unsigned v = 0;
                std::sscanf(a[2].c_str() + 8 * j, "%8x", &v);
                m[j] = v;
            }
            co_sha256_short(m, len, st);
            for (int j = 0; j < 8; j++) std::printf("%08x", st[j]);
            std::printf("\n");
        } else if (op == "mask") {  // x y id(16 hex digits)
            uint32_t out[4];
            co_derive_mask(hex32(a[1]), hex32(a[2]), std::stoull(a[3], nullptr, 16), out);
            for (int j = 0; j < 4; j++) std::printf("%08x", out[j]);
            std::printf("\n");
        } else {
            std::printf("bad\n");
        }
    }
    return 0;
}
"""


def h(v):
    return "%064x" % v


def hp(pt):
    return "%s %s" % (h(pt[0]), h(pt[1]))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("p256_host")
    src, exe = d / "p256_check.cpp", d / "p256_check"
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def go(cases):
        r = subprocess.run([str(exe)], input="".join(c + "\n" for c in cases), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        return lines

    return go


def field_values():
    r = random.Random("p256/field")
    return [0, 1, 2, P - 1, P - 2, (P + 1) // 2, 1 << 255, (1 << 224) - 1, 1 << 96] + [r.randrange(P) for _ in range(300)]


def test_constants(run):
    assert run(["const"]) == ["%s 1" % h(P)]


def test_field_multiply_square_invert_subtract(run):
    vs = field_values()
    ws = vs[::-1]
    cases, want = [], []
    for v, w in list(zip(vs, ws)) + [(e, f) for e in (0, 1, P - 1) for f in (0, 1, P - 1)]:
        cases.append("mul %s %s" % (h(v), h(w)))
        want.append(v * w % P)
        cases.append("sub %s %s" % (h(v), h(w)))
        want.append((v - w) % P)
    for v in vs:
        cases.append("sqr %s" % h(v))
        want.append(v * v % P)
        cases.append("inv %s" % h(v))
        want.append(pow(v, P - 2, P))  # 0 -> 0
    assert run(cases) == [h(w) for w in want]
    assert pow(P - 1, P - 2, P) == P - 1 and pow(1, P - 2, P) == 1


def some_points(n, seed):
    r = random.Random(seed)
    return [co.mul(G, r.randrange(1, N)) for _ in range(n)]


def test_doubling_and_additions(run):
    r = random.Random("p256/z")
    pts = some_points(6, "p256/points")
    cases, want = [], []
    for p in pts:
        z = r.randrange(1, P)
        for zz in (1, z):
            cases.append("dbl %s %s" % (hp(p), h(zz)))
            want.append(co.add(p, p))
            for q in pts:
                if q == p or q == co.neg(p):
                    continue
                cases.append("madd %s %s %s" % (hp(p), h(zz), hp(q)))  # the ladder's addition: distinct points
                want.append(co.add(p, q))
            # the complete addition: P + P, P + (-P), P + inf, inf + P, P + Q; the plain one agrees except on P + P
            for q in [p, co.neg(p), co.INF, pts[0]]:
                cases.append("cadd %s %s %s" % (hp(p), h(zz), hp(q)))
                want.append(co.add(p, q))
            for name in ("madd", "cadd"):
                cases.append("%s %s %s %s" % (name, hp(co.INF), h(zz), hp(p)))
                want.append(p)
                cases.append("%s %s %s %s" % (name, hp(p), h(zz), hp(co.neg(p))))
                want.append(co.INF)
                cases.append("%s %s %s %s" % (name, hp(p), h(zz), hp(co.INF)))
                want.append(p)
    cases += ["dbl %s %s" % (hp(co.INF), h(1)), "cadd %s %s %s" % (hp(co.INF), h(1), hp(co.INF))]
    want += [co.INF, co.INF]
    assert run(cases) == [hp(w) for w in want]


SCALARS = [0, 1, 2, N - 1, N, N + 1, TOP - 1, co.SHORT_A_SCALAR]


def test_scalar_multiplication(run):
    r = random.Random("p256/scalars")
    ks = SCALARS + [r.getrandbits(256) for _ in range(12)] + [r.getrandbits(r.randrange(1, 200)) for _ in range(4)]
    bases = [G] + some_points(1, "p256/base")
    cases = ["smul %s %s" % (h(k), hp(b)) for b in bases for k in ks]
    cases += ["smul %s %s" % (h(k), hp(co.INF)) for k in (0, 5)]
    want = [co.mul(b, k) for b in bases for k in ks] + [co.INF, co.INF]
    assert run(cases) == [hp(w) for w in want]
    assert run(["red %s" % h(k) for k in ks]) == [h(k % N) for k in ks]


def test_on_curve_check(run):
    pts = some_points(3, "p256/curve")
    sb = co.SQRT_B
    cases = [(p, True) for p in pts] + [((p[0], (p[1] + 1) % P), False) for p in pts] + [
        ((0, sb), True), ((0, P - sb), True), ((P, sb), False), ((0, sb + P), False) if sb + P < TOP else ((0, 1), False),
        (co.INF, False), ((G[0] + P, G[1]), False) if G[0] + P < TOP else ((1, 1), False), ((TOP - 1, TOP - 1), False), (G, True)]
    for p, ok in cases:
        assert co.valid_point(p) == ok, p
    assert run(["curve %s" % hp(p) for p, _ in cases]) == ["1" if ok else "0" for _, ok in cases]


def test_sha256_at_every_length(run):
    r = random.Random("p256/sha")
    cases, want = [], []
    for n in range(8, 73):
        for msg in (bytes(r.getrandbits(8) for _ in range(n)), b"\xff" * n, bytes(n)):
            cases.append("sha %d %s" % (n, (msg + bytes(72 - n)).hex()))
            want.append(hashlib.sha256(msg).hexdigest())
    assert run(cases) == want


def test_derive_mask_strips_leading_zero_bytes(run):
    r = random.Random("p256/mask")
    cases, want = [], []
    for lx in list(range(0, 33)):
        for ly in (0, 1, 29, 30, 31, 32, r.randrange(33)):
            x = (r.getrandbits(8 * lx) | (1 << (8 * lx - 1))) if lx else 0
            y = (r.getrandbits(8 * ly) | (1 << (8 * ly - 8))) if ly else 0
            assert co.coord_lengths((x, y)) == (lx, ly)
            idx = r.choice([0, 1, (1 << 32) + 5, (1 << 64) - 1, r.getrandbits(64)])
            cases.append("mask %s %s %016x" % (h(x), h(y), idx))
            want.append(co.mask((x, y), idx).hex())
    assert run(cases) == want
