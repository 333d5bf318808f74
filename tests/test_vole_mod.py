"""CPU check of the VOLE kernels' 256-bit arithmetic (mpc_amd/csrc/vole_mod.h): the header is compiled into a small C++
program with the host compiler, and every constant, reduction, product and sum it computes is compared with Python
integers — for odd moduli from 3 to 2^256 - 1, tiny and composite ones included, 2 000 seeded values each plus the edges
(0, 1, p - 1, p, p + 1, 2^256 - 1, all-0xff / all-0x00 byte patterns) — and the moduli the ABI refuses are refused."""
import os
import random
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpc_amd", "csrc")
TOP = 1 << 256

PROGRAM = r"""
#include <cstdio>
#include <cstring>

#include "vole_mod.h"

using namespace gc;

static bool hex32(const char *s, uint8_t *b) {
    if (std::strlen(s) != 64) return false;
    for (int i = 0; i < 32; i++) {
        unsigned v;
        if (std::sscanf(s + 2 * i, "%2x", &v) != 1) return false;
        b[i] = (uint8_t)v;
    }
    return true;
}

static void put(const uint32_t (&v)[kVoleLimbs]) {
    uint8_t b[32];
    vole_store_be(v, b);
    for (int i = 0; i < 32; i++) std::printf("%02x", b[i]);
}

// one case per line: OP P A B (hex, 64 digits; '-' for an unused operand) -> one line of results
//   C: constants of P ("refused" or "n0 r2")     R: A mod P        M: A * B mod P        T: A * B * 2^-256 mod P (B < P)
//   A: (A + B) mod P (A, B < P)                  W: A through the word form: load words, limbs, store words
int main() {
    char op[4], ps[80], as[80], bs[80];
    while (std::scanf("%3s %79s %79s %79s", op, ps, as, bs) == 4) {
        uint8_t pb[32], ab[32], bb[32];
        hex32(ps, pb);
        const bool ha = hex32(as, ab), hb = hex32(bs, bb);
        VoleMod m;
        const bool ok = vole_mod_init(pb, &m);
        if (op[0] == 'C') {
            if (!ok) {
                std::printf("refused\n");
                continue;
            }
            std::printf("%08x ", m.n0);
            put(m.r2);
            std::printf("\n");
            continue;
        }
        uint32_t a[kVoleLimbs], b[kVoleLimbs], out[kVoleLimbs];
        if (ha) vole_load_be(ab, a);
        if (hb) vole_load_be(bb, b);
        if (!ok || !ha) {
            std::printf("bad\n");
            continue;
        }
        if (op[0] == 'R') {
            vole_reduce(a, m, out);
        } else if (op[0] == 'M' && hb) {
            vole_mul_mod(a, b, m, out);
        } else if (op[0] == 'T' && hb) {
            vole_mont_mul(a, b, m, out);
        } else if (op[0] == 'A' && hb) {
            vole_add_mod(a, b, m, out);
            vole_add_mod(a, b, m, a);  // out aliasing an input
            for (int j = 0; j < kVoleLimbs; j++)
                if (a[j] != out[j]) out[0] ^= 1;
        } else if (op[0] == 'W') {
            uint32_t w[kVoleLimbs], v[kVoleLimbs];
            std::memcpy(w, ab, 32);  // a little-endian load of the 32 bytes (the kernels' uint4 loads)
            vole_from_be_words(w, v);
            for (int j = 0; j < kVoleLimbs; j++)
                if (v[j] != a[j]) v[0] ^= 1;
            vole_to_be_words(v, w);
            uint8_t back[32];
            std::memcpy(back, w, 32);
            vole_load_be(back, out);
        } else {
            std::printf("bad\n");
            continue;
        }
        put(out);
        std::printf("\n");
    }
    return 0;
}
"""

SECP256K1 = (1 << 256) - (1 << 32) - 977
P256 = int("ffffffff00000001000000000000000000000000ffffffffffffffffffffffff", 16)


def _random_odd(bits, seed):
    r = random.Random(seed)
    return r.getrandbits(bits) | (1 << (bits - 1)) | 1


MODULI = [3, 5, 65537, (1 << 61) - 1, (1 << 127) - 1, (1 << 128) + 1, (1 << 255) - 19, SECP256K1, P256, (1 << 256) - 189,
          (1 << 256) - 1, _random_odd(200, "vole/p200"), _random_odd(256, "vole/p256")]
REFUSED = [0, 1, 2, 4, 1 << 255]


def h(v):
    return "%064x" % v


def byte_patterns():
    """all-0xff / all-0x00 byte patterns: every 32-byte value made of whole 0x00 / 0xff bytes in runs"""
    out = set()
    for run in (1, 2, 4, 8, 16):
        for phase in (0, 1):
            b = bytes((0xff if ((i // run) + phase) % 2 else 0) for i in range(32))
            out.add(int.from_bytes(b, "big"))
    for k in range(33):  # top k bytes 0xff, the rest 0x00, and the reverse
        out.add(int.from_bytes(b"\xff" * k + b"\x00" * (32 - k), "big"))
        out.add(int.from_bytes(b"\x00" * k + b"\xff" * (32 - k), "big"))
    return sorted(out)


def edges(p):
    e = {0, 1, 2, p - 1, p, p + 1, 2 * p - 1, 2 * p, TOP - 1, TOP - p, TOP - p - 1, (TOP - 1) - (TOP - 1) % p}
    e |= set(byte_patterns())
    return sorted(v for v in e if 0 <= v < TOP)


def values(p, n, seed):
    """n seeded values below 2^256: uniform, below p, and near multiples of p"""
    r = random.Random("%s/%d" % (seed, p))
    out = []
    for i in range(n):
        k = i % 4
        if k == 0:
            out.append(r.getrandbits(256))
        elif k == 1:
            out.append(r.randrange(p))
        elif k == 2:
            out.append(r.getrandbits(r.randrange(1, 257)))
        else:
            q = r.randrange(TOP // p) if TOP // p > 0 else 0
            out.append(min(TOP - 1, max(0, q * p + r.randrange(-2, 3))))
    return out


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("vole_mod")
    src, exe = d / "vole_mod_check.cpp", d / "vole_mod_check"
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def go(cases):
        text = "".join("%s %s %s %s\n" % c for c in cases)
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        return lines

    return go


def test_constants(run):
    lines = run([("C", h(p), "-", "-") for p in MODULI])
    for p, line in zip(MODULI, lines):
        n0, r2 = line.split()
        assert int(n0, 16) == (-pow(p, -1, 1 << 32)) % (1 << 32), p
        assert int(r2, 16) == pow(2, 512, p), p


def test_refused_moduli(run):
    lines = run([("C", h(p), "-", "-") for p in REFUSED] + [("R", h(p), h(5), "-") for p in REFUSED])
    assert all(l == "refused" for l in lines[: len(REFUSED)]), lines
    assert all(l == "bad" for l in lines[len(REFUSED):]), lines


@pytest.mark.parametrize("p", MODULI, ids=lambda p: "%d_bits" % p.bit_length())
def test_reduce_mul_add(run, p):
    vs = edges(p) + values(p, 2000, "vole/v")
    ws = values(p, len(vs), "vole/w")
    below = [v % p for v in vs]
    below_w = [w % p for w in ws]
    cases, want = [], []
    for v in vs:  # reductions of any 256-bit value
        cases.append(("R", h(p), h(v), "-"))
        want.append(v % p)
    for v, w in zip(vs, ws):  # products of any two 256-bit values
        cases.append(("M", h(p), h(v), h(w)))
        want.append(v * w % p)
    for v, w in zip(vs, below_w):  # Montgomery products, the second factor below p
        cases.append(("T", h(p), h(v), h(w)))
        want.append(v * w * pow(TOP, -1, p) % p)
    for a, b in zip(below, below_w + below_w[::-1]):  # modular sums of values below p
        cases.append(("A", h(p), h(a), h(b)))
        want.append((a + b) % p)
    for e in edges(p):  # edges against edges
        for f in (0, 1, p - 1, TOP - 1):
            cases.append(("M", h(p), h(e), h(f % TOP)))
            want.append(e * f % p)
        cases.append(("A", h(p), h(e % p), h((p - 1) % p)))
        want.append((e % p + p - 1) % p)
    lines = run(cases)
    bad = [(c, l, h(w)) for c, l, w in zip(cases, lines, want) if l != h(w)]
    assert not bad, "%d of %d differ, first: %s" % (len(bad), len(cases), bad[:3])


def test_big_endian_load_store(run):
    vs = byte_patterns() + values(P256, 500, "vole/be")
    lines = run([("W", h(P256), h(v), "-") for v in vs])
    assert lines == [h(v) for v in vs]
