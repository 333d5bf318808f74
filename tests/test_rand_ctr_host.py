"""CPU check of the arithmetic of the random streams (mpc_amd/csrc/rand_ctr.h), which the engine and the kernels of gc_rand_*
share: the header is compiled into a small stand-alone C++ program with the host compiler and the address and
undefined-behaviour sanitizers, and its answers are held against Python integers: the 128-bit big-endian counter addition
over 2 000 seeded (iv, j) and the carry edges the GPU tests use, and the cover of 2 000 seeded byte ranges (pos, n) by blocks,
with the piece of the range every block of the cover holds (all of them for short ranges, the first two and the last
otherwise)."""
import os
import subprocess

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpc_amd", "csrc")

PROGRAM = r"""
#include <cinttypes>
#include <cstdio>

#include "rand_ctr.h"

using namespace gc;

static void piece(const RandCover &c, uint64_t n, uint64_t k) {
    const RandPiece p = rand_piece(c, n, k);
    std::printf(" %" PRIu64 ":%" PRIu64 ":%u:%u", k, p.at, p.from, p.to);
}

// "A <32 hex digits> <j>" -> the sum as 32 hex digits; "C <pos> <n>" -> ok first nblocks head units, then k:at:from:to
int main() {
    char op;
    while (std::scanf(" %c", &op) == 1) {
        if (op == 'A') {
            char hex[33];
            uint64_t j;
            if (std::scanf("%32s %" SCNu64, hex, &j) != 2) return 1;
            uint8_t iv[16];
            for (int i = 0; i < 16; i++) {
                unsigned v;
                std::sscanf(hex + 2 * i, "%2x", &v);
                iv[i] = (uint8_t)v;
            }
            const RandCtr c = rand_ctr_add(rand_ctr_from_bytes(iv), j);
            std::printf("%016" PRIx64 "%016" PRIx64 "\n", c.hi, c.lo);
        } else {
            uint64_t pos, n;
            if (std::scanf("%" SCNu64 " %" SCNu64, &pos, &n) != 2) return 1;
            if (!rand_range_ok(pos, n)) {
                std::printf("refused\n");
                continue;
            }
            const RandCover c = rand_cover(pos, n);
            const RandPos p = rand_pos_split(pos);
            std::printf("ok %" PRIu64 " %" PRIu64 " %u %" PRIu64 " %" PRIu64 " %u", c.first, c.nblocks, c.head, rand_units(c.nblocks),
                        p.block, p.off);
            if (c.nblocks <= 300) {
                for (uint64_t k = 0; k < c.nblocks; k++) piece(c, n, k);
            } else {
                piece(c, n, 0);
                piece(c, n, 1);
                piece(c, n, c.nblocks - 1);
            }
            std::printf("\n");
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("rand_ctr")
    src, exe = d / "rand_ctr_host.cpp", d / "rand_ctr_host"
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def run(prog, lines):
    r = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
    out = r.stdout.strip().split("\n")
    assert len(out) == len(lines)
    return out


def test_counter_addition(prog):
    rng = np.random.default_rng(2025)
    ff = (1 << 64) - 1
    cases = [(int.from_bytes(rng.bytes(16), "big"), int(rng.integers(0, 1 << 63)) >> int(rng.integers(0, 63)))
             for _ in range(2000)]
    edges = [ff - 1, (1 << 128) - 1, (0x0123456789abcdef << 64) | 0xffffffff, (ff << 64) | (ff - 1), 0]
    for iv in edges:  # the IVs of the GPU test, and what surrounds their carries
        cases += [(iv, j) for j in (0, 1, 2, 3, 4, (1 << 32) + 7, 1 << 60, ff)]
    cases += [(int.from_bytes(rng.bytes(8), "big") << 64 | (ff - int(rng.integers(0, 1000))), int(rng.integers(0, 2000)))
              for _ in range(200)]
    out = run(prog, ["A %032x %d" % c for c in cases])
    for (iv, j), got in zip(cases, out):
        assert int(got, 16) == (iv + j) % (1 << 128), (hex(iv), j)


def want_piece(pos, n, k):
    head = pos % 16
    lo, hi = max(0, 16 * k - head), min(n, 16 * k - head + 16)  # the bytes of the range that block k holds
    frm = head if k == 0 else 0
    return lo, frm, frm + (hi - lo)


def test_block_cover(prog):
    rng = np.random.default_rng(2026)
    cases = []
    for _ in range(2000):
        pos = int(rng.integers(0, 1 << 62)) >> int(rng.integers(0, 62))
        n = 1 + (int(rng.integers(0, 1 << 40)) >> int(rng.integers(0, 40)))
        cases.append((pos, n))
    cases += [(0, 1), (0, 16), (0, 17), (15, 1), (15, 2), (5, 11), (5, 12), (32, 4112), (8, 24), (33, 4112),
              ((1 << 36) + 5, 40), ((1 << 64) - 2, 1), ((1 << 64) - 17, 16), (0, (1 << 64) - 1), (7, (1 << 64) - 8)]
    out = run(prog, ["C %d %d" % c for c in cases] + ["C %d 2" % ((1 << 64) - 2), "C 1 %d" % ((1 << 64) - 1)])
    assert out[-2:] == ["refused", "refused"]  # the range would end past 2^64 - 1
    for (pos, n), line in zip(cases, out):
        f = line.split()
        first, last = pos // 16, (pos + n - 1) // 16
        nblocks = last - first + 1
        assert f[:7] == ["ok", str(first), str(nblocks), str(pos % 16), str(-(-nblocks // 64)), str(pos // 16), str(pos % 16)], (pos, n, line)
        ks = range(nblocks) if nblocks <= 300 else (0, 1, nblocks - 1)
        assert len(f) == 7 + len(ks)
        covered = 0
        for k, got in zip(ks, f[7:]):
            at, frm, to = want_piece(pos, n, k)
            assert got == "%d:%d:%d:%d" % (k, at, frm, to), (pos, n, k, got)
            assert 0 <= frm < to <= 16 and at + (to - frm) <= n
            covered += to - frm
        if nblocks <= 300:
            assert covered == n
