"""CPU check of the split level kernels' launch geometry (mpc_amd/csrc/split_grid.h): the header is compiled into a small
C++ program with the host compiler, which walks the grid exactly as the kernels do (list index = blockIdx.y * gridDim.x +
blockIdx.x, entries past the list return) and reports what it covered.  Every grid dimension must be one HIP accepts
(blocks * 256 < 2^32 along x), and every (hashed gate, chunk) and (free-gate block, instance block) must be visited
exactly once — including past 2^24 workgroups, where a 1-D grid is refused (e.g. 64 Ki instances, 16 Ki hashed gates)."""
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpc_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <vector>

#include "split_grid.h"

using namespace gc;

// one case per line: count nonfree batch lg per -> one line of results
int main() {
    unsigned long long count, nonfree, batch, lg, per;
    while (std::scanf("%llu %llu %llu %llu %llu", &count, &nonfree, &batch, &lg, &per) == 5) {
        const SplitGrid s = split_grid((uint32_t)count, (uint32_t)nonfree, (uint32_t)batch, (uint32_t)lg, (uint32_t)per);
        if (!s.ok) {
            std::printf("refused\n");
            continue;
        }
        const unsigned long long yblocks = (batch + 255) / 256, nfree = count - nonfree;
        const unsigned long long total = (unsigned long long)s.gx * s.gy;
        int walked = 0;
        long long dup = 0, missing = 0, stray = 0;
        if (total <= (1ull << 26)) {  // walk the whole grid as the kernels do
            walked = 1;
            std::vector<bool> hash_seen((size_t)nonfree * s.chunks), free_seen(nfree ? (size_t)s.gx_free * yblocks : 0);
            for (uint32_t y = 0; y < s.gy; y++)
                for (uint32_t x = 0; x < s.gx; x++) {
                    const uint32_t bid = y * s.gx + x;
                    if (bid >= s.nblocks) continue;
                    const SplitBlock b = split_block(bid, s.chunks, s.nb_hash, s.gx_free);
                    if (b.hash) {
                        if (b.gate >= nonfree || b.sub >= s.chunks) { stray++; continue; }
                        const size_t k = (size_t)b.gate * s.chunks + b.sub;
                        dup += hash_seen[k];
                        hash_seen[k] = true;
                    } else {
                        if (!nfree || b.gate >= s.gx_free || b.sub >= yblocks) { stray++; continue; }
                        const size_t k = (size_t)b.sub * s.gx_free + b.gate;
                        dup += free_seen[k];
                        free_seen[k] = true;
                    }
                }
            for (bool v : hash_seen) missing += !v;
            for (bool v : free_seen) missing += !v;
        }
        std::printf("ok %u %u %u %u %u %u %d %lld %lld %lld\n", s.gx, s.gy, s.nblocks, s.chunks, s.nb_hash, s.gx_free, walked,
                    dup, missing, stray);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def geometry(tmp_path_factory):
    d = tmp_path_factory.mktemp("split_grid")
    src, exe = d / "split_grid_check.cpp", d / "split_grid_check"
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(cases):
        text = "".join("%d %d %d %d %d\n" % c for c in cases)
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        return lines

    return run


def lg_of(batch):
    """BatchGeom::lg (make_geom, gc_kernels.hip)"""
    return 8 if batch >= 256 else max(0, (batch - 1).bit_length())


def cases():
    out = []
    batches = [1, 2, 5, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1024, 1030, 4096, 65535, 65536, 65537, 1 << 20,
               (1 << 24) + 3, (1 << 31) + 5, (1 << 32) - 1]
    levels = [(1, 1), (7, 7), (48, 10), (700, 0), (700, 280), (1 << 14, 1 << 14), ((1 << 14) + 7, 1 << 14),
              ((1 << 18) + 3, (1 << 18) + 3), ((1 << 18) + 300, (1 << 18) + 3), (1 << 20, 1 << 19), ((1 << 29) - 1, (1 << 29) - 1),
              ((1 << 29) - 1, 1), ((1 << 32) - 1, (1 << 32) - 1), ((1 << 32) - 1, 1)]
    for batch in batches:
        for count, nonfree in levels:
            if nonfree == 0:
                continue  # the split kernels run only levels with a hashed gate
            for per in (64, 128):
                out.append((count, nonfree, batch, lg_of(batch), per))
    return out


def test_split_grid_is_legal_and_covers_every_block_once(geometry):
    cs = cases()
    walked = 0
    for (count, nonfree, batch, lg, per), line in zip(cs, geometry(cs)):
        what = "count %d nonfree %d batch %d per %d: %s" % (count, nonfree, batch, per, line)
        chunks = -(-batch // per)
        nfree, per_blk, yblocks = count - nonfree, 256 >> lg, -(-batch // 256)
        gx_free = -(-nfree // per_blk) if nfree else 1
        nblocks = nonfree * chunks + (gx_free * yblocks if nfree else 0)
        f = line.split()
        if f[0] == "refused":
            # only a list no legal grid holds may be refused: more than 65 535 rows of 2^16 workgroups
            assert nblocks > 65535 * (1 << 16), what
            continue
        gx, gy, nb, ch, nbh, gxf, w, dup, missing, stray = (int(x) for x in f[1:])
        assert (nb, ch, nbh, gxf) == (nblocks, chunks, nonfree * chunks, gx_free), what
        # HIP's limits: gridDim * blockDim < 2^32 in each dimension; the list index itself fits in 32 bits
        assert 1 <= gx and gx * 256 < 1 << 32, what
        assert 1 <= gy <= 65535, what
        assert gx * gy < 1 << 32, what
        assert gx * gy >= nblocks, what
        if nblocks < 1 << 24:
            assert (gx, gy) == (nblocks, 1), "below 2^24 workgroups the grid stays 1-D: " + what
        else:
            assert gx * (gy - 1) < nblocks, "no row of the grid is empty: " + what
        # chunks of `per` cover the batch exactly; free-gate blocks cover the free gates and instances
        assert (chunks - 1) * per < batch <= chunks * per, what
        if w:
            walked += 1
            assert (dup, missing, stray) == (0, 0, 0), what
    assert walked >= 100


def test_split_grid_advice_example(geometry):
    """batch 65 536 and >= 16 Ki hashed gates in one level: nonfree * ceil(batch / 64) = 2^24 workgroups, one past what a 1-D
    grid of 256-thread workgroups may hold; also the old limit's test shape (2^18 + 3 INV gates x 4 096 instances) and 2^31
    workgroups (2^17 hashed gates x 2^20 instances)"""
    cs = [(1 << 14, 1 << 14, 65536, 8, 64), ((1 << 14) + 40, 1 << 14, 65536, 8, 64), (1 << 15, 1 << 15, 65536, 8, 128),
          ((1 << 18) + 3, (1 << 18) + 3, 4096, 8, 64), (1 << 17, 1 << 17, 1 << 20, 8, 64)]
    for c, line in zip(cs, geometry(cs)):
        f = line.split()
        assert f[0] == "ok", (c, line)
        gx, gy, nblocks = int(f[1]), int(f[2]), int(f[3])
        assert gx * 256 < 1 << 32 and gy <= 65535 and gx * gy >= nblocks, (c, line)
        assert nblocks >= c[1] * -(-c[2] // c[4]) >= 1 << 24, (c, line)
        if int(f[7]):
            assert f[8:] == ["0", "0", "0"], (c, line)
