// split_grid.h — launch geometry of the split level kernels (k_garble_level_split / k_eval_level_split, gc_kernels.hip).
// Plain C++ with no HIP types, so that a host-only test can compile it (tests/test_split_grid.py).
//
// A split level launch is a list of workgroups: first the hash workgroups, one per (table-producing gate, chunk of PER
// instances), gate-major; behind them the free-gate blocks, one per (block of 256 >> lg gates, block of 256 instances),
// gate-block-minor.  HIP rejects a launch whose gridDim.x * blockDim.x (256) reaches 2^32, i.e. 2^24 workgroups along x:
// nonfree * ceil(batch / 64) passes that at 64 Ki instances and 16 Ki hashed gates, and the 32-bit product itself wraps
// further out.  The block count is therefore computed in 64 bits and, past 2^24 - 1 workgroups, the list is spread over
// grid.y rows of kSplitRowBlocks; the kernel takes its list index as blockIdx.y * gridDim.x + blockIdx.x, and the
// (< kSplitRowBlocks) workgroups past the end of the list return at once.  This keeps the split kernels (and their bytes)
// at every size rather than falling back to the whole-gate level kernels: those are slower and have a grid limit of their
// own (ceil(count / (256 >> lg)) blocks along x).  Below 2^24 workgroups the grid is the 1-D one it always was.
#pragma once

#include <cstdint>

namespace gc {

constexpr uint64_t kSplitMaxX = (1u << 24) - 1;   // workgroups along x: (2^24 - 1) * 256 < 2^32
constexpr uint32_t kSplitRowBlocks = 1u << 16;   // workgroups per grid.y row once the list is spread
constexpr uint32_t kSplitMaxY = 65535;           // grid.y rows

struct SplitGrid {
    uint32_t chunks;   // instance chunks of PER per hashed gate: ceil(batch / PER)
    uint32_t nb_hash;  // hash workgroups: nonfree * chunks
    uint32_t gx_free;  // free-gate blocks along the gate axis (1 when the level has no free gate)
    uint32_t nblocks;  // workgroups in the list: nb_hash + free-gate blocks
    uint32_t gx, gy;   // launch grid (gx * gy >= nblocks)
    bool ok;           // false: the list does not fit any legal grid (nothing may be launched)
};

// count gates of which the first nonfree produce tables; lg = log2 of the free-gate blocks' instance tile (BatchGeom::lg);
// per = instances per hash workgroup (64 garbler, 128 evaluator)
inline SplitGrid split_grid(uint32_t count, uint32_t nonfree, uint32_t batch, uint32_t lg, uint32_t per) {
    SplitGrid s{};
    const uint64_t chunks = ((uint64_t)batch + per - 1) / per;
    const uint64_t nfree = (uint64_t)count - nonfree, per_blk = 256u >> lg;
    const uint64_t yblocks = ((uint64_t)batch + 255) / 256;  // BatchGeom::yblocks (1 below 256 instances)
    const uint64_t gx_free = nfree ? (nfree + per_blk - 1) / per_blk : 1;
    const uint64_t nb_hash = (uint64_t)nonfree * chunks;
    const uint64_t nblocks = nb_hash + (nfree ? gx_free * yblocks : 0);
    uint64_t gx = nblocks, gy = 1;
    if (nblocks > kSplitMaxX) {
        gx = kSplitRowBlocks;
        gy = (nblocks + gx - 1) / gx;
    }
    s.ok = gy <= kSplitMaxY && nblocks > 0;
    if (!s.ok) return s;
    s.chunks = (uint32_t)chunks;
    s.nb_hash = (uint32_t)nb_hash;
    s.gx_free = (uint32_t)gx_free;
    s.nblocks = (uint32_t)nblocks;
    s.gx = (uint32_t)gx;
    s.gy = (uint32_t)gy;
    return s;
}

// What list entry `bid` (< nblocks) does.  hash: gate = the hashed gate, sub = its chunk; else gate = the free-gate
// block along the gate axis (bx), sub = the instance block (by).
struct SplitBlock {
    bool hash;
    uint32_t gate, sub;
};

#if defined(__HIPCC__)
__host__ __device__
#endif
inline SplitBlock split_block(uint32_t bid, uint32_t chunks, uint32_t nb_hash, uint32_t gx_free) {
    SplitBlock b;
    if (bid >= nb_hash) {
        const uint32_t f = bid - nb_hash;
        b.hash = false;
        b.gate = f % gx_free;
        b.sub = f / gx_free;
    } else {
        b.hash = true;
        b.gate = bid / chunks;
        b.sub = bid - b.gate * chunks;
    }
    return b;
}

}  // namespace gc
