// kos_multi.h — the index arithmetic of the multi-session KOS check (gc_kos_multi_*, kos_multi_kernels.hip): S sessions of
// `per` OTs each, session-major.  A session's sums run over n = per + 256 labels: label i < per is result[s][i], label
// per + j is choice_vec[s][j], and chi_i is label i of the AES-128-CTR stream keyed by seed2[s] — the index restarts in every
// session and goes on at per, not at a padded length (ot/iknp.go:159-174, 422-454).  This header says which session a team of
// lanes owns, where label i of a session lies and where its choice bit lies.  Plain C++ without HIP types: hipcc compiles it
// for host and device, g++ for the walk of tests/test_kos_multi_index_host.py.  Everything is 64-bit.
//
//   result      [S][per] gc_label            choice_vec [S][256] gc_label
//   choice      [S][64 * ceil(per / 512)] bytes, packed LSB first: the buffer gc_iknp_multi_receive_dev consumed at `per`
//   bcv         [S][64] bytes, packed LSB first: the buffer of the call at 256 (bytes 32 .. 63 of a row are padding)
//   tags        [S][3] gc_label: x, t0, t1
//
// Teams.  A team is `team` consecutive lanes of a workgroup of kKosMultiThreads: one wave while n <= kKosMultiWaveMax, the
// whole workgroup above.  A workgroup holds tpw = threads / team teams and the grid is `grid` workgroups; team t of
// workgroup b takes, on its trip k, session (k * tpw + t) * grid + b: the sessions go round the WORKGROUPS first, so that S
// sessions short of one sweep (grid * tpw) still spread over min(S, grid) compute units instead of filling S / tpw of them.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GC_KOSM_FN __host__ __device__ inline
#else
#define GC_KOSM_FN inline
#endif

namespace gc {

constexpr uint32_t kKosCvLabels = 256;  // the random choice vector (iknp.go:382-394)
constexpr uint32_t kKosBcvRow = 64;     // bytes of a session's packed bcv: one chunk of the call at 256

// labels of one session's sums; per <= SIZE_MAX / 64 (the engine's size check), so this does not wrap
GC_KOSM_FN uint64_t kos_multi_labels(uint64_t per) { return per + kKosCvLabels; }
// bytes of a session's packed choice bits: iknp_multi_choice_bytes(per)
GC_KOSM_FN uint64_t kos_multi_choice_row(uint64_t per) { return ((per + 511) / 512) * 64; }
// one wave per session?  (wave_max = kKosMultiWaveMax)
GC_KOSM_FN bool kos_multi_wave_team(uint64_t per, uint32_t wave_max) {
    return wave_max >= kKosCvLabels && per <= (uint64_t)wave_max - kKosCvLabels;
}
// sessions one sweep of the grid covers
GC_KOSM_FN uint64_t kos_multi_sweep(uint32_t grid, uint32_t tpw) { return (uint64_t)grid * tpw; }
// workgroups of a launch: one per session until the cap
GC_KOSM_FN uint32_t kos_multi_grid(uint64_t S, uint32_t cap) { return (uint32_t)(S < cap ? S : cap); }
// the session of team `team` of workgroup `block` on its trip `trip`; the team is done when this is >= S
GC_KOSM_FN uint64_t kos_multi_session(uint32_t block, uint32_t team, uint64_t trip, uint32_t grid, uint32_t tpw) {
    return (trip * tpw + team) * grid + block;
}

struct KosMultiLabel {
    uint32_t in_cv;     // 0: the label is in result, 1: in choice_vec
    uint64_t off;       // element of that array
    uint64_t ctr;       // chi counter: the label's index in its session
    uint64_t bit_byte;  // byte of choice (in_cv = 0) or bcv (in_cv = 1) that holds the label's choice bit
    uint32_t bit;       // ... and the bit in it
};

// label i of kos_multi_labels(per) of session s
GC_KOSM_FN KosMultiLabel kos_multi_label(uint64_t s, uint64_t i, uint64_t per) {
    KosMultiLabel m;
    m.ctr = i;
    if (i < per) {
        m.in_cv = 0;
        m.off = s * per + i;
        m.bit_byte = s * kos_multi_choice_row(per) + i / 8;
        m.bit = (uint32_t)(i & 7u);
    } else {
        const uint64_t j = i - per;
        m.in_cv = 1;
        m.off = s * kKosCvLabels + j;
        m.bit_byte = s * kKosBcvRow + j / 8;
        m.bit = (uint32_t)(j & 7u);
    }
    return m;
}

}  // namespace gc
