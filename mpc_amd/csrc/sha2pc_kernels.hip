// sha2pc_kernels.hip — what lies between the device calls under the sha2pc rounds and the bytes a peer sees, for S sessions
// per launch (gcengine.h: gc_sha2pc_*, sha2pc.h).  The compute stays where it is: gc_co_multi_*,
// gc_batch_*_keyed, the dense table egress / ingest and the gathers.  Here:
//
//   k_s2_r1_encode    one lane = one session: "R1", sid, curve chunk, A
//   k_s2_r2_take      one lane = one session: the header checks of Round 1 and A's, A and sid moved out
//   k_s2_r2_encode    one lane = one (session, OT): X of the choice point; the sign bytes by a ballot over eight lanes
//   k_s2_r3_decode    one lane = one (session, OT): X and the sign bit -> the point (p256_sqrt.h: one square root mod p);
//                     the lowest index of a session that does not decode by a wave reduction
//   k_s2_r3_header    one lane = one session: the verdict of Round 3 in the reference's order
//   k_s2_r3_assemble  one lane = one 16-byte field of Round 3 outside the tables: a garbler label, a hint, a ciphertext
//                     half; one more lane per session for magic, sid and key
//   k_s2_zero_bad     zero bytes over the tables of a bad session
//   k_s2_r4_take      the reverse of assemble, with the header checks of Round 3
//   k_s2_r4_decode    one wave = 64 consecutive outputs of one session: BitFromLabel against the hints in the payload, the
//                     bits packed by a ballot
//   k_s2_r4_verdict   one lane = one session: LABEL, and the zero digest of a bad session
//
// Layout.  A payload array is [S][stride] bytes, stride a multiple of 16; Rounds 1 and 2 begin at byte 0 of a slot, Round 3 at
// byte 6, so that every 32-byte and 16-byte field of every round is an aligned 16-byte access.  Per-OT arrays are
// session-major (gc_co_multi_*).  Where a wave must sit in one session (the reductions) the lanes of a session are padded to
// a multiple of 64, and to a multiple of 8 for the sign bytes; the grids are capped and stride by a multiple of 64.
// Every address is computed from the session number, the field number and the geometry: no payload byte is an index.
// No kernel waits on another; the atomics are met by a session with a fault alone.
#include <algorithm>

#include "co_lane.h"
#include "p256_sqrt.h"
#include "sha2pc.h"

namespace gc {

namespace {

constexpr int kS2Threads = 256;
constexpr unsigned kS2Grid = 8192;

// the last word of the curve chunk "\x05P-256", and its first two bytes
constexpr uint32_t kChunkTail = 0x3635322du;  // "-256"
constexpr uint32_t kChunkHead = 0x5005u;      // 0x05 'P'
constexpr uint32_t kMagicR1 = 0x3152u, kMagicR2 = 0x3252u, kMagicR3 = 0x3352u;  // "R1", "R2", "R3" as little-endian u16

// the 16 header bytes of Rounds 1 and 2: magic[2], sid[8], chunk[6]
__device__ __forceinline__ uint4 s2_header(uint32_t magic, uint2 sid) {
    return make_uint4(magic | (sid.x << 16), (sid.x >> 16) | (sid.y << 16), (sid.y >> 16) | (kChunkHead << 16), kChunkTail);
}
__device__ __forceinline__ uint2 s2_header_sid(const uint4 h) {
    return make_uint2((h.x >> 16) | (h.y << 16), (h.y >> 16) | (h.z << 16));
}
// MAGIC, CURVE or 0
__device__ __forceinline__ uint32_t s2_header_code(const uint4 h, uint32_t magic) {
    if ((h.x & 0xffffu) != magic) return kS2Magic;
    if ((h.z >> 16) != kChunkHead || h.w != kChunkTail) return kS2Curve;
    return 0u;
}
__device__ __forceinline__ uint4 s2_zero4() { return make_uint4(0u, 0u, 0u, 0u); }
__device__ __forceinline__ uint4 s2_pick(bool c, const uint4 v) { return c ? v : s2_zero4(); }
// a label in the engine's form <-> its 16 payload bytes BE(D0) || BE(D1)
__device__ __forceinline__ uint4 s2_label_bytes(const uint4 l) { return bswap4(label_be_words(l)); }
__device__ __forceinline__ uint4 s2_bytes_label(const uint4 c) { return label_be_words(bswap4(c)); }
__device__ __forceinline__ bool s2_eq(const uint4 a, const uint4 b) {
    return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) == 0u;
}
__device__ __forceinline__ const uint4 *s2_at(const uint8_t *base, size_t byte) {
    return reinterpret_cast<const uint4 *>(base + byte);
}
__device__ __forceinline__ uint4 *s2_at(uint8_t *base, size_t byte) { return reinterpret_cast<uint4 *>(base + byte); }
// VALID as gc_co_multi_* define it
__device__ __forceinline__ bool s2_point_valid(const uint4 *p) {
    Aff q;
    return pt_on_curve(load_be_fe(p), load_be_fe(p + 2), q);
}

#define S2_FOR(i, n) \
    for (size_t i = (size_t)blockIdx.x * kS2Threads + threadIdx.x; i < (n); i += (size_t)gridDim.x * kS2Threads)

__global__ __launch_bounds__(kS2Threads) void k_s2_r1_encode(size_t S, const uint4 *__restrict__ A,
                                                             const uint2 *__restrict__ sid, uint8_t *__restrict__ r1,
                                                             size_t stride1, uint32_t *__restrict__ verdict) {
    S2_FOR(s, S) {
        const uint4 a0 = A[4 * s], a1 = A[4 * s + 1], a2 = A[4 * s + 2], a3 = A[4 * s + 3];
        // a bad session (a = 0 mod N) has zero bytes for A from k_co_multi_setup; no point of the curve is (0, 0)
        const bool ok = !(s2_eq(a0, s2_zero4()) && s2_eq(a1, s2_zero4()) && s2_eq(a2, s2_zero4()) && s2_eq(a3, s2_zero4()));
        uint4 *out = s2_at(r1, s * stride1);
        out[0] = s2_pick(ok, s2_header(kMagicR1, sid[s]));
        out[1] = a0;
        out[2] = a1;
        out[3] = a2;
        out[4] = a3;
        verdict[s] = ok ? 0u : kS2Setup;
    }
}

__global__ __launch_bounds__(kS2Threads) void k_s2_r2_take(size_t S, const uint8_t *__restrict__ r1, size_t stride1,
                                                           uint4 *__restrict__ A_out, uint2 *__restrict__ sid_out,
                                                           uint32_t *__restrict__ verdict) {
    S2_FOR(s, S) {
        const uint4 *in = s2_at(r1, s * stride1);
        const uint4 h = in[0];
        uint32_t code = s2_header_code(h, kMagicR1);
        if (code == 0u && !s2_point_valid(in + 1)) code = kS2Setup;  // ensureOnCurve(Ax, Ay) of BuildCOChoices
        const bool ok = code == 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) A_out[4 * s + k] = s2_pick(ok, in[1 + k]);
        const uint2 id = s2_header_sid(h);
        sid_out[s] = ok ? id : make_uint2(0u, 0u);
        verdict[s] = code;
    }
}

__global__ __launch_bounds__(kS2Threads) void k_s2_r2_encode(size_t n, uint32_t ne, uint32_t ne8,
                                                             const uint4 *__restrict__ points, const uint2 *__restrict__ sid,
                                                             const uint32_t *__restrict__ verdict, uint8_t *__restrict__ r2,
                                                             size_t stride2) {
    // n = S * ne8 is a multiple of 8 and so is the grid's stride: eight neighbouring lanes are in the loop together
    S2_FOR(i, n) {
        const size_t s = i / ne8;
        const uint32_t j = (uint32_t)(i - s * ne8);
        const bool live = j < ne, ok = verdict[s] == 0u;
        uint8_t *slot = r2 + s * stride2;
        bool odd = false;
        if (live) {
            const uint4 *p = points + 4 * (s * ne + j);
            odd = ok && ((p[3].w >> 24) & 1u);  // the last byte of the big-endian y
            uint4 *x = s2_at(slot, kS2HeaderBytes + 32 * (size_t)j);
            x[0] = s2_pick(ok, p[0]);
            x[1] = s2_pick(ok, p[1]);
        }
        const unsigned long long odds = __builtin_amdgcn_ballot_w64(odd);
        const unsigned lane = threadIdx.x & 63u;
        if (live && (j & 7u) == 0u) slot[kS2HeaderBytes + 32 * (size_t)ne + j / 8] = (uint8_t)(odds >> lane);
        if (j == 0u) *s2_at(slot, 0) = s2_pick(ok, s2_header(kMagicR2, sid[s]));
    }
}

__global__ __launch_bounds__(kS2Threads) void k_s2_r3_decode(size_t n, uint32_t ne, uint32_t ne64,
                                                             const uint8_t *__restrict__ r2, size_t stride2,
                                                             uint4 *__restrict__ points_out, uint32_t *badidx) {
    // n = S * ne64: a wave sits in one session
    S2_FOR(i, n) {
        const size_t s = i / ne64;
        const uint32_t j = (uint32_t)(i - s * ne64);
        const uint8_t *slot = r2 + s * stride2;
        bool bad = false;
        if (j < ne) {
            const bool odd = (slot[kS2HeaderBytes + 32 * (size_t)ne + j / 8] >> (j & 7u)) & 1u;
            Fe x, y;
            bad = !pt_decompress(load_be_fe(s2_at(slot, kS2HeaderBytes + 32 * (size_t)j)), odd, x, y);
            uint4 *out = points_out + 4 * (s * ne + j);
            store_be_fe(out, x);
            store_be_fe(out + 2, y);
        }
        const unsigned long long bads = __builtin_amdgcn_ballot_w64(bad);
        const unsigned lane = threadIdx.x & 63u;
        if (bads != 0ull && lane == 0u) atomicMin(badidx + s, j + (uint32_t)__builtin_ctzll(bads));
    }
}

__global__ __launch_bounds__(kS2Threads) void k_s2_r3_header(size_t S, const uint8_t *__restrict__ r2, size_t stride2,
                                                             const uint2 *__restrict__ sid, const uint4 *__restrict__ a,
                                                             const uint4 *__restrict__ AaInv,
                                                             const uint32_t *__restrict__ badidx,
                                                             uint32_t *__restrict__ verdict) {
    S2_FOR(s, S) {
        // DecodeRound2 (magic, curve, points), then GarblerRound3's sid, then EncryptCOCiphertexts' setup
        const uint4 h = *s2_at(r2, s * stride2);
        uint32_t code = s2_header_code(h, kMagicR2);
        const uint32_t idx = badidx[s];
        if (code == 0u && idx != 0xffffffffu) code = kS2Point | (idx << 8);
        const uint2 id = s2_header_sid(h), own = sid[s];
        if (code == 0u && (id.x != own.x || id.y != own.y)) code = kS2Session;
        if (code == 0u && (fe_is_zero(sc_reduce(load_be_fe(a + 2 * s))) || !s2_point_valid(AaInv + 4 * s))) code = kS2Setup;
        verdict[s] = code;
    }
}

__global__ __launch_bounds__(kS2Threads) void k_s2_r3_assemble(Sha2pcGeom g, size_t n, const uint4 *__restrict__ gwires,
                                                               const uint8_t *__restrict__ bits,
                                                               const uint4 *__restrict__ outs, const uint4 *__restrict__ R,
                                                               const uint4 *__restrict__ ct, const uint2 *__restrict__ sid,
                                                               const uint4 *__restrict__ keys,
                                                               const uint32_t *__restrict__ verdict, uint8_t *__restrict__ r3,
                                                               size_t stride3) {
    const size_t per = (size_t)g.ng + 2 * (size_t)g.nout + 2 * (size_t)g.ne + 1;
    S2_FOR(i, n) {
        const size_t s = i / per;
        size_t u = i - s * per;
        const bool ok = verdict[s] == 0u;
        uint8_t *slot = r3 + s * stride3;
        if (u < g.ng) {  // LabelForBit(wire, bit)
            const size_t w = s * g.ng + u;
            *s2_at(slot, g.at_glabels() + 16 * u) = s2_pick(ok, s2_label_bytes(gwires[2 * w + (bits[w] ? 1 : 0)]));
            continue;
        }
        u -= g.ng;
        if (u < 2 * (size_t)g.nout) {  // L0 and L0 ^ R of output wire u / 2
            uint4 l = outs[(u >> 1) * g.bstride + s];
            if (u & 1) {
                const uint4 r = R[s];
                l = make_uint4(l.x ^ r.x, l.y ^ r.y, l.z ^ r.z, l.w ^ r.w);
            }
            *s2_at(slot, g.at_hints() + 16 * u) = s2_pick(ok, s2_label_bytes(l));
            continue;
        }
        u -= 2 * (size_t)g.nout;
        if (u < 2 * (size_t)g.ne) {
            *s2_at(slot, g.at_ct() + 16 * u) = s2_pick(ok, ct[2 * s * g.ne + u]);
            continue;
        }
        // bytes 6 .. 47 of the slot: "R3", sid, key
        *reinterpret_cast<uint16_t *>(slot + kS2Round3Lead) = ok ? (uint16_t)kMagicR3 : (uint16_t)0;
        *reinterpret_cast<uint2 *>(slot + 8) = ok ? sid[s] : make_uint2(0u, 0u);
        *s2_at(slot, 16) = s2_pick(ok, keys[2 * s]);
        *s2_at(slot, 32) = s2_pick(ok, keys[2 * s + 1]);
    }
}

__global__ __launch_bounds__(kS2Threads) void k_s2_zero_bad(const uint32_t *__restrict__ verdict, uint8_t *__restrict__ base,
                                                            size_t stride, size_t at, size_t n16) {
    const size_t s = blockIdx.x;
    if (verdict[s] == 0u) return;
    uint4 *p = s2_at(base, s * stride + at);
    for (size_t k = (size_t)blockIdx.y * kS2Threads + threadIdx.x; k < n16; k += (size_t)gridDim.y * kS2Threads)
        p[k] = s2_zero4();
}

__global__ __launch_bounds__(kS2Threads) void k_s2_r4_take(Sha2pcGeom g, size_t n, const uint8_t *__restrict__ r3,
                                                           size_t stride3, const uint2 *__restrict__ sid,
                                                           const uint4 *__restrict__ A, uint4 *__restrict__ keys_out,
                                                           uint4 *__restrict__ glabels_out, uint4 *__restrict__ ct_out,
                                                           uint32_t *__restrict__ verdict) {
    const size_t per = (size_t)g.ng + 2 * (size_t)g.ne + 1;
    S2_FOR(i, n) {
        const size_t s = i / per;
        size_t u = i - s * per;
        const uint8_t *slot = r3 + s * stride3;
        if (u < g.ng) {
            glabels_out[s * g.ng + u] = s2_bytes_label(*s2_at(slot, g.at_glabels() + 16 * u));
            continue;
        }
        u -= g.ng;
        if (u < 2 * (size_t)g.ne) {
            ct_out[2 * s * g.ne + u] = *s2_at(slot, g.at_ct() + 16 * u);
            continue;
        }
        // DecodeRound3's magic, EvaluatorRound4's sid, DecryptCOCiphertexts' ensureOnCurve(Ax, Ay)
        const uint32_t magic = *reinterpret_cast<const uint16_t *>(slot + kS2Round3Lead);
        const uint2 id = *reinterpret_cast<const uint2 *>(slot + 8), own = sid[s];
        uint32_t code = 0u;
        if (magic != kMagicR3) code = kS2Magic;
        else if (id.x != own.x || id.y != own.y) code = kS2Session;
        else if (!s2_point_valid(A + 4 * s)) code = kS2Setup;
        keys_out[2 * s] = *s2_at(slot, 16);
        keys_out[2 * s + 1] = *s2_at(slot, 32);
        verdict[s] = code;
    }
}

__global__ __launch_bounds__(kS2Threads) void k_s2_r4_decode(Sha2pcGeom g, size_t n, uint32_t nout64,
                                                             const uint4 *__restrict__ outs, const uint8_t *__restrict__ r3,
                                                             size_t stride3, uint8_t *__restrict__ digest, uint32_t *badidx) {
    // n = S * nout64: a wave owns 64 consecutive outputs of one session
    S2_FOR(i, n) {
        const size_t s = i / nout64;
        const uint32_t j = (uint32_t)(i - s * nout64);
        bool one = false, bad = false;
        if (j < g.nout) {
            const uint4 l = s2_label_bytes(outs[(size_t)j * g.bstride + s]);
            const uint4 *hint = s2_at(r3 + s * stride3, g.at_hints() + 32 * (size_t)j);
            const bool is0 = s2_eq(l, hint[0]), is1 = s2_eq(l, hint[1]);  // BitFromLabel: L0 is asked first
            one = !is0 && is1;
            bad = !is0 && !is1;
        }
        const unsigned long long ones = __builtin_amdgcn_ballot_w64(one), bads = __builtin_amdgcn_ballot_w64(bad);
        const unsigned lane = threadIdx.x & 63u;
        const uint32_t byte = (j - lane) / 8 + lane;  // lanes 0 .. 7 write the wave's eight bytes
        if (lane < 8u && byte < g.digest_bytes()) digest[s * g.digest_bytes() + byte] = (uint8_t)(ones >> (8 * lane));
        if (bads != 0ull && lane == 0u) atomicMin(badidx + s, j + (uint32_t)__builtin_ctzll(bads));
    }
}

__global__ __launch_bounds__(kS2Threads) void k_s2_r4_verdict(size_t S, uint32_t digest_bytes,
                                                              const uint32_t *__restrict__ badidx,
                                                              uint32_t *__restrict__ verdict, uint8_t *__restrict__ digest) {
    S2_FOR(s, S) {
        uint32_t code = verdict[s];
        const uint32_t idx = badidx[s];
        if (code == 0u && idx != 0xffffffffu) code = kS2Label | (idx << 8);
        verdict[s] = code;
        if (code != 0u)
            for (uint32_t k = 0; k < digest_bytes; k++) digest[s * digest_bytes + k] = 0;
    }
}

__global__ __launch_bounds__(kS2Threads) void k_s2_repack(const uint8_t *__restrict__ src, size_t src_stride,
                                                          uint8_t *__restrict__ dst, size_t dst_stride, size_t len) {
    const size_t s = blockIdx.x;
    for (size_t k = (size_t)blockIdx.y * kS2Threads + threadIdx.x; k < len; k += (size_t)gridDim.y * kS2Threads)
        dst[s * dst_stride + k] = src[s * src_stride + k];
}

unsigned s2_grid(size_t n) { return (unsigned)std::min<size_t>(kS2Grid, (n + kS2Threads - 1) / kS2Threads); }
// one block column per session, up to 64 blocks over its n units
dim3 s2_grid2(size_t S, size_t n) { return dim3((unsigned)S, (unsigned)std::min<size_t>(64, (n + kS2Threads - 1) / kS2Threads)); }
size_t s2_round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }

}  // namespace

void launch_s2_r1_encode(size_t S, const uint4 *A, const uint2 *sid, uint8_t *r1, size_t stride1, uint32_t *verdict,
                         hipStream_t s) {
    hipLaunchKernelGGL(k_s2_r1_encode, dim3(s2_grid(S)), dim3(kS2Threads), 0, s, S, A, sid, r1, stride1, verdict);
}

void launch_s2_r2_take(size_t S, const uint8_t *r1, size_t stride1, uint4 *A_out, uint2 *sid_out, uint32_t *verdict,
                       hipStream_t s) {
    hipLaunchKernelGGL(k_s2_r2_take, dim3(s2_grid(S)), dim3(kS2Threads), 0, s, S, r1, stride1, A_out, sid_out, verdict);
}

void launch_s2_r2_encode(const Sha2pcGeom &g, const uint4 *points, const uint2 *sid, const uint32_t *verdict, uint8_t *r2,
                         size_t stride2, hipStream_t s) {
    const uint32_t ne8 = (uint32_t)s2_round_up(g.ne, 8);
    const size_t n = g.S * ne8;
    hipLaunchKernelGGL(k_s2_r2_encode, dim3(s2_grid(n)), dim3(kS2Threads), 0, s, n, g.ne, ne8, points, sid, verdict, r2,
                       stride2);
}

void launch_s2_r3_decode(const Sha2pcGeom &g, const uint8_t *r2, size_t stride2, uint4 *points_out, uint32_t *badidx,
                         hipStream_t s) {
    const uint32_t ne64 = (uint32_t)s2_round_up(g.ne, 64);
    const size_t n = g.S * ne64;
    hipLaunchKernelGGL(k_s2_r3_decode, dim3(s2_grid(n)), dim3(kS2Threads), 0, s, n, g.ne, ne64, r2, stride2, points_out,
                       badidx);
}

void launch_s2_r3_header(size_t S, const uint8_t *r2, size_t stride2, const uint2 *sid, const uint4 *a, const uint4 *AaInv,
                         const uint32_t *badidx, uint32_t *verdict, hipStream_t s) {
    hipLaunchKernelGGL(k_s2_r3_header, dim3(s2_grid(S)), dim3(kS2Threads), 0, s, S, r2, stride2, sid, a, AaInv, badidx,
                       verdict);
}

void launch_s2_r3_assemble(const Sha2pcGeom &g, const uint4 *gwires, const uint8_t *bits, const uint4 *outs, const uint4 *R,
                           const uint4 *ct, const uint2 *sid, const uint4 *keys, const uint32_t *verdict, uint8_t *r3,
                           size_t stride3, hipStream_t s) {
    const size_t n = g.S * ((size_t)g.ng + 2 * (size_t)g.nout + 2 * (size_t)g.ne + 1);
    hipLaunchKernelGGL(k_s2_r3_assemble, dim3(s2_grid(n)), dim3(kS2Threads), 0, s, g, n, gwires, bits, outs, R, ct, sid, keys,
                       verdict, r3, stride3);
}

void launch_s2_zero_bad(size_t S, const uint32_t *verdict, uint8_t *base, size_t stride, size_t at, size_t n16,
                        hipStream_t s) {
    if (n16 == 0) return;
    hipLaunchKernelGGL(k_s2_zero_bad, s2_grid2(S, n16), dim3(kS2Threads), 0, s, verdict, base, stride, at, n16);
}

void launch_s2_r4_take(const Sha2pcGeom &g, const uint8_t *r3, size_t stride3, const uint2 *sid, const uint4 *A,
                       uint4 *keys_out, uint4 *glabels_out, uint4 *ct_out, uint32_t *verdict, hipStream_t s) {
    const size_t n = g.S * ((size_t)g.ng + 2 * (size_t)g.ne + 1);
    hipLaunchKernelGGL(k_s2_r4_take, dim3(s2_grid(n)), dim3(kS2Threads), 0, s, g, n, r3, stride3, sid, A, keys_out,
                       glabels_out, ct_out, verdict);
}

void launch_s2_r4_decode(const Sha2pcGeom &g, const uint4 *outs, const uint8_t *r3, size_t stride3, uint8_t *digest,
                         uint32_t *badidx, hipStream_t s) {
    const uint32_t nout64 = (uint32_t)s2_round_up(g.nout, 64);
    const size_t n = g.S * nout64;
    hipLaunchKernelGGL(k_s2_r4_decode, dim3(s2_grid(n)), dim3(kS2Threads), 0, s, g, n, nout64, outs, r3, stride3, digest,
                       badidx);
}

void launch_s2_r4_verdict(size_t S, uint32_t digest_bytes, const uint32_t *badidx, uint32_t *verdict, uint8_t *digest,
                          hipStream_t s) {
    hipLaunchKernelGGL(k_s2_r4_verdict, dim3(s2_grid(S)), dim3(kS2Threads), 0, s, S, digest_bytes, badidx, verdict, digest);
}

void launch_s2_repack(size_t S, const uint8_t *src, size_t src_stride, uint8_t *dst, size_t dst_stride, size_t len,
                      hipStream_t s) {
    if (len == 0) return;
    hipLaunchKernelGGL(k_s2_repack, s2_grid2(S, len), dim3(kS2Threads), 0, s, src, src_stride, dst, dst_stride, len);
}

}  // namespace gc
