// sha2pc.h — the geometry of the sha2pc rounds for S sessions per call (gcengine.h: gc_sha2pc_*) and the
// launchers of sha2pc_kernels.hip.  The encodings are those of sha2pc/encoding.go: EncodeRound1 :35, EncodeRound2 :84,
// EncodeRound3 :149.  No device code here: sha2pc_engine.cpp includes it next to the host's headers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct gc_ctx;

namespace gc {

// the verdict codes (gcengine.h: GC_SHA2PC_*); a verdict is code | index << 8
constexpr uint32_t kS2Magic = 1, kS2Curve = 2, kS2Session = 3, kS2Setup = 4, kS2Point = 5, kS2Label = 6;

constexpr size_t kS2HeaderBytes = 16;  // magic[2], sid[8], "\x05P-256" of Rounds 1 and 2
constexpr size_t kS2Round3Lead = 6;    // Round 3 begins at byte 6 of its slot: magic[2], sid[8], key[32] end at byte 48
constexpr size_t kS2TablesAt = 48;     // ... where the tables begin, in bytes from the slot

struct Sha2pcGeom {
    uint32_t ng, ne, nout, rows;
    uint32_t bstride;  // of the handle's batch
    size_t S;
    // Round 3 fields in bytes from the slot: the garbler's labels, the hints, the ciphertexts; all multiples of 16
    constexpr size_t at_glabels() const { return kS2TablesAt + 16 * (size_t)rows; }
    constexpr size_t at_hints() const { return at_glabels() + 16 * (size_t)ng; }
    constexpr size_t at_ct() const { return at_hints() + 32 * (size_t)nout; }
    constexpr size_t len1() const { return kS2HeaderBytes + 64; }
    constexpr size_t len2() const { return kS2HeaderBytes + 32 * (size_t)ne + (ne + 7) / 8; }
    constexpr size_t len3() const { return at_ct() + 32 * (size_t)ne - kS2Round3Lead; }
    constexpr uint32_t digest_bytes() const { return (nout + 7) / 8; }
};

// G's window table for the gc_co_multi_* calls a round makes (co_engine.cpp): uploaded by create, so that no round waits
int co_multi_prepare(gc_ctx *ctx);

// Round 1: header and A of every session; verdict = SETUP where the setup kernel left A zero
void launch_s2_r1_encode(size_t S, const uint4 *A, const uint2 *sid, uint8_t *r1, size_t stride1, uint32_t *verdict,
                         hipStream_t s);
// Round 2, from Round 1: the header checks and A's, A and sid moved out (zero for a bad session)
void launch_s2_r2_take(size_t S, const uint8_t *r1, size_t stride1, uint4 *A_out, uint2 *sid_out, uint32_t *verdict,
                       hipStream_t s);
// Round 2 encode: header, X of every choice point, the sign bytes
void launch_s2_r2_encode(const Sha2pcGeom &g, const uint4 *points, const uint2 *sid, const uint32_t *verdict, uint8_t *r2,
                         size_t stride2, hipStream_t s);
// Round 3, from Round 2: the choice points decompressed (badidx: lowest index per session that does not decode, else ~0;
// set to ~0 by the caller), then the verdict of every session
void launch_s2_r3_decode(const Sha2pcGeom &g, const uint8_t *r2, size_t stride2, uint4 *points_out, uint32_t *badidx,
                         hipStream_t s);
void launch_s2_r3_header(size_t S, const uint8_t *r2, size_t stride2, const uint2 *sid, const uint4 *a, const uint4 *AaInv,
                         const uint32_t *badidx, uint32_t *verdict, hipStream_t s);
// Round 3 assemble: everything but the tables
void launch_s2_r3_assemble(const Sha2pcGeom &g, const uint4 *gwires, const uint8_t *bits, const uint4 *outs, const uint4 *R,
                           const uint4 *ct, const uint2 *sid, const uint4 *keys, const uint32_t *verdict, uint8_t *r3,
                           size_t stride3, hipStream_t s);
// n16 units of 16 bytes at byte `at` of every BAD session's slot set to zero
void launch_s2_zero_bad(size_t S, const uint32_t *verdict, uint8_t *base, size_t stride, size_t at, size_t n16, hipStream_t s);
// Round 4, from Round 3: header checks and A's, the key, the garbler's labels and the ciphertexts moved out
void launch_s2_r4_take(const Sha2pcGeom &g, const uint8_t *r3, size_t stride3, const uint2 *sid, const uint4 *A,
                       uint4 *keys_out, uint4 *glabels_out, uint4 *ct_out, uint32_t *verdict, hipStream_t s);
// Round 4 decode: BitFromLabel of every output against the hints in the payload, then the verdict and the zeroing
void launch_s2_r4_decode(const Sha2pcGeom &g, const uint4 *outs, const uint8_t *r3, size_t stride3, uint8_t *digest,
                         uint32_t *badidx, hipStream_t s);
void launch_s2_r4_verdict(size_t S, uint32_t digest_bytes, const uint32_t *badidx, uint32_t *verdict, uint8_t *digest,
                          hipStream_t s);
// host forms: `len` bytes per session from src + s * src_stride to dst + s * dst_stride
void launch_s2_repack(size_t S, const uint8_t *src, size_t src_stride, uint8_t *dst, size_t dst_stride, size_t len,
                      hipStream_t s);

}  // namespace gc
