// stream_batch.h — launch wrappers of the session-batched streaming engine (stream_batch_kernels.hip; the host side is
// stream_batch.cpp): S sessions of one streamed program, a step = one keyed batch pass over S instances.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace gcsb {

constexpr uint32_t kThreads = 256;
// bytes of ONE session's step that one workgroup of the serialiser / ingester handles: the piece is built in LDS at the
// alignment of its place in the session's byte stream and moved as whole 16-byte lines
constexpr uint32_t kPieceBytes = 4096;

// What is the same for every session of a step, in device memory (one upload per step):
//   skel       the step's bytes with zeros where the table rows go — op | flag bytes and wire ids (circuit/stream_garble.go:
//              391-441), which depend on nothing secret; readable up to the next multiple of 16 past nbytes
//   row_off    byte offset of table row r, in slab order = stream order (ascending)
//   piece_row  [npieces]: the first row that ends behind the piece's first byte (row_off + 16 > piece * kPieceBytes)
struct StepDev {
    const uint8_t *skel;
    const uint32_t *row_off;
    const uint32_t *piece_row;
    uint32_t nbytes, nrows, npieces, pad_;
};

// rnd [S][n1] labels as launch_gather left them (column 0 unset) -> the d_rnd form of gc_batch_garble_keyed: big-endian label
// bytes, column 0 = R[s]
void launch_rnd_form(uint4 *rnd, const uint4 *R, uint32_t S, uint32_t n1, hipStream_t s);
// the create call: R[s] and store[ids[j]][s] from rnd u8 [S][1 + n][16] (ids 0xffffffff: skipped)
void launch_init_store(const uint4 *rnd, const uint32_t *ids, uint32_t n, uint4 *store, uint32_t bstride, uint4 *R, uint32_t S,
                       hipStream_t s);
// dst[dl.at(drow[j], s)] = src[sl.at(srow[j], s)] for j < n, s < S; a null map is the identity, a row 0xffffffff is skipped
void launch_rows(const uint4 *src, const gc::Layout &sl, const uint32_t *srow, uint4 *dst, const gc::Layout &dl,
                 const uint32_t *drow, uint32_t n, uint32_t S, hipStream_t s);
// session s's step bytes at out + s * stride: the skeleton with row r = BE(D0) || BE(D1) of T[lt.at(r, s)]
void launch_serialise(const StepDev &d, const uint4 *T, const gc::Layout &lt, uint8_t *out, size_t stride, uint32_t S,
                      hipStream_t s);
// bytes [b0, b1) of the same, b1 <= d.nbytes: session s's byte b0 + i at out + s * stride + i (k_sb_serialise_range; any b0, any
// alignment of out).  Writes b1 - b0 bytes per session and nothing else.
void launch_serialise_range(const StepDev &d, const uint4 *T, const gc::Layout &lt, uint8_t *out, size_t stride, uint32_t S,
                            uint32_t b0, uint32_t b1, hipStream_t s);
// the inverse: rows of session s's block (in + s * stride) into T, and bad[s] += bytes outside the rows that differ from the
// skeleton.  Reads bytes [0, nbytes) of every block and nothing else.
void launch_ingest(const StepDev &d, uint4 *T, const gc::Layout &lt, const uint8_t *in, size_t stride, uint32_t S, uint32_t *bad,
                   hipStream_t s);

// the tile of the two movers below: ids x sessions, and the most tiles along the ids that one grid holds (more are swept)
constexpr uint32_t kIoIds = 64, kIoSessions = 32, kIoMaxTiles = 1024;
// out [S][n] = store[ids[j]][s] ^ (bits[s][n] ? R[s] : 0): the garbler's label for a bit (streamer.go:79-102)
void launch_select(const uint4 *store, uint32_t bstride, const uint32_t *ids, uint32_t n, const uint4 *R, const uint8_t *bits,
                   uint4 *out, uint32_t S, hipStream_t s);
// bits_out [S][n] = 0 / 1 / 0xff for labels [S][n] equal to store[ids[j]][s] / that ^ R[s] / neither (streamer.go:563-579), and
// bad[s] += session s's 0xff entries (one add per wave that saw any)
void launch_decode_labels(const uint4 *store, uint32_t bstride, const uint32_t *ids, uint32_t n, const uint4 *R, const uint4 *labels,
                          uint8_t *bits_out, uint32_t *bad, uint32_t S, hipStream_t s);

// out [S][n] = store[ids[j]][s]: the evaluator's active labels in the order gc_stream_batch_decode_dev reads them
// (stream_evaluator.go:434-461)
void launch_return_labels(const uint4 *store, uint32_t bstride, const uint32_t *ids, uint32_t n, uint4 *out, uint32_t S, hipStream_t s);

// the OpCircuit header in front of a block: BE32 op, step, numGates, numTmpWires, numWires (streamer.go:679-693)
constexpr uint32_t kFrameBytes = 20;
// bad[s] += the bytes of [off[m], off[m] + kFrameBytes) that differ between row s and row `ref` of buf [S][pitch], summed over
// m < nmsg (one add per wave that saw a difference).  Reads those bytes and nothing else.
void launch_frames(const uint8_t *buf, size_t pitch, const uint32_t *off, uint32_t nmsg, uint32_t S, uint32_t ref, uint32_t *bad,
                   hipStream_t s);

}  // namespace gcsb
