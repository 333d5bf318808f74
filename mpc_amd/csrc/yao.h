// yao.h — the geometry of circuit.Garbler's / circuit.Evaluator's messages for S sessions per call (gcengine.h: gc_yao_*,
// DESIGN.md §23) and the launchers of yao_kernels.hip.  The messages are those of circuit/garbler.go:64-167 and
// circuit/evaluator.go:31-148 in the framing of p2p/protocol.go:216-261.  No device code here: yao_engine.cpp includes it
// next to the host's headers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels.h"
#include "yao_m3.h"

namespace gc {

// the verdict codes (gcengine.h: GC_YAO_*); a verdict is code | index << 8
constexpr uint32_t kYaoKey = 1, kYaoGates = 2, kYaoRows = 3, kYaoLabel = 4, kYaoLength = 5;

// what the intake leaves per session for its verdict kernel: the lowest failing check, ~0 for none
constexpr uint32_t kYaoBadKey = 0, kYaoBadGates = 1, kYaoBadGate0 = 2;  // gate g: kYaoBadGate0 + g

// The M1 kernels give a workgroup piece p of a tile of consecutive sessions.  Chosen by measurement on one MI355X with aes_128
// x 1 024 sessions and 32-byte keys (profiles/yao_geometry.jsonl): 4 sessions x 4 096 bytes, 16.6 KB of LDS,
// nine workgroups per CU.  At 1 024 sessions the batch's own layout tile is 4 instances, so 4 sessions are one contiguous
// run per row; wider tiles and longer pieces lost to the occupancy they cost (16 x 4 096: twice the time), shorter pieces to
// the share of ragged rows (4 x 1 024: 1.7 times).  GC_YAO_TILE / GC_YAO_PIECE choose others at create.
constexpr uint32_t kYaoThreads = 256;
constexpr uint32_t kYaoTile = 4;           // sessions per workgroup: 4, 8, 16, 32 or 64
constexpr uint32_t kYaoPieceBytes = 4096;  // a multiple of 16, 64 .. 16 384
// LDS of a workgroup: a stage of piece_bytes + 16 per session (the line behind the piece takes the end of a row that begins
// in it, and keeps the stages 4 banks apart), then one word per session for the intake's lowest failing check
constexpr size_t yao_m1_lds_bytes(uint32_t tile, uint32_t piece_bytes) { return (size_t)tile * (piece_bytes + 16) + 4 * (size_t)tile; }

struct YaoGeom {
    uint32_t ng, ne, nout, ngates, rows, keylen;
    uint32_t len1;  // 4 + keylen + gc_tables_wire_bytes() + 16 ng
    size_t S;
    constexpr size_t len2() const { return 16 * (size_t)nout; }
    constexpr uint32_t bits_bytes() const { return yao_m3_bits_bytes(nout); }
    constexpr size_t slot3() const { return yao_m3_slot_bytes(nout); }
};

// the device copy of a YaoSkel (yao_skel.h)
struct YaoDev {
    const uint4 *skel;
    const uint32_t *gate_off, *row_off, *piece_gate, *piece_row;
    uint32_t ngates, nrows, keylen, ng;
    uint32_t at_tables, at_labels, len1;
    uint32_t piece_bytes, npieces, tile;
};

// M1 out: skeleton, key, table rows and the garbler's own labels (L0 ^ bit R of input wires 0 .. ng) of every session
hipError_t launch_yao_m1_out(const YaoDev &d, const uint4 *T, const Layout &lt, const uint4 *W, const Layout &lw, const uint4 *R,
                             const uint32_t *keys, const uint8_t *bits, uint8_t *m1, size_t stride1, uint32_t S, hipStream_t s);
// M1 in: the key to keys_out, the rows to T, the labels to input wires 0 .. ng of W; badidx[s] (set to ~0 by the caller) =
// the lowest failing check of session s
hipError_t launch_yao_m1_in(const YaoDev &d, uint4 *T, const Layout &lt, uint4 *W, const Layout &lw, uint32_t *keys_out,
                            const uint8_t *m1, size_t stride1, uint32_t S, uint32_t *badidx, hipStream_t s);
// badidx -> the verdict, to the caller's array and to the handle's
hipError_t launch_yao_m1_verdict(uint32_t S, const uint32_t *badidx, uint32_t *verdict, uint32_t *kept, hipStream_t s);
// M2 out: the evaluator's output labels, session-major and big-endian; a session with kept[s] != 0 gets zeros; verdict = kept
hipError_t launch_yao_m2_out(const YaoGeom &g, const uint4 *W, const Layout &lw, const uint32_t *out_slots, const uint32_t *kept,
                             uint8_t *m2, size_t stride2, uint32_t *verdict, hipStream_t s);
// M2 in and M3 out: BitFromLabel of every label against the garbler's output wires, the bits, the message, its length
hipError_t launch_yao_m2_decode(const YaoGeom &g, const uint4 *W, const Layout &lw, const uint32_t *out_slots, const uint4 *R,
                                const uint8_t *m2, size_t stride2, uint8_t *m3, size_t stride3, uint32_t *len3, uint8_t *bits_out,
                                uint32_t *verdict, hipStream_t s);
// M3 in
hipError_t launch_yao_m3_parse(const YaoGeom &g, const uint8_t *m3, size_t stride3, uint8_t *bits_out, uint32_t *verdict,
                               hipStream_t s);

}  // namespace gc
