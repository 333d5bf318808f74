// yao_skel.h — the skeleton and the piece table of circuit.Garbler's first message (gc_yao_*), built once per
// handle on the host.  No HIP here: yao_engine.cpp uploads the arrays, and tests/cpp/yao_host_check.cpp walks them.
//
// M1 of one session (circuit/garbler.go:64-102, p2p/protocol.go:216-261), offsets in bytes from the slot:
//   0            BE32(keylen)                     SendData(key)
//   4            key
//   at_tables    BE32(ngates)                     at_tables = 4 + keylen
//   ...          per gate BE32(rows), rows x 16   gate_off[g] = its row word, row_off[r] = row r of the slab
//   at_labels    ng x 16                          the garbler's own input labels
//   len1
// keylen is a multiple of 8, so every field is on a multiple of 4: the kernels move 32-bit words and 16-byte lines, never
// bytes.  The skeleton holds every word that is the same for all sessions (the three counts and the row words) and zero
// elsewhere.  The message is cut into pieces of piece_bytes (a multiple of 16, so a piece starts on a line of its slot);
// piece p is [p * piece_bytes, ...), and the table says where its gates and rows begin:
//   piece_gate[p]  the first gate whose row word is at or behind the piece's first byte
//   piece_row[p]   the first row with a byte at or behind it — a row across a piece boundary belongs to both pieces
// each with npieces + 1 entries, the last one ngates / nrows.
#pragma once

#include <cstdint>
#include <vector>

namespace gc {

struct YaoSkel {
    uint32_t keylen = 0, ng = 0, ngates = 0, nrows = 0;
    uint32_t at_tables = 0, at_labels = 0, len1 = 0;
    uint32_t piece_bytes = 0, npieces = 0;
    std::vector<uint32_t> words;  // len1 / 4 words as a little-endian host reads the message's bytes, zero-padded to a line
    std::vector<uint32_t> gate_off, row_off, piece_gate, piece_row;
};

constexpr uint32_t yao_be32(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }

// bytes of M1; 0 when they do not fit 32 bits (with room for a line behind them)
inline uint64_t yao_len1(uint32_t keylen, uint32_t ngates, uint32_t nrows, uint32_t ng) {
    const uint64_t n = 4 + (uint64_t)keylen + 4 + 4 * (uint64_t)ngates + 16 * (uint64_t)nrows + 16 * (uint64_t)ng;
    return n <= 0xffffffc0ull ? n : 0;
}

// row_of_gate: ngates + 1 entries, the first slab row of every gate and the slab's row count (Plan::row_of_gate)
inline YaoSkel yao_build_skel(const uint32_t *row_of_gate, uint32_t ngates, uint32_t keylen, uint32_t ng, uint32_t piece_bytes) {
    YaoSkel k;
    k.keylen = keylen, k.ng = ng, k.ngates = ngates, k.nrows = row_of_gate[ngates];
    k.at_tables = 4 + keylen;
    k.at_labels = k.at_tables + 4 + 4 * ngates + 16 * k.nrows;
    k.len1 = k.at_labels + 16 * ng;
    k.piece_bytes = piece_bytes;
    k.npieces = (k.len1 + piece_bytes - 1) / piece_bytes;
    k.words.assign(((size_t)k.len1 + 15) / 16 * 4, 0);
    k.words[0] = yao_be32(keylen);
    k.words[k.at_tables / 4] = yao_be32(ngates);
    k.gate_off.resize(ngates);
    k.row_off.resize(k.nrows);
    for (uint32_t g = 0; g < ngates; g++) {
        const uint32_t r0 = row_of_gate[g], n = row_of_gate[g + 1] - r0;
        k.gate_off[g] = k.at_tables + 4 + 4 * g + 16 * r0;
        k.words[k.gate_off[g] / 4] = yao_be32(n);
        for (uint32_t r = 0; r < n; r++) k.row_off[r0 + r] = k.gate_off[g] + 4 + 16 * r;
    }
    k.piece_gate.resize(k.npieces + 1);
    k.piece_row.resize(k.npieces + 1);
    uint32_t g = 0, r = 0;
    for (uint32_t p = 0; p < k.npieces; p++) {
        const uint64_t lo = (uint64_t)p * piece_bytes;
        while (g < ngates && k.gate_off[g] < lo) g++;
        while (r < k.nrows && (uint64_t)k.row_off[r] + 16 <= lo) r++;
        k.piece_gate[p] = g, k.piece_row[p] = r;
    }
    k.piece_gate[k.npieces] = ngates, k.piece_row[k.npieces] = k.nrows;
    return k;
}

}  // namespace gc
