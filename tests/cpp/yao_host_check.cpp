// yao_host_check.cpp — the host side of gc_yao_* on the CPU (tests/test_yao_layout.py), compiled with the host compiler from
// the engine's own headers mpc_amd/csrc/yao_skel.h and yao_m3.h.
//
//   yao_host_check pieces <keylen> <ng> <piece_bytes> <file>     file: row_of_gate, ngates + 1 little-endian u32
//     builds the skeleton and walks the piece table as k_yao_m1_out does: per piece the row words of gates
//     [piece_gate[p], piece_gate[p + 1]) and the bytes inside the piece of rows [piece_row[p], piece_row[p + 1] + 1) that begin
//     before its end.  Prints the geometry, every piece, how often a byte of the table section was covered (min, max), the
//     rows that lie across a piece boundary, and the skeleton's bytes.
//   yao_host_check m3            stdin: "pack <nout> <hex bits>" / "parse <nout> <room> <hex message>" lines
//     prints "<len> <hex message>" / "<ok> <hex bits>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "yao_m3.h"
#include "yao_skel.h"

static std::vector<uint8_t> unhex(const char *s) {
    std::vector<uint8_t> out;
    if (!std::strcmp(s, "-")) return out;
    for (size_t i = 0; s[i] && s[i + 1]; i += 2) {
        char b[3] = {s[i], s[i + 1], 0};
        out.push_back((uint8_t)std::strtoul(b, nullptr, 16));
    }
    return out;
}

static void hex(const uint8_t *p, size_t n) {
    if (!n) std::printf("-");
    for (size_t i = 0; i < n; i++) std::printf("%02x", p[i]);
}

static int pieces(int argc, char **argv) {
    if (argc != 6) return 2;
    const uint32_t keylen = (uint32_t)std::atoi(argv[2]), ng = (uint32_t)std::atoi(argv[3]), piece = (uint32_t)std::atoi(argv[4]);
    std::FILE *f = std::fopen(argv[5], "rb");
    if (!f) return 2;
    std::vector<uint32_t> rog;
    uint32_t v;
    while (std::fread(&v, 4, 1, f) == 1) rog.push_back(v);
    std::fclose(f);
    if (rog.empty()) return 2;
    const uint32_t ngates = (uint32_t)rog.size() - 1;
    if (!gc::yao_len1(keylen, ngates, rog[ngates], ng)) return 3;
    const gc::YaoSkel k = gc::yao_build_skel(rog.data(), ngates, keylen, ng, piece);
    std::printf("geom %u %u %u %u %u\n", k.len1, k.at_tables, k.at_labels, k.npieces, k.piece_bytes);
    std::vector<uint8_t> cover(k.len1, 0);
    uint32_t across = 0;
    for (uint32_t p = 0; p < k.npieces; p++) {
        const uint32_t lo = p * piece, hi = lo + piece < k.len1 ? lo + piece : k.len1;
        std::printf("piece %u %u %u %u %u\n", p, lo, hi, k.piece_gate[p], k.piece_row[p]);
        for (uint32_t g = k.piece_gate[p]; g < k.piece_gate[p + 1]; g++) {
            const uint32_t off = k.gate_off[g];
            if (off < lo || off + 4 > hi) {
                std::printf("bad gate %u of piece %u lies outside it\n", g, p);
                return 1;
            }
            for (uint32_t b = 0; b < 4; b++) cover[off + b]++;
        }
        const uint32_t r1 = k.piece_row[p + 1] + 1 < k.nrows ? k.piece_row[p + 1] + 1 : k.nrows;
        for (uint32_t r = k.piece_row[p]; r < r1; r++) {
            const uint32_t off = k.row_off[r];
            if (off >= hi) continue;
            if (off + 16 <= lo) {
                std::printf("bad row %u of piece %u ends before it\n", r, p);
                return 1;
            }
            if (off + 16 > hi) across++;
            for (uint32_t b = 0; b < 16; b++)
                if (off + b >= lo && off + b < hi) cover[off + b]++;
        }
    }
    uint32_t mn = 255, mx = 0;
    for (uint32_t b = k.at_tables + 4; b < k.at_labels; b++) {
        if (cover[b] < mn) mn = cover[b];
        if (cover[b] > mx) mx = cover[b];
    }
    uint32_t outside = 0;
    for (uint32_t b = 0; b < k.len1; b++)
        if ((b < k.at_tables + 4 || b >= k.at_labels) && cover[b]) outside++;
    std::printf("cover %u %u %u %u\n", mn, mx, across, outside);
    std::printf("skel ");
    hex((const uint8_t *)k.words.data(), k.len1);
    std::printf("\n");
    return 0;
}

static int m3() {
    char line[1 << 16];
    while (std::fgets(line, sizeof line, stdin)) {
        char what[16], a[1 << 15];
        unsigned nout = 0, room = 0;
        if (std::sscanf(line, "%15s", what) != 1) continue;
        if (!std::strcmp(what, "pack")) {
            if (std::sscanf(line, "%*s %u %32767s", &nout, a) != 2) return 2;
            std::vector<uint8_t> bits = unhex(a), out(gc::yao_m3_slot_bytes(nout), 0xEE);
            if (bits.size() != gc::yao_m3_bits_bytes(nout)) return 2;
            const uint32_t n = gc::yao_m3_pack(bits.data(), nout, out.data());
            std::printf("%u ", n);
            hex(out.data(), n);
            std::printf("\n");
        } else if (!std::strcmp(what, "parse")) {
            if (std::sscanf(line, "%*s %u %u %32767s", &nout, &room, a) != 3) return 2;
            std::vector<uint8_t> msg = unhex(a), bits(gc::yao_m3_bits_bytes(nout), 0xEE);
            msg.resize(room > msg.size() ? room : msg.size(), 0);
            const bool ok = gc::yao_m3_parse(msg.data(), room, nout, bits.data());
            std::printf("%d ", ok ? 1 : 0);
            hex(bits.data(), ok ? bits.size() : 0);
            std::printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "pieces")) return pieces(argc, argv);
    if (argc == 2 && !std::strcmp(argv[1], "m3")) return m3();
    return 2;
}
