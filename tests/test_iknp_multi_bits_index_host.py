"""CPU walk of the index arithmetic of bit-COT over the multi-session IKNP handle (mpc_amd/csrc/iknp_multi_bits.h on top of
iknp_multi.h).  The headers are compiled into a stand-alone C++ program with the host compiler under AddressSanitizer and
UBSan; the program walks a launch of each kernel the way the kernel does (workgroup, step or trip, item or lane) and writes
records of what would be read and written.  They are compared with a model written from the reference's two loops
(ReceiveBits, ot/iknp.go:566-613; SendBits, :265-307), run once per session:

  * every result word is written exactly once by either kernel, with exactly the bits the reference can set;
  * every byte of the receiver's u is written exactly once, where the reference's chunks put it;
  * the receiver reads the choice words the reference reads (whole words only) and none outside a session's W words;
  * the sender's stream bytes are pos + j, its u reads are the column-0 bytes the reference XORs and nothing else, in the
    message layout and in the packed column-0 copy of the host form;
  * nothing lies outside an array.

per covers values that are no multiple of 8, of 64 and of 512, positions on and off a block boundary, every stride form,
and S past one trip of both capped grids."""
import os
import subprocess

import numpy as np
import pytest

from tests.util import kernel_constants

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpc_amd", "csrc")
GRID, RECV_ITEMS, SEND_THREADS, SEND_GRID = kernel_constants("kIknpMultiGrid", "kIknpRecvChunks", "kIknpBitsSendThreads",
                                                             "kIknpBitsSendGrid")

PERS = [1, 7, 8, 37, 63, 64, 65, 100, 127, 128, 129, 500, 511, 512, 513, 549, 576, 1024, 1030]


def W(per):
    return -(-per // 64)


CASES = [(S, per, pos, stride) for S in (1, 3) for per in PERS for pos, stride in ((0, 0), (5, W(per)), (93, W(per) + 3))]
CASES += [(3, per, pos, 0) for per in (37, 549) for pos in (12, 16, 19, 24)]
CASES += [(GRID * RECV_ITEMS // 2 + 1, 549, 3, 0)]                  # the receiver's workgroup 0 gets a second, ragged step
CASES += [(SEND_GRID * SEND_THREADS // 5 + 1, 549, 3, 9)]           # ... and the sender's (5 lanes per session)
CASES += [(SEND_GRID * SEND_THREADS + 1, 37, 0, 0)]                 # ... with one lane per session

PROGRAM = r"""
#include <algorithm>
#include <cstdio>
#include <vector>

#include "iknp_multi_bits.h"

using namespace gc;

// argv[1]: output file.  "S per pos stride grid nch sthreads sgrid" on stdin, one pair of launches per line -> a header
// record {S, per, pos, stride, records, 0} and records of six words:
//   {0, session, chunk, u_off, byte_rows, stream_pos}        an item of the receiver (its 128 columns follow each other)
//   {1, result word, mask, 0, 0, 0}                          a result word the receiver stores
//   {2, choice word, session, 0, 0, 0}                       a choice word the receiver loads
//   {3, session, word, words, nbytes, stream_pos}            a lane of the sender
//   {4, session, u_off in the message, u_off in the packed copy, blocks, 0}
//   {5, result word, mask, 0, 0, 0}                          a result word the sender stores
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "wb");
    if (!f) return 2;
    unsigned long long S, per, pos, stride, cap, nch, sthreads, sgrid;
    while (std::scanf("%llu %llu %llu %llu %llu %llu %llu %llu", &S, &per, &pos, &stride, &cap, &nch, &sthreads, &sgrid) == 8) {
        if (!iknp_bits_stride_ok(stride, per)) return 3;
        const uint64_t Wd = iknp_bits_words(per);  // a stride in (0, W) is refused, W and above are not
        if ((Wd > 1 && iknp_bits_stride_ok(Wd - 1, per)) || !iknp_bits_stride_ok(Wd, per) || !iknp_bits_stride_ok(0, per)) return 3;
        if (iknp_bits_choice_span(S, per, stride) != (S - 1) * stride + Wd) return 3;
        std::vector<uint64_t> rec;
        auto put = [&](uint64_t a, uint64_t b, uint64_t c, uint64_t d, uint64_t e, uint64_t g) {
            const uint64_t r[6] = {a, b, c, d, e, g};
            rec.insert(rec.end(), r, r + 6);
        };
        // k_iknp_multi_recv_bits
        const uint64_t items = iknp_multi_items(S, per), steps = iknp_multi_steps(items, (uint32_t)nch);
        const uint64_t grid = std::min<uint64_t>(steps, cap);
        for (uint64_t b = 0; b < grid; b++)
            for (uint64_t step = b; step < steps; step += grid)
                for (uint64_t cig = 0; cig < nch; cig++) {
                    const uint64_t it = step * nch + cig;
                    if (it >= items) continue;
                    const IknpMultiItem m = iknp_multi_item(it, per, pos);
                    const IknpBitsItem bi = iknp_bits_item(m, per, stride);
                    put(0, m.session, m.chunk, m.u_off, m.byte_rows, m.stream_pos);
                    for (uint32_t w = 0; w < 8; w++)
                        if (w < bi.result_words) put(1, bi.result_word + w, iknp_bits_word_mask(per, 8 * m.chunk + w), 0, 0, 0);
                    for (uint32_t q = 0; q < (m.byte_rows + 15) / 16; q++)
                        for (uint32_t k = 2 * q; k < 2 * q + 2; k++)
                            if (k < bi.choice_words) put(2, bi.choice_word + k, m.session, 0, 0, 0);
                }
        // k_iknp_multi_send_bits
        const uint64_t lanes = iknp_bits_send_lanes(S, per);
        const uint64_t sg = std::min<uint64_t>((lanes + sthreads - 1) / sthreads, sgrid);
        for (uint64_t b = 0; b < sg; b++)
            for (uint64_t t = 0; t < sthreads; t++)
                for (uint64_t g = b * sthreads + t; g < lanes; g += sg * sthreads) {
                    const IknpBitsLane n = iknp_bits_send_lane(g, per, pos, iknp_multi_u_bytes(per), 8192);
                    const IknpBitsLane p = iknp_bits_send_lane(g, per, pos, iknp_bits_col0_row(per), 64);
                    if (p.session != n.session || p.word != n.word || p.nbytes != n.nbytes || p.blocks != n.blocks) return 3;
                    put(3, n.session, n.word, n.words, n.nbytes, n.stream_pos);
                    put(4, n.session, n.u_off, p.u_off, n.blocks, 0);
                    for (uint32_t k = 0; k < n.words; k++)
                        put(5, n.session * Wd + n.word + k, iknp_bits_word_mask(per, n.word + k), 0, 0, 0);
                }
        const uint64_t head[6] = {S, per, pos, stride, rec.size() / 6, 0};
        std::fwrite(head, sizeof head, 1, f);
        if (!rec.empty()) std::fwrite(rec.data(), 8, rec.size(), f);
    }
    return std::fclose(f) == 0 ? 0 : 2;
}
"""


@pytest.fixture(scope="module")
def walks(tmp_path_factory):
    d = tmp_path_factory.mktemp("iknp_multi_bits_index")
    src, exe, out = d / "bits_walk.cpp", d / "bits_walk", d / "walk.bin"
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = "".join("%d %d %d %d %d %d %d %d\n" % (c + (GRID, RECV_ITEMS, SEND_THREADS, SEND_GRID)) for c in CASES)
    r = subprocess.run([str(exe), str(out)], input=lines, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    raw = np.fromfile(str(out), np.uint64).reshape(-1, 6)
    res, k = {}, 0
    for case in CASES:
        head = [int(v) for v in raw[k]]
        assert tuple(head[:4]) == case
        res[case] = raw[k + 1:k + 1 + head[4]]
        k += 1 + head[4]
    assert k == len(raw)
    return res


def u_bytes(per):
    return (per // 512) * 8192 + ((per % 512 + 7) // 8) * 128


def go_session(per, pos):
    """both loops for ONE session (they walk the same chunks): per chunk (ofs, rows, byteRows, bytes of u before it, stream
    position), the choice words ReceiveBits reads, the bits of every result word it can set, and per result byte the stream
    byte and the u byte SendBits combines"""
    chunks, choice, mask = [], [], np.zeros(W(per), np.uint64)
    stream, ubyte = [], []
    ofs, u_at, p = 0, 0, pos
    while ofs < per:
        rows = min(512, per - ofs)
        byte_rows = (rows + 7) // 8
        chunks.append((ofs, rows, byte_rows, u_at, p))
        choice += [ofs // 64 + w for w in range(byte_rows // 8)]  # wordOffset + w, w < words (iknp.go:577-592)
        for row in range(rows):                                   # :605-610, :295-304
            idx = ofs + row
            mask[idx // 64] |= np.uint64(1) << np.uint64(idx % 64)
        stream += [p + j for j in range(byte_rows)]               # prg(g0[0], t[0:byteRows]) (:281)
        ubyte += [u_at + j for j in range(byte_rows)]             # xor(t[0:byteRows], chunk[0:]) (:283)
        u_at += 128 * byte_rows                                   # len(chunk) = K * byteRows (:274, :597)
        p += byte_rows
        ofs += rows
    assert u_at == u_bytes(per) and len(stream) == (per + 7) // 8
    return chunks, choice, mask, np.array(stream, np.uint64), np.array(ubyte, np.uint64)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "S%d-per%d-pos%d-stride%d" % c)
def test_both_walks_against_the_reference_loops(walks, case):
    S, per, pos, stride = case
    rec = walks[case]
    Wd, ub = W(per), u_bytes(per)
    chunks, choice, mask, stream, ubyte = go_session(per, pos)
    sess = np.arange(S, dtype=np.uint64)
    kind = rec[:, 0]

    # ---- receiver ----
    items = rec[kind == 0]
    order = np.lexsort((items[:, 2], items[:, 1]))
    want = np.array([(0, s, c, s * ub + ch[3], ch[2], ch[4]) for s in range(S) for c, ch in enumerate(chunks)], np.uint64)
    assert (items[order] == want).all(), "an item is missing, doubled or misplaced"
    # u: an item's columns are col * byte_rows behind u_off, so it covers [u_off, u_off + 128 * byte_rows): together the
    # items tile [0, S * ub) without gap or overlap
    it = items[order]
    ends = it[:, 3] + np.uint64(128) * it[:, 4]
    assert it[0, 3] == 0 and (it[1:, 3] == ends[:-1]).all() and ends[-1] == S * ub
    words = rec[kind == 1]
    o = np.argsort(words[:, 1], kind="stable")
    assert (words[o, 1] == np.arange(S * Wd, dtype=np.uint64)).all(), "a result word is unwritten or written twice"
    assert (words[o, 2] == np.tile(mask, S)).all(), "tail bits"
    reads = rec[kind == 2]
    want_reads = (sess[:, None] * np.uint64(stride) + np.array(choice, np.uint64)[None, :]).reshape(-1)
    assert sorted(reads[:, 1].tolist()) == sorted(want_reads.tolist()), "the choice words that enter u"
    if len(reads):
        local = reads[:, 1] - reads[:, 2] * np.uint64(stride)
        assert (local < Wd).all() and reads[:, 1].max() < (S - 1) * stride + Wd, "a choice word outside the session's W words"

    # ---- sender ----
    lanes, us, swords = rec[kind == 3], rec[kind == 4], rec[kind == 5]
    assert len(lanes) == len(us) == S * ((Wd + 1) // 2)
    o = np.argsort(swords[:, 1], kind="stable")
    assert (swords[o, 1] == np.arange(S * Wd, dtype=np.uint64)).all(), "a result word is unwritten or written twice"
    assert (swords[o, 2] == np.tile(mask, S)).all(), "tail bits"
    nbytes_total = (per + 7) // 8
    row = (nbytes_total + 15) // 16 * 16
    got_stream = np.full((S, nbytes_total), -1, np.int64)
    got_u = np.full((S, nbytes_total), -1, np.int64)
    got_packed = np.full((S, nbytes_total), -1, np.int64)
    for (_, s, word, nwords, nb, sp), (_, s2, uo, po, blocks, _) in zip(lanes.tolist(), us.tolist()):
        assert s == s2 and 1 <= nb <= 16 and 1 <= nwords <= 2 and word + nwords <= Wd
        j0 = 8 * word
        assert (got_stream[s, j0:j0 + nb] == -1).all(), "two lanes make one result byte"
        got_stream[s, j0:j0 + nb] = np.arange(sp, sp + nb)
        got_u[s, j0:j0 + nb] = np.arange(uo, uo + nb)
        got_packed[s, j0:j0 + nb] = np.arange(po, po + nb)
        assert blocks == (sp + nb - 1) // 16 - sp // 16 + 1, "the AES blocks that hold the lane's bytes"
        assert uo % 16 == 0 and po % 16 == 0, "a full lane loads its u bytes as one 16-byte word"
        assert nb == 16 or j0 + nb == nbytes_total, "only the last lane of a session is short"
    assert (got_stream == stream[None, :].astype(np.int64)).all(), "result byte j is stream byte pos + j"
    assert (got_u == (sess[:, None] * np.uint64(ub) + ubyte[None, :]).astype(np.int64)).all(), "u reads: column 0 only"
    assert got_u.max() < S * ub
    assert (got_packed == (sess[:, None] * np.uint64(row) + np.arange(nbytes_total, dtype=np.uint64)[None, :]).astype(np.int64)).all()
    assert got_packed.max() < S * row

