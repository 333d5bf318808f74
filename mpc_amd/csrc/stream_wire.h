// stream_wire.h — the wire format of a streamed circuit's gates, once: what circuit/stream_garble.go:385-449
// writes and circuit/stream_evaluator.go:272-345 reads.  A gate is
//   one byte  op | flags: the low nibble is the operation, kTmpIn0 / kTmpIn1 / kTmpOut say that in0 / in1 / out is a tmp wire
//             of the block (else a global wire of the stream's store), kShortIds that every id of the gate has 16 bits;
//   2-3 ids   in0, in1 (not for INV), out — big-endian u16 or u32;
//   0-3 rows  of 16 bytes, BE(D0) || BE(D1).
// The writer side is host and device code (the serialiser kernels of stream_serialise.cpp, the skeleton of stream_batch.cpp);
// the reader side is host code that reads the PEER's bytes for both evaluators (stream_eval.cpp, stream_batch.cpp): every
// refusal in it is a security boundary.  No HIP dependency: tests/cpp/stream_wire_check.cpp compiles it with the host compiler.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/gcengine.h"

#if defined(__HIPCC__)
#define GCW_HD __host__ __device__
#else
#define GCW_HD
#endif

namespace gcw {

constexpr uint32_t kTmpIn0 = 0x80, kTmpIn1 = 0x40, kTmpOut = 0x20, kShortIds = 0x10, kOpMask = 0x0f;

// table rows and wire ids of a gate, by operation (XOR XNOR AND OR INV): {0, 0, 2, 3, 1} and {3, 3, 3, 3, 2}, a nibble each; any
// other operation counts as 0 rows and 3 ids (a reader refuses it, a writer's caller has checked its gates: GC_E_GATE)
GCW_HD inline uint32_t rows_of(uint32_t op) { return (0x00013200u >> (4 * (op < 7 ? op : 7))) & 15u; }
GCW_HD inline uint32_t wires_of(uint32_t op) { return (0x33323333u >> (4 * (op < 7 ? op : 7))) & 15u; }

// ---- writer ---------------------------------------------------------------------------------------------------------------
struct GateForm {  // one gate as it goes on the wire: its ids, its byte size, its op | flags byte
    uint32_t ai, bi, ci, size;
    uint8_t op, wc, rows, shortf;
};

// Gate (op, w0, w1 -> w2) of a circuit whose wires [0, first_tmp) are bound to the global wires in[] and [first_out, ...) to
// out[]: streaming Get / Set go through in[] first, then out[], else the wire is a tmp wire of the block under its own id
// (stream_garble.go:131-157).  16-bit ids if all of the gate's ids fit.
GCW_HD inline GateForm gate_form(uint32_t op, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t first_tmp, uint32_t first_out,
                                 const uint32_t *in, const uint32_t *out) {
    GateForm g{};
    uint32_t flags = op;
    auto get = [&](uint32_t w, uint32_t bit) -> uint32_t {
        if (w < first_tmp) return in[w];
        if (w >= first_out) return out[w - first_out];
        flags |= bit;
        return w;
    };
    g.bi = op != GC_INV ? get(w1, kTmpIn1) : 0;
    g.ai = get(w0, kTmpIn0);
    g.ci = get(w2, kTmpOut);
    g.wc = (uint8_t)wires_of(op), g.rows = (uint8_t)rows_of(op);
    g.shortf = g.ai <= 0xffff && g.bi <= 0xffff && g.ci <= 0xffff;
    g.op = (uint8_t)(flags | (g.shortf ? kShortIds : 0));
    g.size = 1 + (g.shortf ? 2u : 4u) * g.wc + 16u * g.rows;
    return g;
}

// the op byte and the ids at p; returns where the gate's first table row goes
GCW_HD inline uint8_t *put_gate_head(uint8_t *p, const GateForm &q) {
    *p++ = q.op;
    auto put = [&](uint32_t v) {
        if (!q.shortf) *p++ = (uint8_t)(v >> 24), *p++ = (uint8_t)(v >> 16);
        *p++ = (uint8_t)(v >> 8), *p++ = (uint8_t)v;
    };
    put(q.ai);
    if (q.wc == 3) put(q.bi);
    put(q.ci);
    return p;
}

// ---- reader (host) --------------------------------------------------------------------------------------------------------
struct GateView {  // one gate as read: where its fields are, not a copy of its rows
    uint8_t op, nw, rows;
    bool tmp0, tmp1, tmp_out, shortf;
    uint32_t w[3];           // in0, in1 (nw == 3), out: w[nw - 1]
    size_t id_off, row_off;  // byte offsets of the first id field and of the first row
};

// The gate at buf[*pos]; *pos moves behind it.  GC_E_ROWS: the bytes end inside the gate ("corrupted circuit"); GC_E_GATE:
// "invalid operation" — tested in the reference's order: op byte there, operation known, ids and rows there.
inline int read_gate(const uint8_t *buf, size_t len, size_t *pos, GateView *v) {
    size_t p = *pos;
    if (p >= len) return GC_E_ROWS;
    const uint8_t b = buf[p++];
    v->tmp0 = b & kTmpIn0, v->tmp1 = b & kTmpIn1, v->tmp_out = b & kTmpOut, v->shortf = b & kShortIds;
    v->op = b & kOpMask;
    if (v->op > GC_INV) return GC_E_GATE;
    v->nw = (uint8_t)wires_of(v->op), v->rows = (uint8_t)rows_of(v->op);
    const size_t idsz = v->shortf ? 2 : 4;
    if (idsz * v->nw + 16u * v->rows > len - p) return GC_E_ROWS;
    v->id_off = p;
    v->w[0] = v->w[1] = v->w[2] = 0;
    for (uint32_t i = 0; i < v->nw; i++, p += idsz)
        v->w[i] = v->shortf ? ((uint32_t)buf[p] << 8) | buf[p + 1]
                            : ((uint32_t)buf[p] << 24) | ((uint32_t)buf[p + 1] << 16) | ((uint32_t)buf[p + 2] << 8) | buf[p + 3];
    v->row_off = p;
    *pos = p + 16u * v->rows;
    return GC_OK;
}

// "Who wrote (tmp / global) wire idx last" as an array look-up under a generation stamp: generation << 32 | id, no clearing
// between blocks.
struct WireStamps {
    std::vector<uint64_t> last_t, last_w;
    uint32_t gen = 0;
    uint32_t next_gen() {  // a new generation: nothing stamped before it counts (after 2^32 of them the arrays start over)
        if (++gen == 0) {
            std::fill(last_t.begin(), last_t.end(), 0);
            std::fill(last_w.begin(), last_w.end(), 0);
            gen = 1;
        }
        return gen;
    }
    void touch_w(uint32_t idx) {  // (ids are sparse and mostly rising: half as much again, not one by one)
        if (idx >= last_w.size()) last_w.resize((size_t)idx + 1 + last_w.size() / 2, 0);
    }
};

// What a walk learns about the block's global wires (kept by the caller across blocks: no allocation per block).
struct BlockIo {
    std::vector<uint32_t> inputs, in_field;  // wires read before the block writes them, in order of first use; their field
    std::vector<uint64_t> writers;           // gate << 32 | wire of every gate that writes a global wire, in gate order
    std::vector<uint32_t> out_field;         // ... and the field that names the wire
};

// The gate loop of both evaluators over one OpCircuit block of the peer's (stream_evaluator.go:272-345), under a generation
// of its own.  An operand is named by the gate that wrote the wire IN THIS BLOCK; a global wire nobody has written yet is the
// block's k-th input, 0x80000000 | k.  A tmp wire is private to its block (stream_garble.go:131-157 gives every non-input,
// non-output wire of the circuit a tmp id, written by a gate before any gate reads it): a block that reads a tmp it has not
// written is refused instead of evaluated on a stale label.  Global ids must stay below the nwires of the block's own header
// (the reference indexes its store with them, stream_evaluator.go:29-96: an id beyond it panics there), tmp ids below ntmp:
// GC_E_ARG.  The caller has bounded ntmp and nwires (they size last_t / last_w).
// The sink (a template parameter, not a std::function: a block has ~10^5 gates) sees
//   uint32_t global_field(size_t byte_offset, bool is_short)   every id field that names a global wire, in stream order, once
//                                                              its id is known to be < nwires; returns its field number
//   void gate(uint32_t g, uint32_t in0, uint32_t in1, uint32_t op, bool writes_tmp)   (INV: in1 == in0)
//   void rows(size_t byte_offset, uint32_t n)                  the gate's n > 0 table rows
template <class Sink>
int walk_block(const uint8_t *buf, size_t len, uint32_t ngates, uint32_t ntmp, uint32_t nwires, WireStamps &st, BlockIo &io,
               Sink &sink, size_t *used) {
    if (st.last_t.size() < ntmp) st.last_t.resize(ntmp, 0);
    const uint64_t gen = st.next_gen(), stamp = gen << 32;
    io.inputs.clear(), io.in_field.clear(), io.writers.clear(), io.out_field.clear();
    size_t pos = 0;
    GateView v;
    for (uint32_t g = 0; g < ngates; g++) {
        int err = read_gate(buf, len, &pos, &v);
        if (err != GC_OK) return err;
        const size_t idsz = v.shortf ? 2 : 4;
        auto use = [&](bool tmp, uint32_t idx, uint32_t field) -> uint32_t {  // current id of a wire; bit 31: a block input
            if (tmp ? idx >= ntmp || (st.last_t[idx] >> 32) != gen : idx >= nwires) {
                err = GC_E_ARG;
                return 0;
            }
            if (tmp) return (uint32_t)st.last_t[idx];
            const uint32_t f = sink.global_field(v.id_off + idsz * field, v.shortf);
            st.touch_w(idx);
            if ((st.last_w[idx] >> 32) == gen) return (uint32_t)st.last_w[idx];
            const uint32_t id = 0x80000000u | (uint32_t)io.inputs.size();
            io.inputs.push_back(idx);
            io.in_field.push_back(f);
            st.last_w[idx] = stamp | id;
            return id;
        };
        const uint32_t in0 = use(v.tmp0, v.w[0], 0);
        const uint32_t in1 = v.nw == 3 ? use(v.tmp1, v.w[1], 1) : in0;
        if (err != GC_OK) return err;
        sink.gate(g, in0, in1, v.op, v.tmp_out);
        const uint32_t ci = v.w[v.nw - 1];
        if (v.tmp_out) {
            if (ci >= ntmp) return GC_E_ARG;
            st.last_t[ci] = stamp | g;
        } else {
            if (ci >= nwires) return GC_E_ARG;
            io.out_field.push_back(sink.global_field(v.id_off + idsz * (v.nw - 1u), v.shortf));
            st.touch_w(ci);
            st.last_w[ci] = stamp | g;
            io.writers.push_back(((uint64_t)g << 32) | ci);
        }
        if (v.rows) sink.rows(v.row_off, v.rows);
    }
    *used = pos;
    return GC_OK;
}

struct ParsedGate {  // a walked gate as a sink may keep it: operands as walk_block names them
    uint32_t in0, in1, op;
    bool writes_tmp;
};

// The walked gates (records with in0, in1, op; writes_tmp(record) says whether the gate writes a tmp wire) as a
// single-assignment gc_gate list.  Wire ids of the device circuit: [0, nin) the block's inputs, in order of first use; then
// one id per gate, first the gates that write a tmp wire, last the nout gates that write a global wire — those are the
// circuit's outputs and the only labels that leave it (streaming.Set, stream_evaluator.go:346-432).
template <class Parsed, class WritesTmp>
void ssa_gate_list(const std::vector<Parsed> &parsed, uint32_t nin, uint32_t nout, WritesTmp writes_tmp, std::vector<uint32_t> *id_of,
                   std::vector<gc_gate> *gates) {
    const uint32_t ngates = (uint32_t)parsed.size(), n_tmp = ngates - nout;
    id_of->resize(ngates);
    uint32_t kt = 0, kg = 0;
    for (uint32_t g = 0; g < ngates; g++) (*id_of)[g] = writes_tmp(parsed[g]) ? nin + kt++ : nin + n_tmp + kg++;
    auto fix = [&](uint32_t v) { return (v & 0x80000000u) ? (v & 0x7fffffffu) : (*id_of)[v]; };
    gates->assign(ngates, gc_gate{});
    for (uint32_t g = 0; g < ngates; g++) {
        gc_gate &q = (*gates)[g];
        q.in0 = fix(parsed[g].in0), q.in1 = parsed[g].op == GC_INV ? 0 : fix(parsed[g].in1);
        q.out = (*id_of)[g], q.op = (uint8_t)parsed[g].op;
    }
}

// Only the LAST gate of a block that writes a global wire stores it (streaming.Set in gate order, stream_evaluator.go:346-432:
// the last write wins): live[k] for io.writers[k], straight after the walk (its stamps are read).
inline void live_outputs(const WireStamps &st, const BlockIo &io, std::vector<uint8_t> *live) {
    live->resize(io.writers.size());
    for (size_t k = 0; k < io.writers.size(); k++)
        (*live)[k] = (uint32_t)st.last_w[(uint32_t)io.writers[k]] == (uint32_t)(io.writers[k] >> 32);
}

}  // namespace gcw
