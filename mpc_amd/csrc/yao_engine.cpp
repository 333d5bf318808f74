// yao_engine.cpp — C ABI of circuit.Garbler's / circuit.Evaluator's messages for S sessions per call (gcengine.h: gc_yao_*;
// DESIGN.md §23; circuit/garbler.go:38-180, circuit/evaluator.go:20-157, p2p/protocol.go:216-261).  A call is a fixed
// sequence of launches on the ctx stream: the keyed batch pass the library has already (gc_batch_garble_keyed /
// _eval_keyed), the gathers, and the kernels of yao_kernels.hip, which build and read the messages.  A handle owns its batch,
// the skeleton of M1 and every array a call needs, so a _dev call allocates nothing and waits for nothing.  The host forms
// stage packed messages through host_staging.h and run the _dev sequence on the staged copies.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <memory>
#include <new>

#include "engine.h"
#include "sha2pc.h"  // launch_s2_repack
#include "yao.h"
#include "yao_skel.h"

using namespace gc;

namespace {

int refuse(const char *what) {
    std::snprintf(gc::tls_error, sizeof gc::tls_error, "gc_yao: %s", what);
    return GC_E_ARG;
}

int done(hipError_t e) {
    GC_HIP(e);
    return GC_OK;
}

size_t slot_stride(size_t len) { return (len + 15) / 16 * 16; }

// sessions per workgroup and bytes per piece of the M1 kernels: yao.h's, or GC_YAO_TILE / GC_YAO_PIECE (developer aids)
int kernel_shape(uint32_t *tile, uint32_t *piece) {
    *tile = kYaoTile, *piece = kYaoPieceBytes;
    if (const char *e = std::getenv("GC_YAO_TILE")) *tile = (uint32_t)std::strtoul(e, nullptr, 10);
    if (const char *e = std::getenv("GC_YAO_PIECE")) *piece = (uint32_t)std::strtoul(e, nullptr, 10);
    const bool tile_ok = *tile == 4 || *tile == 8 || *tile == 16 || *tile == 32 || *tile == 64;
    if (!tile_ok || *piece < 64 || *piece > 16384 || (*piece & 15) || yao_m1_lds_bytes(*tile, *piece) > 160 * 1024)
        return refuse("GC_YAO_TILE is not 4, 8, 16, 32 or 64, GC_YAO_PIECE no multiple of 16 in 64 .. 16384, or their LDS is past 160 KiB");
    return GC_OK;
}

// the geometry of a handle; GC_E_KEYSIZE, or GC_E_ARG with a text for what create refuses
int geometry(const gc_plan_info &info, uint32_t ng, uint32_t ne, size_t keylen, size_t S, YaoGeom *g) {
    if (keylen != 16 && keylen != 24 && keylen != 32) return GC_E_KEYSIZE;
    if ((uint64_t)ng + ne != info.ninputs) return refuse("ng + ne is not the circuit's input count");
    if (ne == 0 || info.noutputs == 0) return refuse("a circuit without evaluator inputs or without outputs");
    const uint64_t len1 = yao_len1((uint32_t)keylen, info.ngates, info.slab_rows, ng);
    if (!len1) return refuse("the first message does not fit 32 bits");
    g->ng = ng, g->ne = ne, g->nout = info.noutputs, g->ngates = info.ngates, g->rows = info.slab_rows;
    g->keylen = (uint32_t)keylen, g->len1 = (uint32_t)len1, g->S = S;
    // the largest arrays around a handle: S slots of M1, S * ne wires, S slots of M2
    const size_t per = slot_stride(len1) + 32 * (size_t)ne + 16 * (size_t)info.noutputs + 64;
    if (S > UINT32_MAX || (S && per > SIZE_MAX / S)) return refuse("a size does not fit size_t");
    return GC_OK;
}

int layout(const gc_plan_info &info, uint32_t ng, uint32_t ne, size_t keylen, size_t len[3]) {
    YaoGeom g;
    const int rc = geometry(info, ng, ne, keylen, 1, &g);
    if (rc != GC_OK) return rc;
    if (len) len[0] = g.len1, len[1] = g.len2(), len[2] = g.slot3();
    return GC_OK;
}

template <class T>
int dev_alloc(T **p, size_t bytes) {
    GC_HIP(hipMalloc((void **)p, bytes ? bytes : 16));
    return GC_OK;
}

template <class T>
int dev_upload(T **p, const std::vector<T> &v) {
    const int rc = dev_alloc(p, v.size() * sizeof(T));
    if (rc != GC_OK) return rc;
    if (!v.empty()) GC_HIP(hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return GC_OK;
}

// what both handles are made of
struct Core {
    gc_ctx *ctx = nullptr;
    gc_batch *batch = nullptr;
    YaoGeom g{};
    YaoDev d{};
    uint32_t *d_skel = nullptr, *d_gate_off = nullptr, *d_row_off = nullptr, *d_piece_gate = nullptr, *d_piece_row = nullptr;
    uint32_t *d_badidx = nullptr;  // evaluator: [S] lowest failing check of accept
    uint32_t *d_kept = nullptr;    // evaluator: [S] accept's verdicts, until the next accept
    uint32_t *d_keys = nullptr;    // evaluator: [S][keylen] bytes
    ~Core() {
        if (!ctx) return;
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);  // a _dev call may still use the arrays
        for (uint32_t *p : {d_skel, d_gate_off, d_row_off, d_piece_gate, d_piece_row, d_badidx, d_kept, d_keys})
            if (p) (void)hipFree(p);
        if (batch) gc_batch_free(batch);
    }
};

int core_init(Core *h, gc_ctx *ctx, gc_circ *circ, uint32_t ng, uint32_t ne, size_t keylen, size_t S, bool garbler) {
    if (!ctx || !circ || circ->ctx != ctx || S == 0 || ctx->capturing) return GC_E_ARG;
    int rc = geometry(circ->plan.p.info, ng, ne, keylen, S, &h->g);
    if (rc != GC_OK) return rc;
    uint32_t tile, piece;
    rc = kernel_shape(&tile, &piece);
    if (rc != GC_OK) return rc;
    h->ctx = ctx;
    h->batch = gc_batch_create(circ, (uint32_t)S, &rc);
    if (!h->batch) return rc;
    if (h->batch->schedule != 1) rc = gc_batch_set_schedule(h->batch, 1);
    if (rc != GC_OK) return rc;
    if (!gc_batch_keyed_supported(h->batch)) return refuse("gc_batch_keyed_supported is 0 for a batch of S instances of this circuit");
    GC_HIP(hipSetDevice(ctx->device));
    // the keyed passes' expanded keys, which the batch would allocate at its first keyed pass
    if (!h->batch->d_keyed_rk) rc = dev_alloc(&h->batch->d_keyed_rk, S * 60 * sizeof(uint32_t));
    const YaoSkel k = yao_build_skel(circ->plan.p.row_of_gate.data(), h->g.ngates, h->g.keylen, ng, piece);
    if (rc == GC_OK) rc = dev_upload(&h->d_skel, k.words);
    if (rc == GC_OK) rc = dev_upload(&h->d_gate_off, k.gate_off);
    if (rc == GC_OK) rc = dev_upload(&h->d_row_off, k.row_off);
    if (rc == GC_OK) rc = dev_upload(&h->d_piece_gate, k.piece_gate);
    if (rc == GC_OK) rc = dev_upload(&h->d_piece_row, k.piece_row);
    if (rc == GC_OK && !garbler) rc = dev_alloc(&h->d_badidx, S * sizeof(uint32_t));
    if (rc == GC_OK && !garbler) rc = dev_alloc(&h->d_kept, S * sizeof(uint32_t));
    if (rc == GC_OK && !garbler) rc = dev_alloc(&h->d_keys, S * keylen);
    if (rc != GC_OK) return rc;
    if (!garbler) GC_HIP(hipMemset(h->d_kept, 0, S * sizeof(uint32_t)));
    h->d = YaoDev{(const uint4 *)h->d_skel, h->d_gate_off, h->d_row_off, h->d_piece_gate, h->d_piece_row, k.ngates, k.nrows,
                  k.keylen, k.ng, k.at_tables, k.at_labels, k.len1, k.piece_bytes, k.npieces, tile};
    return GC_OK;
}

bool slots_ok(const void *d, size_t stride, size_t len) {
    return d && (stride & 15) == 0 && stride >= len && ((uintptr_t)d & 15) == 0;
}

// ---- the calls on device pointers: what a _dev form does behind its checks -------------------------------------------------

int send_run(Core *h, const void *d_keys, const void *d_rnd, const void *d_bits, void *d_m1, size_t stride1) {
    const int rc = gc_batch_garble_keyed(h->batch, d_keys, h->g.keylen, d_rnd);
    if (rc != GC_OK) return rc;
    const gc_batch *b = h->batch;
    return done(launch_yao_m1_out(h->d, b->d_T, b->g.lt, b->d_W, b->g.lw, b->d_R, (const uint32_t *)d_keys, (const uint8_t *)d_bits,
                                  (uint8_t *)d_m1, stride1, (uint32_t)h->g.S, h->ctx->stream));
}

int garbler_result_run(Core *h, const void *d_m2, size_t stride2, void *d_m3, size_t stride3, void *d_len3, void *d_bits_out,
                       void *d_verdict) {
    const gc_batch *b = h->batch;
    return done(launch_yao_m2_decode(h->g, b->d_W, b->g.lw, b->circ->d_out_slots, b->d_R, (const uint8_t *)d_m2, stride2,
                                     (uint8_t *)d_m3, stride3, (uint32_t *)d_len3, (uint8_t *)d_bits_out, (uint32_t *)d_verdict,
                                     h->ctx->stream));
}

int accept_run(Core *h, const void *d_m1, size_t stride1, void *d_verdict) {
    gc_batch *b = h->batch;
    hipStream_t st = h->ctx->stream;
    const uint32_t S = (uint32_t)h->g.S;
    GC_HIP(hipMemsetAsync(h->d_badidx, 0xff, S * sizeof(uint32_t), st));
    GC_HIP(launch_yao_m1_in(h->d, b->d_T, b->g.lt, b->d_W, b->g.lw, h->d_keys, (const uint8_t *)d_m1, stride1, S, h->d_badidx, st));
    return done(launch_yao_m1_verdict(S, h->d_badidx, (uint32_t *)d_verdict, h->d_kept, st));
}

int eval_run(Core *h, const void *d_labels, void *d_m2, size_t stride2, void *d_verdict) {
    gc_batch *b = h->batch;
    int rc = gc_batch_set_input_range(b, h->g.ng, h->g.ne, d_labels);
    if (rc == GC_OK) rc = gc_batch_eval_keyed(b, h->d_keys, h->g.keylen, b);
    if (rc != GC_OK) return rc;
    return done(launch_yao_m2_out(h->g, b->d_W, b->g.lw, b->circ->d_out_slots, h->d_kept, (uint8_t *)d_m2, stride2,
                                  (uint32_t *)d_verdict, h->ctx->stream));
}

int evaluator_result_run(Core *h, const void *d_m3, size_t stride3, void *d_bits_out, void *d_verdict) {
    return done(launch_yao_m3_parse(h->g, (const uint8_t *)d_m3, stride3, (uint8_t *)d_bits_out, (uint32_t *)d_verdict, h->ctx->stream));
}

// ---- host forms ------------------------------------------------------------------------------------------------------------

// the verdicts of a host form -> its return code: that of the lowest bad session
int verdict_code(const uint32_t *v, size_t S, uint32_t *verdict_out, size_t *bad_session) {
    if (verdict_out) std::memcpy(verdict_out, v, S * sizeof(uint32_t));
    for (size_t s = 0; s < S; s++) {
        if (!v[s]) continue;
        if (bad_session) *bad_session = s;
        const uint32_t code = v[s] & 0xffu;
        return code == kYaoGates || code == kYaoRows ? GC_E_ROWS : GC_E_ARG;
    }
    return GC_OK;
}

// a Staged that is device memory alone: the slots of a message array
Staged slots(size_t bytes) { return Staged{nullptr, nullptr, 0, bytes}; }

int repack(size_t S, const void *src, size_t src_stride, void *dst, size_t dst_stride, size_t len, hipStream_t st) {
    launch_s2_repack(S, (const uint8_t *)src, src_stride, (uint8_t *)dst, dst_stride, len, st);
    GC_HIP(hipGetLastError());
    return GC_OK;
}

// a host form begins: the handle's ctx, not inside a capture
int host_begin(Core *c) {
    if (c->ctx->capturing) return GC_E_ARG;
    GC_HIP(hipSetDevice(c->ctx->device));
    return GC_OK;
}

}  // namespace

struct gc_yao_garbler {
    Core c;
};
struct gc_yao_evaluator {
    Core c;
};

namespace {

template <class H>
H *create(gc_ctx *ctx, gc_circ *circ, uint32_t ng, uint32_t ne, size_t keylen, size_t S, bool garbler, int *status) try {
    std::unique_ptr<H> h(new H);
    const int rc = core_init(&h->c, ctx, circ, ng, ne, keylen, S, garbler);
    if (status) *status = rc;
    return rc == GC_OK ? h.release() : nullptr;
} catch (...) {
    const int rc__ = gc::on_exception();
    if (status) *status = rc__;
    return nullptr;
}

}  // namespace

extern "C" {

gc_yao_garbler *gc_yao_garbler_create(gc_ctx *ctx, gc_circ *circ, uint32_t ng, uint32_t ne, size_t keylen, size_t S, int *status) {
    return create<gc_yao_garbler>(ctx, circ, ng, ne, keylen, S, true, status);
}
gc_yao_evaluator *gc_yao_evaluator_create(gc_ctx *ctx, gc_circ *circ, uint32_t ng, uint32_t ne, size_t keylen, size_t S,
                                          int *status) {
    return create<gc_yao_evaluator>(ctx, circ, ng, ne, keylen, S, false, status);
}
void gc_yao_garbler_free(gc_yao_garbler *h) { delete h; }
void gc_yao_evaluator_free(gc_yao_evaluator *h) { delete h; }

int gc_yao_layout_plan(const gc_plan *plan, uint32_t ng, uint32_t ne, size_t keylen, size_t len[3]) {
    return plan ? layout(plan->p.info, ng, ne, keylen, len) : GC_E_ARG;
}
int gc_yao_layout(const gc_circ *circ, uint32_t ng, uint32_t ne, size_t keylen, size_t len[3]) {
    return circ ? layout(circ->plan.p.info, ng, ne, keylen, len) : GC_E_ARG;
}
int gc_yao_kernel_shape(uint32_t *session_tile, uint32_t *piece_bytes) {
    uint32_t tile, piece;
    const int rc = kernel_shape(&tile, &piece);
    if (rc != GC_OK) return rc;
    if (session_tile) *session_tile = tile;
    if (piece_bytes) *piece_bytes = piece;
    return GC_OK;
}

gc_batch *gc_yao_garbler_batch(gc_yao_garbler *h) { return h ? h->c.batch : nullptr; }
gc_batch *gc_yao_evaluator_batch(gc_yao_evaluator *h) { return h ? h->c.batch : nullptr; }

int gc_yao_garbler_send_dev(gc_yao_garbler *h, const void *d_keys, const void *d_rnd, const void *d_bits, void *d_m1_out,
                            size_t stride1) try {
    if (!h || !d_keys || ((uintptr_t)d_keys & 3) || !d_rnd || (!d_bits && h->c.g.ng) || !slots_ok(d_m1_out, stride1, h->c.g.len1))
        return GC_E_ARG;
    GC_HIP(hipSetDevice(h->c.ctx->device));
    return send_run(&h->c, d_keys, d_rnd, d_bits, d_m1_out, stride1);
} catch (...) {
    return gc::on_exception();
}

int gc_yao_garbler_ot_wires_dev(gc_yao_garbler *h, void *d_wires_out) try {
    if (!h || !d_wires_out) return GC_E_ARG;
    return gc_batch_gather_input_wires(h->c.batch, h->c.g.ng, h->c.g.ne, d_wires_out);
} catch (...) {
    return gc::on_exception();
}

int gc_yao_garbler_result_dev(gc_yao_garbler *h, const void *d_m2, size_t stride2, void *d_m3_out, size_t stride3,
                              void *d_len3_out, void *d_bits_out, void *d_verdict) try {
    if (!h || !d_len3_out || !d_bits_out || !d_verdict || !slots_ok(d_m2, stride2, h->c.g.len2()) ||
        !slots_ok(d_m3_out, stride3, h->c.g.slot3()))
        return GC_E_ARG;
    GC_HIP(hipSetDevice(h->c.ctx->device));
    return garbler_result_run(&h->c, d_m2, stride2, d_m3_out, stride3, d_len3_out, d_bits_out, d_verdict);
} catch (...) {
    return gc::on_exception();
}

int gc_yao_evaluator_accept_dev(gc_yao_evaluator *h, const void *d_m1, size_t stride1, void *d_verdict) try {
    if (!h || !d_verdict || !slots_ok(d_m1, stride1, h->c.g.len1)) return GC_E_ARG;
    GC_HIP(hipSetDevice(h->c.ctx->device));
    return accept_run(&h->c, d_m1, stride1, d_verdict);
} catch (...) {
    return gc::on_exception();
}

int gc_yao_evaluator_eval_dev(gc_yao_evaluator *h, const void *d_labels, void *d_m2_out, size_t stride2, void *d_verdict) try {
    if (!h || !d_labels || !d_verdict || !slots_ok(d_m2_out, stride2, h->c.g.len2())) return GC_E_ARG;
    GC_HIP(hipSetDevice(h->c.ctx->device));
    return eval_run(&h->c, d_labels, d_m2_out, stride2, d_verdict);
} catch (...) {
    return gc::on_exception();
}

int gc_yao_evaluator_result_dev(gc_yao_evaluator *h, const void *d_m3, size_t stride3, void *d_bits_out, void *d_verdict) try {
    if (!h || !d_bits_out || !d_verdict || !slots_ok(d_m3, stride3, h->c.g.slot3())) return GC_E_ARG;
    GC_HIP(hipSetDevice(h->c.ctx->device));
    return evaluator_result_run(&h->c, d_m3, stride3, d_bits_out, d_verdict);
} catch (...) {
    return gc::on_exception();
}

// The host forms.  A packed message array is staged as it is; its slots are device memory of their own and one kernel moves
// the messages between the two.  They are ordered against other work of the ctx by the stream alone.

int gc_yao_garbler_send(gc_yao_garbler *h, const uint8_t *keys, const uint8_t *rnd, const uint8_t *bits, uint8_t *m1_out) try {
    if (!h || !keys || !rnd || (!bits && h->c.g.ng) || !m1_out) return GC_E_ARG;
    Core *c = &h->c;
    const YaoGeom &g = c->g;
    const size_t S = g.S, len1 = g.len1, stride1 = slot_stride(len1);
    int rc = host_begin(c);
    if (rc != GC_OK) return rc;
    hipStream_t st = c->ctx->stream;
    Staged io[] = {{keys, nullptr, S * g.keylen}, {rnd, nullptr, S * 16 * (1 + (size_t)g.ng + g.ne)}, {bits, nullptr, S * g.ng},
                   {nullptr, m1_out, S * len1}, slots(S * stride1)};
    rc = stage_in(io, std::size(io), st);
    if (rc == GC_OK) rc = send_run(c, io[0].d.p, io[1].d.p, io[2].d.p, io[4].d.p, stride1);
    if (rc == GC_OK) rc = repack(S, io[4].d.p, stride1, io[3].d.p, len1, len1, st);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), st);
    return rc;
} catch (...) {
    return gc::on_exception();
}

int gc_yao_garbler_ot_wires(gc_yao_garbler *h, gc_wire *wires_out) try {
    if (!h || !wires_out) return GC_E_ARG;
    Core *c = &h->c;
    int rc = host_begin(c);
    if (rc != GC_OK) return rc;
    hipStream_t st = c->ctx->stream;
    Staged io[] = {{nullptr, wires_out, c->g.S * c->g.ne * sizeof(gc_wire)}};
    rc = stage_in(io, std::size(io), st);
    if (rc == GC_OK) rc = gc_batch_gather_input_wires(c->batch, c->g.ng, c->g.ne, io[0].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), st);
    return rc;
} catch (...) {
    return gc::on_exception();
}

int gc_yao_garbler_result(gc_yao_garbler *h, const uint8_t *m2, uint8_t *m3_out, uint32_t *len3_out, uint8_t *bits_out,
                          uint32_t *verdict, size_t *bad_session) try {
    if (!h || !m2 || !m3_out || !len3_out || !bits_out) return GC_E_ARG;
    Core *c = &h->c;
    const YaoGeom &g = c->g;
    const size_t S = g.S, len2 = g.len2(), slot3 = g.slot3(), stride3 = slot_stride(slot3);
    int rc = host_begin(c);
    if (rc != GC_OK) return rc;
    hipStream_t st = c->ctx->stream;
    std::unique_ptr<uint32_t[]> v(new uint32_t[S]);
    // M2 is a multiple of 16 bytes: the packed array is its slots.  M3's slots are zero behind a message
    Staged io[] = {{m2, nullptr, S * len2}, {nullptr, m3_out, S * slot3}, {nullptr, len3_out, S * sizeof(uint32_t)},
                   {nullptr, bits_out, S * g.bits_bytes()}, {nullptr, v.get(), S * sizeof(uint32_t)}, slots(S * stride3)};
    rc = stage_in(io, std::size(io), st);
    if (rc == GC_OK) rc = done(hipMemsetAsync(io[5].d.p, 0, S * stride3, st));
    if (rc == GC_OK) rc = garbler_result_run(c, io[0].d.p, len2, io[5].d.p, stride3, io[2].d.p, io[3].d.p, io[4].d.p);
    if (rc == GC_OK) rc = repack(S, io[5].d.p, stride3, io[1].d.p, slot3, slot3, st);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), st);
    return rc == GC_OK ? verdict_code(v.get(), S, verdict, bad_session) : rc;
} catch (...) {
    return gc::on_exception();
}

int gc_yao_evaluator_accept(gc_yao_evaluator *h, const uint8_t *m1, uint32_t *verdict, size_t *bad_session) try {
    if (!h || !m1) return GC_E_ARG;
    Core *c = &h->c;
    const size_t S = c->g.S, len1 = c->g.len1, stride1 = slot_stride(len1);
    int rc = host_begin(c);
    if (rc != GC_OK) return rc;
    hipStream_t st = c->ctx->stream;
    std::unique_ptr<uint32_t[]> v(new uint32_t[S]);
    Staged io[] = {{m1, nullptr, S * len1}, {nullptr, v.get(), S * sizeof(uint32_t)}, slots(S * stride1)};
    rc = stage_in(io, std::size(io), st);
    if (rc == GC_OK) rc = repack(S, io[0].d.p, len1, io[2].d.p, stride1, len1, st);
    if (rc == GC_OK) rc = accept_run(c, io[2].d.p, stride1, io[1].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), st);
    return rc == GC_OK ? verdict_code(v.get(), S, verdict, bad_session) : rc;
} catch (...) {
    return gc::on_exception();
}

int gc_yao_evaluator_eval(gc_yao_evaluator *h, const gc_label *labels, uint8_t *m2_out, uint32_t *verdict,
                          size_t *bad_session) try {
    if (!h || !labels || !m2_out) return GC_E_ARG;
    Core *c = &h->c;
    const size_t S = c->g.S, len2 = c->g.len2();
    int rc = host_begin(c);
    if (rc != GC_OK) return rc;
    hipStream_t st = c->ctx->stream;
    std::unique_ptr<uint32_t[]> v(new uint32_t[S]);
    Staged io[] = {{labels, nullptr, S * c->g.ne * sizeof(gc_label)}, {nullptr, m2_out, S * len2},
                   {nullptr, v.get(), S * sizeof(uint32_t)}};
    rc = stage_in(io, std::size(io), st);
    if (rc == GC_OK) rc = eval_run(c, io[0].d.p, io[1].d.p, len2, io[2].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), st);
    return rc == GC_OK ? verdict_code(v.get(), S, verdict, bad_session) : rc;
} catch (...) {
    return gc::on_exception();
}

int gc_yao_evaluator_result(gc_yao_evaluator *h, const uint8_t *m3, uint8_t *bits_out, uint32_t *verdict,
                            size_t *bad_session) try {
    if (!h || !m3 || !bits_out) return GC_E_ARG;
    Core *c = &h->c;
    const size_t S = c->g.S, slot3 = c->g.slot3(), stride3 = slot_stride(slot3);
    int rc = host_begin(c);
    if (rc != GC_OK) return rc;
    hipStream_t st = c->ctx->stream;
    std::unique_ptr<uint32_t[]> v(new uint32_t[S]);
    Staged io[] = {{m3, nullptr, S * slot3}, {nullptr, bits_out, S * c->g.bits_bytes()}, {nullptr, v.get(), S * sizeof(uint32_t)},
                   slots(S * stride3)};
    rc = stage_in(io, std::size(io), st);
    // (an n past the packed slot that still fits the stride reads the slot's padding: zero here)
    if (rc == GC_OK) rc = done(hipMemsetAsync(io[3].d.p, 0, S * stride3, st));
    if (rc == GC_OK) rc = repack(S, io[0].d.p, slot3, io[3].d.p, stride3, slot3, st);
    if (rc == GC_OK) rc = evaluator_result_run(c, io[3].d.p, stride3, io[1].d.p, io[2].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), st);
    return rc == GC_OK ? verdict_code(v.get(), S, verdict, bad_session) : rc;
} catch (...) {
    return gc::on_exception();
}

}  // extern "C"
