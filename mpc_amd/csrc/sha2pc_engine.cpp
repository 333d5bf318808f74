// sha2pc_engine.cpp — C ABI of the sha2pc rounds for S sessions per call (gcengine.h: gc_sha2pc_*; DESIGN.md §19;
// sha2pc/garbler.go, evaluator.go, encoding.go).  A round is a fixed sequence of launches on the ctx stream: the device calls
// the library has already (gc_co_multi_*_dev, gc_batch_garble_keyed / _eval_keyed, the dense table egress / ingest, the
// gathers) and between them the kernels of sha2pc_kernels.hip, which build and read the payloads.  A handle owns its batch
// and every array a round needs, so a _dev call allocates nothing and waits for nothing.  The host forms stage packed
// payloads through host_staging.h and run the _dev sequence on the staged copies.
#include <cstdio>
#include <cstring>
#include <iterator>
#include <memory>
#include <new>

#include "engine.h"
#include "sha2pc.h"

using namespace gc;

namespace {

constexpr size_t kKeyBytes = 32, kSidBytes = 8, kScalarBytes = 32, kPointBytes = sizeof(gc_p256_point);

int launched() {
    GC_HIP(hipGetLastError());
    return GC_OK;
}

int refuse(const char *what) {
    std::snprintf(gc::tls_error, sizeof gc::tls_error, "gc_sha2pc: %s", what);
    return GC_E_ARG;
}

size_t slot_stride(size_t lead, size_t len) { return (lead + len + 15) / 16 * 16; }

// the geometry of a handle; GC_E_ARG with a text for what create refuses
int geometry(const gc_plan_info &info, uint32_t ng, uint32_t ne, size_t S, Sha2pcGeom *g) {
    if ((uint64_t)ng + ne != info.ninputs) return refuse("ng + ne is not the circuit's input count");
    if (ne == 0 || info.noutputs == 0) return refuse("a circuit without evaluator inputs or without outputs");
    g->ng = ng;
    g->ne = ne;
    g->nout = info.noutputs;
    g->rows = info.slab_rows;
    g->S = S;
    g->bstride = 0;
    // the largest arrays of a handle: S slots of Round 3, S * (ng + ne) wires, nout rows of the batch
    const size_t per = slot_stride(kS2Round3Lead, g->len3()) + 64 * ((size_t)info.ninputs + info.noutputs + 64);
    if (S > UINT32_MAX || (S && per > SIZE_MAX / S)) return refuse("a size does not fit size_t");
    return GC_OK;
}

int layout(const gc_plan_info &info, uint32_t ng, uint32_t ne, size_t len[3], size_t lead[3], size_t *digest_bytes) {
    Sha2pcGeom g;
    const int rc = geometry(info, ng, ne, 1, &g);
    if (rc != GC_OK) return rc;
    if (len) len[0] = g.len1(), len[1] = g.len2(), len[2] = g.len3();
    if (lead) lead[0] = 0, lead[1] = 0, lead[2] = kS2Round3Lead;
    if (digest_bytes) *digest_bytes = g.digest_bytes();
    return GC_OK;
}

// what both handles are made of
struct Core {
    gc_ctx *ctx = nullptr;
    gc_batch *batch = nullptr;
    Sha2pcGeom g{};
    void *d_status = nullptr;   // the four uint64 of the gc_co_multi_*_dev calls
    uint32_t *d_badidx = nullptr;  // [S] lowest bad index of a session
    uint4 *d_points = nullptr;  // [S][ne] gc_p256_point
    uint4 *d_ct = nullptr;      // [S][ne][2]
    uint4 *d_outs = nullptr;    // [nout][bstride]
    uint4 *d_gl = nullptr;      // garbler: gc_wire [S][ng]; evaluator: gc_label [S][ng]
    uint4 *d_el = nullptr;      // garbler: gc_wire [S][ne]; evaluator: gc_label [S][ne]
    uint4 *d_keys = nullptr;    // evaluator: [S][32] bytes
    ~Core() {
        if (!ctx) return;
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);  // a _dev call may still use the arrays
        for (void *p : {d_status, (void *)d_badidx, (void *)d_points, (void *)d_ct, (void *)d_outs, (void *)d_gl, (void *)d_el,
                        (void *)d_keys})
            if (p) (void)hipFree(p);
        if (batch) gc_batch_free(batch);
    }
};

template <class T>
int dev_alloc(T **p, size_t bytes) {
    GC_HIP(hipMalloc((void **)p, bytes ? bytes : 16));
    return GC_OK;
}

int core_init(Core *h, gc_ctx *ctx, gc_circ *circ, uint32_t ng, uint32_t ne, size_t S, bool garbler) {
    if (!ctx || !circ || circ->ctx != ctx || S == 0 || ctx->capturing) return GC_E_ARG;
    int rc = geometry(circ->plan.p.info, ng, ne, S, &h->g);
    if (rc != GC_OK) return rc;
    rc = co_multi_prepare(ctx);
    if (rc != GC_OK) return rc;
    h->ctx = ctx;
    h->batch = gc_batch_create(circ, (uint32_t)S, &rc);
    if (!h->batch) return rc;
    if (h->batch->schedule != 1) rc = gc_batch_set_schedule(h->batch, 1);
    if (rc != GC_OK) return rc;
    if (!gc_batch_keyed_supported(h->batch)) return refuse("gc_batch_keyed_supported is 0 for a batch of S instances of this circuit");
    h->g.bstride = gc_batch_stride(h->batch);
    const Sha2pcGeom &g = h->g;
    GC_HIP(hipSetDevice(ctx->device));
    // the keyed passes' expanded keys, which the batch would allocate at its first keyed pass
    if (!h->batch->d_keyed_rk) rc = dev_alloc(&h->batch->d_keyed_rk, S * 60 * sizeof(uint32_t));
    const size_t per_g = garbler ? sizeof(gc_wire) : sizeof(gc_label);
    if (rc == GC_OK) rc = dev_alloc(&h->d_status, 32);
    if (rc == GC_OK) rc = dev_alloc(&h->d_badidx, S * sizeof(uint32_t));
    if (rc == GC_OK) rc = dev_alloc(&h->d_points, S * g.ne * kPointBytes);
    if (rc == GC_OK) rc = dev_alloc(&h->d_ct, S * g.ne * 32);
    if (rc == GC_OK) rc = dev_alloc(&h->d_outs, (size_t)g.nout * g.bstride * sizeof(gc_label));
    if (rc == GC_OK) rc = dev_alloc(&h->d_gl, S * g.ng * per_g);
    if (rc == GC_OK) rc = dev_alloc(&h->d_el, S * g.ne * per_g);
    if (rc == GC_OK && !garbler) rc = dev_alloc(&h->d_keys, S * kKeyBytes);
    return rc;
}

bool slots_ok(const void *d, size_t stride, size_t lead, size_t len) {
    return d && (stride & 15) == 0 && stride >= lead + len && ((uintptr_t)d & 15) == 0;
}

// ---- the rounds on device pointers, the device set: what a _dev form does behind its checks ------------------------------

int round1_run(Core *h, const void *d_a, const void *d_sid, void *d_A_out, void *d_AaInv_out, void *d_r1, size_t stride1,
               void *d_verdict) {
    const int rc = gc_co_multi_sender_setup_dev(h->ctx, d_a, h->g.S, d_A_out, d_AaInv_out, h->d_status);
    if (rc != GC_OK) return rc;
    launch_s2_r1_encode(h->g.S, (const uint4 *)d_A_out, (const uint2 *)d_sid, (uint8_t *)d_r1, stride1, (uint32_t *)d_verdict,
                        h->ctx->stream);
    return launched();
}

int round2_run(Core *h, const void *d_r1, size_t stride1, const void *d_scalars, const void *d_bits, void *d_A_out,
               void *d_sid_out, void *d_r2, size_t stride2, void *d_verdict) {
    hipStream_t st = h->ctx->stream;
    launch_s2_r2_take(h->g.S, (const uint8_t *)d_r1, stride1, (uint4 *)d_A_out, (uint2 *)d_sid_out, (uint32_t *)d_verdict, st);
    int rc = launched();
    // BuildCOChoices; a bad session has a zero A and gets zero points
    if (rc == GC_OK) rc = gc_co_multi_receiver_choices_dev(h->ctx, d_A_out, d_scalars, d_bits, h->g.S, h->g.ne, h->d_points, h->d_status);
    if (rc != GC_OK) return rc;
    launch_s2_r2_encode(h->g, h->d_points, (const uint2 *)d_sid_out, (const uint32_t *)d_verdict, (uint8_t *)d_r2, stride2, st);
    return launched();
}

int round3_run(Core *h, const void *d_a, const void *d_AaInv, const void *d_sid, const void *d_r2, size_t stride2,
               const void *d_keys, const void *d_rnd, const void *d_bits, void *d_r3, size_t stride3, void *d_verdict) {
    const Sha2pcGeom &g = h->g;
    hipStream_t st = h->ctx->stream;
    uint8_t *r3 = (uint8_t *)d_r3;
    GC_HIP(hipMemsetAsync(h->d_badidx, 0xff, g.S * sizeof(uint32_t), st));
    launch_s2_r3_decode(g, (const uint8_t *)d_r2, stride2, h->d_points, h->d_badidx, st);
    launch_s2_r3_header(g.S, (const uint8_t *)d_r2, stride2, (const uint2 *)d_sid, (const uint4 *)d_a, (const uint4 *)d_AaInv,
                        h->d_badidx, (uint32_t *)d_verdict, st);
    int rc = launched();
    if (rc == GC_OK) rc = gc_batch_garble_keyed(h->batch, d_keys, kKeyBytes, d_rnd);
    if (rc == GC_OK) rc = gc_batch_gather_input_wires(h->batch, 0, g.ng, h->d_gl);
    if (rc == GC_OK) rc = gc_batch_gather_input_wires(h->batch, g.ng, g.ne, h->d_el);
    if (rc == GC_OK) rc = gc_batch_gather_outputs(h->batch, h->d_outs);
    // EncryptCOCiphertexts; its rows are 32 bytes apart and a slot's are not S * ne in a row: copied once by the assemble
    if (rc == GC_OK) rc = gc_co_multi_sender_encrypt_dev(h->ctx, d_a, d_AaInv, h->d_points, h->d_el, g.S, g.ne, 0, h->d_ct, h->d_status);
    // the tables straight into the slots
    if (rc == GC_OK) rc = gc_batch_egress_tables_dense(h->batch, r3 + kS2TablesAt, stride3);
    if (rc != GC_OK) return rc;
    launch_s2_r3_assemble(g, h->d_gl, (const uint8_t *)d_bits, h->d_outs, (const uint4 *)gc_batch_dev_r(h->batch), h->d_ct,
                          (const uint2 *)d_sid, (const uint4 *)d_keys, (const uint32_t *)d_verdict, r3, stride3, st);
    launch_s2_zero_bad(g.S, (const uint32_t *)d_verdict, r3, stride3, kS2TablesAt, g.rows, st);
    return launched();
}

int round4_run(Core *h, const void *d_A, const void *d_sid, const void *d_scalars, const void *d_bits, const void *d_r3,
               size_t stride3, void *d_digest, void *d_verdict) {
    const Sha2pcGeom &g = h->g;
    hipStream_t st = h->ctx->stream;
    const uint8_t *r3 = (const uint8_t *)d_r3;
    GC_HIP(hipMemsetAsync(h->d_badidx, 0xff, g.S * sizeof(uint32_t), st));
    launch_s2_r4_take(g, r3, stride3, (const uint2 *)d_sid, (const uint4 *)d_A, h->d_keys, h->d_gl, h->d_ct,
                      (uint32_t *)d_verdict, st);
    int rc = launched();
    if (rc == GC_OK) rc = gc_batch_ingest_tables_dense(h->batch, r3 + kS2TablesAt, stride3);
    // DecryptCOCiphertexts
    if (rc == GC_OK) rc = gc_co_multi_receiver_decrypt_dev(h->ctx, d_A, d_scalars, d_bits, h->d_ct, g.S, g.ne, 0, h->d_el, h->d_status);
    if (rc == GC_OK) rc = gc_batch_set_input_range(h->batch, 0, g.ng, h->d_gl);
    if (rc == GC_OK) rc = gc_batch_set_input_range(h->batch, g.ng, g.ne, h->d_el);
    if (rc == GC_OK) rc = gc_batch_eval_keyed(h->batch, h->d_keys, kKeyBytes, h->batch);
    if (rc == GC_OK) rc = gc_batch_gather_outputs(h->batch, h->d_outs);
    if (rc != GC_OK) return rc;
    launch_s2_r4_decode(g, h->d_outs, r3, stride3, (uint8_t *)d_digest, h->d_badidx, st);
    launch_s2_r4_verdict(g.S, g.digest_bytes(), h->d_badidx, (uint32_t *)d_verdict, (uint8_t *)d_digest, st);
    return launched();
}

// ---- host forms ------------------------------------------------------------------------------------------------------------

// the verdicts of a host form -> its return code: that of the lowest bad session
int verdict_code(const uint32_t *v, size_t S, bool garbler, uint32_t *verdict_out, size_t *bad_session) {
    if (verdict_out) std::memcpy(verdict_out, v, S * sizeof(uint32_t));
    for (size_t s = 0; s < S; s++) {
        if (!v[s]) continue;
        if (bad_session) *bad_session = s;
        const uint32_t code = v[s] & 0xffu;
        return code == kS2Point || (code == kS2Setup && !garbler) ? GC_E_POINT : GC_E_ARG;
    }
    return GC_OK;
}

// a Staged that is device memory alone: the slots of a payload array
Staged slots(size_t bytes) { return Staged{nullptr, nullptr, 0, bytes}; }

}  // namespace

struct gc_sha2pc_garbler {
    Core c;
};
struct gc_sha2pc_evaluator {
    Core c;
};

namespace {

template <class H>
H *create(gc_ctx *ctx, gc_circ *circ, uint32_t ng, uint32_t ne, size_t S, bool garbler, int *status) try {
    std::unique_ptr<H> h(new H);
    const int rc = core_init(&h->c, ctx, circ, ng, ne, S, garbler);
    if (status) *status = rc;
    return rc == GC_OK ? h.release() : nullptr;
} catch (...) {
    const int rc__ = gc::on_exception();
    if (status) *status = rc__;
    return nullptr;
}

}  // namespace

extern "C" {

gc_sha2pc_garbler *gc_sha2pc_garbler_create(gc_ctx *ctx, gc_circ *circ, uint32_t ng, uint32_t ne, size_t S, int *status) {
    return create<gc_sha2pc_garbler>(ctx, circ, ng, ne, S, true, status);
}
gc_sha2pc_evaluator *gc_sha2pc_evaluator_create(gc_ctx *ctx, gc_circ *circ, uint32_t ng, uint32_t ne, size_t S, int *status) {
    return create<gc_sha2pc_evaluator>(ctx, circ, ng, ne, S, false, status);
}
void gc_sha2pc_garbler_free(gc_sha2pc_garbler *h) { delete h; }
void gc_sha2pc_evaluator_free(gc_sha2pc_evaluator *h) { delete h; }

int gc_sha2pc_layout_plan(const gc_plan *plan, uint32_t ng, uint32_t ne, size_t len[3], size_t lead[3], size_t *digest_bytes) {
    return plan ? layout(plan->p.info, ng, ne, len, lead, digest_bytes) : GC_E_ARG;
}
int gc_sha2pc_layout(const gc_circ *circ, uint32_t ng, uint32_t ne, size_t len[3], size_t lead[3], size_t *digest_bytes) {
    return circ ? layout(circ->plan.p.info, ng, ne, len, lead, digest_bytes) : GC_E_ARG;
}

int gc_sha2pc_garbler_round1_dev(gc_sha2pc_garbler *h, const void *d_a, const void *d_sid, void *d_A_out, void *d_AaInv_out,
                                 void *d_r1_out, size_t stride1, void *d_verdict) try {
    if (!h || !d_a || !d_sid || !d_A_out || !d_AaInv_out || !d_verdict || !slots_ok(d_r1_out, stride1, 0, h->c.g.len1()))
        return GC_E_ARG;
    GC_HIP(hipSetDevice(h->c.ctx->device));
    return round1_run(&h->c, d_a, d_sid, d_A_out, d_AaInv_out, d_r1_out, stride1, d_verdict);
} catch (...) {
    return gc::on_exception();
}

int gc_sha2pc_evaluator_round2_dev(gc_sha2pc_evaluator *h, const void *d_r1, size_t stride1, const void *d_scalars,
                                   const void *d_bits, void *d_A_out, void *d_sid_out, void *d_r2_out, size_t stride2,
                                   void *d_verdict) try {
    if (!h || !d_scalars || !d_bits || !d_A_out || !d_sid_out || !d_verdict || !slots_ok(d_r1, stride1, 0, h->c.g.len1()) ||
        !slots_ok(d_r2_out, stride2, 0, h->c.g.len2()))
        return GC_E_ARG;
    GC_HIP(hipSetDevice(h->c.ctx->device));
    return round2_run(&h->c, d_r1, stride1, d_scalars, d_bits, d_A_out, d_sid_out, d_r2_out, stride2, d_verdict);
} catch (...) {
    return gc::on_exception();
}

int gc_sha2pc_garbler_round3_dev(gc_sha2pc_garbler *h, const void *d_a, const void *d_AaInv, const void *d_sid,
                                 const void *d_r2, size_t stride2, const void *d_keys, const void *d_rnd, const void *d_bits,
                                 void *d_r3_out, size_t stride3, void *d_verdict) try {
    if (!h || !d_a || !d_AaInv || !d_sid || !d_keys || !d_rnd || (!d_bits && h->c.g.ng) || !d_verdict ||
        !slots_ok(d_r2, stride2, 0, h->c.g.len2()) || !slots_ok(d_r3_out, stride3, kS2Round3Lead, h->c.g.len3()))
        return GC_E_ARG;
    GC_HIP(hipSetDevice(h->c.ctx->device));
    return round3_run(&h->c, d_a, d_AaInv, d_sid, d_r2, stride2, d_keys, d_rnd, d_bits, d_r3_out, stride3, d_verdict);
} catch (...) {
    return gc::on_exception();
}

int gc_sha2pc_evaluator_round4_dev(gc_sha2pc_evaluator *h, const void *d_A, const void *d_sid, const void *d_scalars,
                                   const void *d_bits, const void *d_r3, size_t stride3, void *d_digest_out,
                                   void *d_verdict) try {
    if (!h || !d_A || !d_sid || !d_scalars || !d_bits || !d_digest_out || !d_verdict ||
        !slots_ok(d_r3, stride3, kS2Round3Lead, h->c.g.len3()))
        return GC_E_ARG;
    GC_HIP(hipSetDevice(h->c.ctx->device));
    return round4_run(&h->c, d_A, d_sid, d_scalars, d_bits, d_r3, stride3, d_digest_out, d_verdict);
} catch (...) {
    return gc::on_exception();
}

// The host forms.  A packed payload array is staged as it is; where a slot is wider than its payload or begins off its
// slot's start, the slots are device memory of their own and one kernel moves the payloads between the two.  The rounds call
// gc_co_multi_*_dev, which take the ctx lock themselves: a host form does not hold it, and is ordered against other work of
// the ctx by the stream alone.

int gc_sha2pc_garbler_round1(gc_sha2pc_garbler *h, const uint8_t *a, const uint8_t *sid, gc_p256_point *A_out,
                             gc_p256_point *AaInv_out, uint8_t *r1_out, uint32_t *verdict, size_t *bad_session) try {
    if (!h || !a || !sid || !A_out || !AaInv_out || !r1_out) return GC_E_ARG;
    Core *c = &h->c;
    const size_t S = c->g.S, len1 = c->g.len1();  // 80 bytes: a slot as it is
    GC_HIP(hipSetDevice(c->ctx->device));
    std::unique_ptr<uint32_t[]> v(new uint32_t[S]);
    Staged io[] = {{a, nullptr, S * kScalarBytes}, {sid, nullptr, S * kSidBytes}, {nullptr, A_out, S * kPointBytes},
                   {nullptr, AaInv_out, S * kPointBytes}, {nullptr, r1_out, S * len1}, {nullptr, v.get(), S * sizeof(uint32_t)}};
    int rc = stage_in(io, std::size(io), c->ctx->stream);
    if (rc == GC_OK) rc = round1_run(c, io[0].d.p, io[1].d.p, io[2].d.p, io[3].d.p, io[4].d.p, len1, io[5].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), c->ctx->stream);
    return rc == GC_OK ? verdict_code(v.get(), S, true, verdict, bad_session) : rc;
} catch (...) {
    return gc::on_exception();
}

int gc_sha2pc_evaluator_round2(gc_sha2pc_evaluator *h, const uint8_t *r1, const uint8_t *scalars, const uint8_t *bits,
                               gc_p256_point *A_out, uint8_t *sid_out, uint8_t *r2_out, uint32_t *verdict,
                               size_t *bad_session) try {
    if (!h || !r1 || !scalars || !bits || !A_out || !sid_out || !r2_out) return GC_E_ARG;
    Core *c = &h->c;
    const size_t S = c->g.S, n = S * c->g.ne, len1 = c->g.len1(), len2 = c->g.len2(), stride2 = slot_stride(0, len2);
    GC_HIP(hipSetDevice(c->ctx->device));
    hipStream_t st = c->ctx->stream;
    std::unique_ptr<uint32_t[]> v(new uint32_t[S]);
    Staged io[] = {{r1, nullptr, S * len1}, {scalars, nullptr, n * kScalarBytes}, {bits, nullptr, n},
                   {nullptr, A_out, S * kPointBytes}, {nullptr, sid_out, S * kSidBytes}, {nullptr, r2_out, S * len2},
                   {nullptr, v.get(), S * sizeof(uint32_t)}, slots(S * stride2)};
    int rc = stage_in(io, std::size(io), st);
    if (rc == GC_OK) rc = round2_run(c, io[0].d.p, len1, io[1].d.p, io[2].d.p, io[3].d.p, io[4].d.p, io[7].d.p, stride2, io[6].d.p);
    if (rc == GC_OK) {
        launch_s2_repack(S, (const uint8_t *)io[7].d.p, stride2, (uint8_t *)io[5].d.p, len2, len2, st);
        rc = launched();
    }
    if (rc == GC_OK) rc = stage_out(io, std::size(io), st);
    return rc == GC_OK ? verdict_code(v.get(), S, false, verdict, bad_session) : rc;
} catch (...) {
    return gc::on_exception();
}

int gc_sha2pc_garbler_round3(gc_sha2pc_garbler *h, const uint8_t *a, const gc_p256_point *AaInv, const uint8_t *sid,
                             const uint8_t *r2, const uint8_t *keys, const uint8_t *rnd, const uint8_t *bits, uint8_t *r3_out,
                             uint32_t *verdict, size_t *bad_session) try {
    if (!h || !a || !AaInv || !sid || !r2 || !keys || !rnd || (!bits && h->c.g.ng) || !r3_out) return GC_E_ARG;
    Core *c = &h->c;
    const Sha2pcGeom &g = c->g;
    const size_t S = g.S, len2 = g.len2(), len3 = g.len3(), stride2 = slot_stride(0, len2),
                 stride3 = slot_stride(kS2Round3Lead, len3);
    GC_HIP(hipSetDevice(c->ctx->device));
    hipStream_t st = c->ctx->stream;
    std::unique_ptr<uint32_t[]> v(new uint32_t[S]);
    Staged io[] = {{a, nullptr, S * kScalarBytes}, {AaInv, nullptr, S * kPointBytes}, {sid, nullptr, S * kSidBytes},
                   {r2, nullptr, S * len2}, {keys, nullptr, S * kKeyBytes},
                   {rnd, nullptr, S * 16 * (1 + (size_t)g.ng + g.ne)}, {bits, nullptr, S * g.ng}, {nullptr, r3_out, S * len3},
                   {nullptr, v.get(), S * sizeof(uint32_t)}, slots(S * stride2), slots(S * stride3)};
    int rc = stage_in(io, std::size(io), st);
    if (rc == GC_OK) {
        launch_s2_repack(S, (const uint8_t *)io[3].d.p, len2, (uint8_t *)io[9].d.p, stride2, len2, st);
        rc = launched();
    }
    if (rc == GC_OK)
        rc = round3_run(c, io[0].d.p, io[1].d.p, io[2].d.p, io[9].d.p, stride2, io[4].d.p, io[5].d.p, io[6].d.p, io[10].d.p,
                        stride3, io[8].d.p);
    if (rc == GC_OK) {
        launch_s2_repack(S, (const uint8_t *)io[10].d.p + kS2Round3Lead, stride3, (uint8_t *)io[7].d.p, len3, len3, st);
        rc = launched();
    }
    if (rc == GC_OK) rc = stage_out(io, std::size(io), st);
    return rc == GC_OK ? verdict_code(v.get(), S, true, verdict, bad_session) : rc;
} catch (...) {
    return gc::on_exception();
}

int gc_sha2pc_evaluator_round4(gc_sha2pc_evaluator *h, const gc_p256_point *A, const uint8_t *sid, const uint8_t *scalars,
                               const uint8_t *bits, const uint8_t *r3, uint8_t *digest_out, uint32_t *verdict,
                               size_t *bad_session) try {
    if (!h || !A || !sid || !scalars || !bits || !r3 || !digest_out) return GC_E_ARG;
    Core *c = &h->c;
    const Sha2pcGeom &g = c->g;
    const size_t S = g.S, n = S * g.ne, len3 = g.len3(), stride3 = slot_stride(kS2Round3Lead, len3);
    GC_HIP(hipSetDevice(c->ctx->device));
    hipStream_t st = c->ctx->stream;
    std::unique_ptr<uint32_t[]> v(new uint32_t[S]);
    Staged io[] = {{A, nullptr, S * kPointBytes}, {sid, nullptr, S * kSidBytes}, {scalars, nullptr, n * kScalarBytes},
                   {bits, nullptr, n}, {r3, nullptr, S * len3}, {nullptr, digest_out, S * g.digest_bytes()},
                   {nullptr, v.get(), S * sizeof(uint32_t)}, slots(S * stride3)};
    int rc = stage_in(io, std::size(io), st);
    if (rc == GC_OK) {
        launch_s2_repack(S, (const uint8_t *)io[4].d.p, len3, (uint8_t *)io[7].d.p + kS2Round3Lead, stride3, len3, st);
        rc = launched();
    }
    if (rc == GC_OK) rc = round4_run(c, io[0].d.p, io[1].d.p, io[2].d.p, io[3].d.p, io[7].d.p, stride3, io[5].d.p, io[6].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), st);
    return rc == GC_OK ? verdict_code(v.get(), S, false, verdict, bad_session) : rc;
} catch (...) {
    return gc::on_exception();
}

}  // extern "C"
