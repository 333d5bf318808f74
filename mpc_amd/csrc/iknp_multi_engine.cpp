// iknp_multi_engine.cpp — C ABI of the multi-session IKNP extension and COT pad loops (gc_iknp_multi_*, gc_cot_multi_*):
// S sessions of `per` OTs each, session-major, one kernel per call (iknp_multi_kernels.hip; layouts: iknp_multi.h), of
// bit-COT on the same handle (gc_iknp_multi_*_bits*) and of the triple folds over S peers (gc_gmw_triples_multi_*;
// iknp_multi_bits_kernels.hip, iknp_multi_bits.h).  A host form is staging (host_staging.h) around the operation of its _dev
// form.
#include <algorithm>
#include <cstring>
#include <iterator>
#include <new>

#include "engine.h"
#include "iknp_multi_bits.h"

using namespace gc;

struct gc_iknp_multi {
    gc_ctx *ctx = nullptr;
    bool receiver = false;
    size_t S = 0;
    uint4 *d_keys = nullptr;   // sender: k0 [S][128]; receiver: the label pairs [S][128][2]
    uint4 *d_delta = nullptr;  // sender: [S]
    uint64_t pos = 0;          // bytes drawn so far from every column stream of every session
};

namespace {

constexpr size_t kKeyBytesSend = 128 * sizeof(gc_label), kKeyBytesRecv = 128 * sizeof(gc_wire);

// the byte counts of a call of S sessions of per OTs; false: one of them does not fit size_t
struct MultiSizes {
    size_t n, choice, u, labels;
};
bool multi_sizes(size_t S, size_t per, MultiSizes *z) {
    if (per && S > SIZE_MAX / per) return false;
    z->n = S * per;
    if (z->n > SIZE_MAX / 64) return false;  // 16 bytes of label, 32 of wire and 32 of pad per OT, with room to spare
    const uint64_t chunks = iknp_multi_chunks(per);
    if (S > SIZE_MAX / (chunks ? chunks * 8192 : 1)) return false;
    z->choice = S * (size_t)iknp_multi_choice_bytes(per);
    z->u = S * (size_t)iknp_multi_u_bytes(per);
    z->labels = z->n * sizeof(gc_label);
    return true;
}

void multi_release(gc_iknp_multi *h) {
    if (h->d_keys) (void)hipFree(h->d_keys);
    if (h->d_delta) (void)hipFree(h->d_delta);
    delete h;
}

int multi_alloc(void **p, size_t bytes) {
    GC_HIP(hipMalloc(p, bytes));  // (out of memory: GC_E_NOMEM)
    return GC_OK;
}

// copies of the base labels: from the host (synchronous) or from device memory, behind what is queued on the ctx stream
int multi_fill(gc_iknp_multi *h, gc_ctx *ctx, const void *keys, const void *delta, bool dev) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    const size_t kb = h->S * (h->receiver ? kKeyBytesRecv : kKeyBytesSend);
    int rc = multi_alloc((void **)&h->d_keys, kb);
    if (rc == GC_OK && !h->receiver) rc = multi_alloc((void **)&h->d_delta, h->S * sizeof(gc_label));
    if (rc != GC_OK) return rc;
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    GC_HIP(hipMemcpyAsync(h->d_keys, keys, kb, kind, ctx->stream));
    if (!h->receiver) GC_HIP(hipMemcpyAsync(h->d_delta, delta, h->S * sizeof(gc_label), kind, ctx->stream));
    if (!dev) GC_HIP(hipStreamSynchronize(ctx->stream));  // the caller's arrays are free again on return
    return GC_OK;
}

gc_iknp_multi *multi_create(gc_ctx *ctx, bool receiver, const void *keys, const void *delta, size_t S, bool dev,
                            int *status) try {
    int rc = GC_OK;
    gc_iknp_multi *h = nullptr;
    if (!ctx || !keys || (!receiver && !delta) || S == 0 || S > SIZE_MAX / kKeyBytesRecv) {
        rc = GC_E_ARG;
    } else if (ctx->capturing) {
        rc = GC_E_ARG;  // allocates: not between gc_ctx_capture_begin and _end
    } else if (!(h = new (std::nothrow) gc_iknp_multi)) {
        rc = GC_E_NOMEM;
    } else {
        h->ctx = ctx;
        h->receiver = receiver;
        h->S = S;
        rc = multi_fill(h, ctx, keys, delta, dev);
        if (rc != GC_OK) {
            (void)hipStreamSynchronize(ctx->stream);  // a copy may be queued on what is freed next
            multi_release(h);
            h = nullptr;
        }
    }
    if (status) *status = rc;
    return h;
} catch (...) {
    const int rc__ = gc::on_exception();
    if (status) *status = rc__;
    return nullptr;
}

// the checks every receive / send shares; GC_OK with *z filled, or the code to return (per = 0: z->n = 0)
int multi_call_args(const gc_iknp_multi *h, bool receiver, size_t per, MultiSizes *z) {
    if (!h || h->receiver != receiver || !multi_sizes(h->S, per, z)) return GC_E_ARG;
    // the stream position is a kernel argument and advances with every call: a replayed capture would reuse it
    if (per && h->ctx->capturing) return GC_E_ARG;
    return GC_OK;
}

// The operations on device pointers, the device set: what a _dev form does behind its argument checks.  The stream position
// is the caller's to advance.
// the receiver's (d_choice_packed -> d_u_out, d_labels_out) or the sender's (d_u_in -> d_labels_out) extension
int extend_run(gc_iknp_multi *h, size_t per, const void *d_choice_packed, const void *d_u_in, void *d_u_out, void *d_labels_out) {
    GC_HIP(launch_iknp_multi(h->receiver, h->d_keys, h->d_delta, h->pos, h->S, per, (const uint8_t *)d_choice_packed,
                             (const uint8_t *)d_u_in, (uint8_t *)d_u_out, (uint4 *)d_labels_out, h->ctx->d_te0, h->ctx->stream));
    return GC_OK;
}
int cot_send_run(gc_ctx *ctx, const void *d_seed, const void *d_delta, const void *d_data, const void *d_wires, size_t S,
                 size_t per, void *d_out) {
    GC_HIP(launch_cot_multi_send((const uint4 *)d_seed, (const uint4 *)d_delta, (const uint4 *)d_data, (const uint4 *)d_wires, S,
                                 per, (uint4 *)d_out, ctx->d_te0, ctx->stream));
    return GC_OK;
}
int cot_recv_run(gc_ctx *ctx, const void *d_seed, const void *d_flags, const void *d_sent, void *d_result, size_t S, size_t per) {
    GC_HIP(launch_cot_multi_recv((const uint4 *)d_seed, (const uint8_t *)d_flags, (const uint4 *)d_sent, (uint4 *)d_result, S,
                                 per, ctx->d_te0, ctx->stream));
    return GC_OK;
}

}  // namespace

extern "C" {

gc_iknp_multi *gc_iknp_multi_sender_create(gc_ctx *ctx, const gc_label *delta, const gc_label *k0, size_t S, int *status) {
    return multi_create(ctx, false, k0, delta, S, false, status);
}

gc_iknp_multi *gc_iknp_multi_sender_create_dev(gc_ctx *ctx, const void *d_delta, const void *d_k0, size_t S, int *status) {
    return multi_create(ctx, false, d_k0, d_delta, S, true, status);
}

gc_iknp_multi *gc_iknp_multi_receiver_create(gc_ctx *ctx, const gc_wire *base, size_t S, int *status) {
    return multi_create(ctx, true, base, nullptr, S, false, status);
}

gc_iknp_multi *gc_iknp_multi_receiver_create_dev(gc_ctx *ctx, const void *d_base, size_t S, int *status) {
    return multi_create(ctx, true, d_base, nullptr, S, true, status);
}

void gc_iknp_multi_free(gc_iknp_multi *h) {
    if (!h) return;
    if (h->ctx) {
        (void)hipSetDevice(h->ctx->device);
        (void)hipStreamSynchronize(h->ctx->stream);  // a _dev call may still read the labels
    }
    multi_release(h);
}

int gc_iknp_multi_info(const gc_iknp_multi *h, size_t *S, int *receiver, uint64_t *pos) {
    if (!h) return GC_E_ARG;
    if (S) *S = h->S;
    if (receiver) *receiver = h->receiver ? 1 : 0;
    if (pos) *pos = h->pos;
    return GC_OK;
}

int gc_iknp_multi_receive_dev(gc_iknp_multi *h, const void *d_choice_packed, size_t per, void *d_u_out, void *d_labels_out) {
    MultiSizes z;
    int rc = multi_call_args(h, true, per, &z);
    if (rc != GC_OK) return rc;
    if (per == 0) return GC_OK;
    if (!d_choice_packed || !d_u_out || !d_labels_out) return GC_E_ARG;
    gc_ctx *ctx = h->ctx;
    GC_HIP(hipSetDevice(ctx->device));
    rc = extend_run(h, per, d_choice_packed, nullptr, d_u_out, d_labels_out);
    if (rc == GC_OK) h->pos += iknp_multi_advance(per);
    return rc;
}

int gc_iknp_multi_send_dev(gc_iknp_multi *h, const void *d_u_in, size_t per, void *d_labels_out) {
    MultiSizes z;
    int rc = multi_call_args(h, false, per, &z);
    if (rc != GC_OK) return rc;
    if (per == 0) return GC_OK;
    if (!d_u_in || !d_labels_out) return GC_E_ARG;
    gc_ctx *ctx = h->ctx;
    GC_HIP(hipSetDevice(ctx->device));
    rc = extend_run(h, per, nullptr, d_u_in, nullptr, d_labels_out);
    if (rc == GC_OK) h->pos += iknp_multi_advance(per);
    return rc;
}

int gc_iknp_multi_receive(gc_iknp_multi *h, const uint8_t *choice, size_t per, uint8_t *u_out, gc_label *labels_out) try {
    MultiSizes z;
    int rc = multi_call_args(h, true, per, &z);
    if (rc != GC_OK) return rc;
    if (per == 0) return GC_OK;
    if (!choice || !u_out || !labels_out) return GC_E_ARG;
    const std::vector<uint8_t> bbuf = pack_rows(choice, h->S, per, (size_t)iknp_multi_choice_bytes(per));  // z.choice bytes
    gc_ctx *ctx = h->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    Staged io[] = {{bbuf.data(), nullptr, z.choice}, {nullptr, u_out, z.u}, {nullptr, labels_out, z.labels}};
    rc = stage_in(io, std::size(io), ctx->stream);
    if (rc == GC_OK) rc = extend_run(h, per, io[0].d.p, nullptr, io[1].d.p, io[2].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), ctx->stream);
    if (rc == GC_OK) h->pos += iknp_multi_advance(per);
    return rc;
} catch (...) {
    return gc::on_exception();
}

int gc_iknp_multi_send(gc_iknp_multi *h, const uint8_t *u_in, size_t u_len, size_t per, gc_label *labels_out) try {
    MultiSizes z;
    int rc = multi_call_args(h, false, per, &z);
    if (rc != GC_OK) return rc;
    if (per == 0) return GC_OK;
    if (!u_in || !labels_out || u_len != z.u) return GC_E_ARG;  // "invalid chunk size" (iknp.go:207-209)
    gc_ctx *ctx = h->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    Staged io[] = {{u_in, nullptr, z.u}, {nullptr, labels_out, z.labels}};
    rc = stage_in(io, std::size(io), ctx->stream);
    if (rc == GC_OK) rc = extend_run(h, per, nullptr, io[0].d.p, nullptr, io[1].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), ctx->stream);
    if (rc == GC_OK) h->pos += iknp_multi_advance(per);
    return rc;
} catch (...) {
    return gc::on_exception();
}

// ---- the COT pad loops (cot.go:136-235) per session: key index j of session s under seed_s, delta_s -----------------------

int gc_cot_multi_send_pads_dev(gc_ctx *ctx, const void *d_seed, const void *d_delta, const void *d_data, const void *d_wires,
                               size_t S, size_t per, void *d_out) {
    MultiSizes z;
    if (!ctx || S == 0 || !multi_sizes(S, per, &z)) return GC_E_ARG;
    if (per == 0) return GC_OK;
    if (!d_seed || !d_delta || !d_data || !d_wires || !d_out) return GC_E_ARG;
    GC_HIP(hipSetDevice(ctx->device));
    return cot_send_run(ctx, d_seed, d_delta, d_data, d_wires, S, per, d_out);
}

int gc_cot_multi_receive_unpad_dev(gc_ctx *ctx, const void *d_seed, const void *d_flags, const void *d_sent, void *d_result,
                                   size_t S, size_t per) {
    MultiSizes z;
    if (!ctx || S == 0 || !multi_sizes(S, per, &z)) return GC_E_ARG;
    if (per == 0) return GC_OK;
    if (!d_seed || !d_flags || !d_sent || !d_result) return GC_E_ARG;
    GC_HIP(hipSetDevice(ctx->device));
    return cot_recv_run(ctx, d_seed, d_flags, d_sent, d_result, S, per);
}

int gc_cot_multi_send_pads(gc_ctx *ctx, const gc_label *seed, const gc_label *delta, const gc_label *data,
                           const gc_wire *wires, size_t S, size_t per, gc_label *out) try {
    MultiSizes z;
    if (!ctx || S == 0 || !multi_sizes(S, per, &z)) return GC_E_ARG;
    if (per == 0) return GC_OK;
    if (!seed || !delta || !data || !wires || !out) return GC_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    Staged io[] = {{seed, nullptr, S * 16}, {delta, nullptr, S * 16}, {data, nullptr, z.n * 16}, {wires, nullptr, z.n * 32},
                   {nullptr, out, z.n * 32}};
    int rc = stage_in(io, std::size(io), ctx->stream);
    if (rc == GC_OK) rc = cot_send_run(ctx, io[0].d.p, io[1].d.p, io[2].d.p, io[3].d.p, S, per, io[4].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), ctx->stream);
    return rc;
} catch (...) {
    return gc::on_exception();
}

int gc_cot_multi_receive_unpad(gc_ctx *ctx, const gc_label *seed, const uint8_t *flags, const gc_label *sent,
                               gc_label *result, size_t S, size_t per) try {
    MultiSizes z;
    if (!ctx || S == 0 || !multi_sizes(S, per, &z)) return GC_E_ARG;
    if (per == 0) return GC_OK;
    if (!seed || !flags || !sent || !result) return GC_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    Staged io[] = {{seed, nullptr, S * 16}, {flags, nullptr, z.n}, {sent, nullptr, z.n * 32}, {result, result, z.n * 16}};
    int rc = stage_in(io, std::size(io), ctx->stream);
    if (rc == GC_OK) rc = cot_recv_run(ctx, io[0].d.p, io[1].d.p, io[2].d.p, io[3].d.p, S, per);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), ctx->stream);
    return rc;
} catch (...) {
    return gc::on_exception();
}

// ---- bit-COT (ReceiveBits / SendBits, iknp.go:259-310, 554-620) per session: column 0 of the same matrix ------------------

namespace {

// the checks of a bits call on top of multi_call_args; *words = S * ceil(per / 64)
int bits_call_args(const gc_iknp_multi *h, bool receiver, size_t per, MultiSizes *z, size_t *words) {
    int rc = multi_call_args(h, receiver, per, z);
    if (rc != GC_OK) return rc;
    *words = h->S * (size_t)iknp_bits_words(per);  // below S * per + S, which multi_sizes has bounded
    return GC_OK;
}

// stride 0 or >= W, and the span of words the call reads fits size_t in bytes
bool bits_choice_span(size_t S, size_t per, size_t stride, size_t *span) {
    if (!iknp_bits_stride_ok(stride, per)) return false;
    if (stride && S - 1 > (SIZE_MAX / 16) / stride) return false;
    *span = (size_t)iknp_bits_choice_span(S, per, stride);
    return true;
}

// the bits operations on device pointers, as extend_run.  u_session, u_chunk: where the sender finds column 0 of chunk c of
// session s (launch_iknp_multi_send_bits)
int recv_bits_run(gc_iknp_multi *h, size_t per, const void *d_choices, size_t choice_stride, void *d_u_out, void *d_result) {
    GC_HIP(launch_iknp_multi_recv_bits(h->d_keys, h->pos, h->S, per, (const uint64_t *)d_choices, choice_stride,
                                       (uint8_t *)d_u_out, (uint64_t *)d_result, h->ctx->d_te0, h->ctx->stream));
    return GC_OK;
}
int send_bits_run(gc_iknp_multi *h, size_t per, const void *d_u_in, size_t u_session, size_t u_chunk, void *d_result) {
    GC_HIP(launch_iknp_multi_send_bits(h->d_keys, h->d_delta, h->pos, h->S, per, (const uint8_t *)d_u_in, u_session, u_chunk,
                                       (uint64_t *)d_result, h->ctx->d_te0, h->ctx->stream));
    return GC_OK;
}

}  // namespace

int gc_iknp_multi_receive_bits_dev(gc_iknp_multi *h, const void *d_choices, size_t choice_stride, size_t per, void *d_u_out,
                                   void *d_result) {
    MultiSizes z;
    size_t words, span;
    int rc = bits_call_args(h, true, per, &z, &words);
    if (rc != GC_OK) return rc;
    if (per == 0) return GC_OK;
    if (!d_choices || !d_u_out || !d_result || !bits_choice_span(h->S, per, choice_stride, &span)) return GC_E_ARG;
    gc_ctx *ctx = h->ctx;
    GC_HIP(hipSetDevice(ctx->device));
    rc = recv_bits_run(h, per, d_choices, choice_stride, d_u_out, d_result);
    if (rc == GC_OK) h->pos += iknp_multi_advance(per);
    return rc;
}

int gc_iknp_multi_send_bits_dev(gc_iknp_multi *h, const void *d_u_in, size_t per, void *d_result) {
    MultiSizes z;
    size_t words;
    int rc = bits_call_args(h, false, per, &z, &words);
    if (rc != GC_OK) return rc;
    if (per == 0) return GC_OK;
    if (!d_u_in || !d_result) return GC_E_ARG;
    gc_ctx *ctx = h->ctx;
    GC_HIP(hipSetDevice(ctx->device));
    rc = send_bits_run(h, per, d_u_in, (size_t)iknp_multi_u_bytes(per), 8192, d_result);
    if (rc == GC_OK) h->pos += iknp_multi_advance(per);
    return rc;
}

int gc_iknp_multi_receive_bits(gc_iknp_multi *h, const uint64_t *choices, size_t choice_stride, size_t per, uint8_t *u_out,
                               uint64_t *result) try {
    MultiSizes z;
    size_t words, span;
    int rc = bits_call_args(h, true, per, &z, &words);
    if (rc != GC_OK) return rc;
    if (per == 0) return GC_OK;
    if (!choices || !u_out || !result || !bits_choice_span(h->S, per, choice_stride, &span)) return GC_E_ARG;
    gc_ctx *ctx = h->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    Staged io[] = {{choices, nullptr, span * 8}, {nullptr, u_out, z.u}, {nullptr, result, words * 8}};
    rc = stage_in(io, std::size(io), ctx->stream);
    if (rc == GC_OK) rc = recv_bits_run(h, per, io[0].d.p, choice_stride, io[1].d.p, io[2].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), ctx->stream);
    if (rc == GC_OK) h->pos += iknp_multi_advance(per);
    return rc;
} catch (...) {
    return gc::on_exception();
}

int gc_iknp_multi_send_bits(gc_iknp_multi *h, const uint8_t *u_in, size_t u_len, size_t per, uint64_t *result) try {
    MultiSizes z;
    size_t words;
    int rc = bits_call_args(h, false, per, &z, &words);
    if (rc != GC_OK) return rc;
    if (per == 0) return GC_OK;
    if (!u_in || !result || u_len != z.u) return GC_E_ARG;  // "invalid chunk size" (iknp.go:270-272)
    // column 0 is all the kernel reads: a session's ceil(per / 8) bytes in a row, 1 / 128 of the message
    const size_t row = (size_t)iknp_bits_col0_row(per), ub = (size_t)iknp_multi_u_bytes(per), bytes = (per + 7) / 8;
    std::vector<uint8_t> col0(h->S * row, 0);
    for (size_t s = 0; s < h->S; s++)
        for (size_t at = 0; at < bytes; at += 64)
            memcpy(&col0[s * row + at], u_in + s * ub + (at / 64) * 8192, std::min<size_t>(64, bytes - at));
    gc_ctx *ctx = h->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    Staged io[] = {{col0.data(), nullptr, col0.size()}, {nullptr, result, words * 8}};
    rc = stage_in(io, std::size(io), ctx->stream);
    if (rc == GC_OK) rc = send_bits_run(h, per, io[0].d.p, row, 64, io[1].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), ctx->stream);
    if (rc == GC_OK) h->pos += iknp_multi_advance(per);
    return rc;
} catch (...) {
    return gc::on_exception();
}

// ---- tripleBatch's local words for S peers in one launch each (triples.go:340-349, 362-364, 387-389) ----------------------

static bool fold_sizes(size_t S, size_t words) { return S != 0 && (!words || S <= (SIZE_MAX / 8) / words); }

int gc_gmw_triples_multi_sender_u_dev(gc_iknp_multi *sender, const void *d_a, void *d_u, size_t words) {
    if (!sender || sender->receiver || !fold_sizes(sender->S, words)) return GC_E_ARG;
    if (!words) return GC_OK;
    if (!d_a || !d_u) return GC_E_ARG;
    gc_ctx *ctx = sender->ctx;
    GC_HIP(hipSetDevice(ctx->device));
    GC_HIP(launch_gmw_multi_sender_u(sender->d_delta, (const uint64_t *)d_a, (uint64_t *)d_u, sender->S, words, ctx->stream));
    return GC_OK;
}

int gc_gmw_triples_multi_sender_fold_dev(gc_ctx *ctx, const void *d_s, const void *d_u, const void *d_v, void *d_c, size_t S,
                                         size_t words) {
    if (!ctx || !fold_sizes(S, words)) return GC_E_ARG;
    if (!words) return GC_OK;
    if (!d_s || !d_u || !d_v || !d_c) return GC_E_ARG;
    GC_HIP(hipSetDevice(ctx->device));
    GC_HIP(launch_gmw_multi_sender_fold((const uint64_t *)d_s, (const uint64_t *)d_u, (const uint64_t *)d_v, (uint64_t *)d_c, S,
                                        words, ctx->stream));
    return GC_OK;
}

int gc_gmw_triples_multi_receiver_fold_dev(gc_ctx *ctx, const void *d_r, void *d_c, size_t S, size_t words) {
    if (!ctx || !fold_sizes(S, words)) return GC_E_ARG;
    if (!words) return GC_OK;
    if (!d_r || !d_c) return GC_E_ARG;
    GC_HIP(hipSetDevice(ctx->device));
    GC_HIP(launch_gmw_multi_receiver_fold((const uint64_t *)d_r, (uint64_t *)d_c, S, words, ctx->stream));
    return GC_OK;
}

}  // extern "C"
