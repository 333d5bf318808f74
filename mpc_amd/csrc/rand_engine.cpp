// rand_engine.cpp — C ABI of the device random streams (gcengine.h: gc_rand_*): S AES-CTR keystreams, one per
// session, expanded where their bytes are consumed.  The streams and every piece of their arithmetic are rand_ctr.h's;
// rand_kernels.hip is the device side.  The handle holds the expanded seeds and one byte position for all S streams; a call
// is one launch on the ctx stream with the position as a kernel argument.  The host form is staging (host_staging.h) around
// the operation of the _dev form.
// The _cur calls take the positions from a caller-owned device array instead, one per session, which the kernels of
// rand_cursor_kernels.hip read and advance: they leave h->pos alone and, with nothing of the call in a kernel argument that a
// replay would have to change, are legal inside a capture.  crand.Int's arithmetic is rand_int.h's.
#include <new>

#include "engine.h"
#include "rand_int.h"

using namespace gc;

struct gc_rand {
    gc_ctx *ctx = nullptr;
    size_t S = 0, keylen = 0;
    int rounds = 0;
    uint32_t *d_rk = nullptr;  // [S][4 (rounds + 1)] plain round keys
    RandCtr *d_iv = nullptr;   // [S]
    uint64_t pos = 0;          // bytes every stream has given out
};

namespace {

void rand_release(gc_rand *h) {
    if (h->d_rk) (void)hipFree(h->d_rk);
    if (h->d_iv) (void)hipFree(h->d_iv);
    delete h;
}

// the schedules of S seeds, from host arrays (staged) or device arrays; waits for the ctx stream: the caller's arrays are
// free again on return
int rand_expand(gc_rand *h, const void *seeds, const void *ivs, bool dev) {
    gc_ctx *ctx = h->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    GC_HIP(hipMalloc((void **)&h->d_rk, h->S * 4 * (size_t)(h->rounds + 1) * sizeof(uint32_t)));
    GC_HIP(hipMalloc((void **)&h->d_iv, h->S * sizeof(RandCtr)));
    Staged io[] = {{dev ? nullptr : seeds, nullptr, dev ? 0 : h->S * h->keylen}, {dev ? nullptr : ivs, nullptr, dev || !ivs ? 0 : h->S * 16}};
    int rc = stage_in(io, 2, ctx->stream);
    if (rc != GC_OK) return rc;
    const void *d_seeds = dev ? seeds : io[0].d.p, *d_ivs = !ivs ? nullptr : dev ? ivs : io[1].d.p;
    GC_HIP(launch_rand_expand((const uint8_t *)d_seeds, h->rounds, (const uint8_t *)d_ivs, h->S, ctx->d_te0, h->d_rk, h->d_iv,
                              ctx->stream));
    return stage_out(io, 2, ctx->stream);  // (nothing to copy back: the one wait)
}

gc_rand *rand_create(gc_ctx *ctx, const void *seeds, size_t keylen, const void *ivs, size_t S, bool dev, int *status) try {
    int rc = GC_OK;
    gc_rand *h = nullptr;
    if (!ctx || !seeds || S == 0 || S > SIZE_MAX / 256) {
        rc = GC_E_ARG;
    } else if (keylen != 16 && keylen != 24 && keylen != 32) {
        rc = GC_E_KEYSIZE;
    } else if (ctx->capturing) {
        rc = GC_E_ARG;  // allocates and waits: not between gc_ctx_capture_begin and _end
    } else if (!(h = new (std::nothrow) gc_rand)) {
        rc = GC_E_NOMEM;
    } else {
        h->ctx = ctx;
        h->S = S;
        h->keylen = keylen;
        h->rounds = (int)(keylen / 4) + 6;
        rc = rand_expand(h, seeds, ivs, dev);
        if (rc != GC_OK) {
            (void)hipStreamSynchronize(ctx->stream);  // the expansion may be queued on what is freed next
            rand_release(h);
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

// the checks of a draw of n > 0 bytes per stream into slots of `stride` bytes
int draw_args(const gc_rand *h, uint64_t n, size_t stride) {
    if (stride < n || !rand_range_ok(h->pos, n)) return GC_E_ARG;
    if (h->S - 1 > (SIZE_MAX - (size_t)n) / stride) return GC_E_ARG;  // the last slot ends past size_t
    // the position is a kernel argument and advances with every call: a replayed capture would reuse it
    if (h->ctx->capturing) return GC_E_ARG;
    return GC_OK;
}

// The operations on device pointers, the device set: what a _dev form does behind its argument checks.  The position is the
// caller's to advance.
int fill_run(gc_rand *h, size_t nbytes, void *d_out, size_t stride) {
    GC_HIP(launch_rand_fill(h->rounds, h->d_rk, h->d_iv, h->S, h->pos, nbytes, (uint8_t *)d_out, stride, h->ctx->d_te0,
                            h->ctx->stream));
    return GC_OK;
}

// ---- per-session cursors ----

struct CurStatus {
    uint64_t bad, lowest;  // what d_status holds
};

bool misaligned8(const void *p) { return ((uintptr_t)p & 7u) != 0; }

// the checks of a cursor fill of n > 0 bytes; nothing is launched or changed where they fail
int fill_cur_args(const gc_rand *h, const void *cur, uint64_t n, const void *out, size_t stride, const void *status, bool dev) {
    if (!cur || !out || (dev && !status) || stride < n) return GC_E_ARG;
    if (dev && (misaligned8(cur) || misaligned8(status))) return GC_E_ARG;
    if (h->S - 1 > (SIZE_MAX - (size_t)n) / stride) return GC_E_ARG;  // the last slot ends past size_t
    return GC_OK;
}

// ... of `count` > 0 scalars below max; the shape of max on the way
int scalars_cur_args(const gc_rand *h, const void *cur, const uint8_t *max, size_t count, const void *out, const void *status,
                     bool dev, RandIntShape &shape) {
    if (!cur || !max || !out || (dev && !status)) return GC_E_ARG;
    if (dev && (misaligned8(cur) || misaligned8(status))) return GC_E_ARG;
    if (count > SIZE_MAX / 32 / h->S) return GC_E_ARG;  // S * count * 32 past size_t
    return rand_int_shape(max, shape) ? GC_OK : GC_E_ARG;  // max of 0 or 1
}

int fill_cur_run(gc_rand *h, void *d_cur, size_t nbytes, void *d_out, size_t stride, void *d_status) {
    GC_HIP(launch_rand_cur_fill(h->rounds, h->d_rk, h->d_iv, h->S, (uint64_t *)d_cur, nbytes, (uint8_t *)d_out, stride,
                                (uint64_t *)d_status, h->ctx->d_te0, h->ctx->stream));
    return GC_OK;
}

int scalars_cur_run(gc_rand *h, void *d_cur, const RandIntShape &shape, size_t count, void *d_out, void *d_status) {
    GC_HIP(launch_rand_cur_scalars(h->rounds, h->d_rk, h->d_iv, h->S, (uint64_t *)d_cur, shape, count, (uint8_t *)d_out,
                                   (uint64_t *)d_status, h->ctx->d_te0, h->ctx->stream));
    return GC_OK;
}

// A host form: the cursors go in and come back, the output array goes in and comes back whole (a bad session's part and the
// gaps between slots return as they came), the status block comes back.  `run` is the _dev operation on the device copies.
template <typename Run>
int cur_host_form(gc_rand *h, uint64_t *cur, uint8_t *out, size_t out_bytes, size_t *bad_session, Run run) {
    gc_ctx *ctx = h->ctx;
    if (ctx->capturing) return GC_E_ARG;  // allocates and waits
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    CurStatus st{0, 0};
    Staged io[] = {{cur, cur, h->S * sizeof(uint64_t)}, {out, out, out_bytes}, {nullptr, &st, sizeof st}};
    int rc = stage_in(io, 3, ctx->stream);
    if (rc == GC_OK) rc = run(io[0].d.p, io[1].d.p, io[2].d.p);
    if (rc == GC_OK) rc = stage_out(io, 3, ctx->stream);
    if (rc != GC_OK || st.bad == 0) return rc;
    if (bad_session) *bad_session = (size_t)st.lowest;
    return GC_E_ARG;
}

}  // namespace

extern "C" {

gc_rand *gc_rand_create(gc_ctx *ctx, const uint8_t *seeds, size_t keylen, const uint8_t *ivs, size_t S, int *status) {
    return rand_create(ctx, seeds, keylen, ivs, S, false, status);
}

gc_rand *gc_rand_create_dev(gc_ctx *ctx, const void *d_seeds, size_t keylen, const void *d_ivs, size_t S, int *status) {
    return rand_create(ctx, d_seeds, keylen, d_ivs, S, true, status);
}

void gc_rand_free(gc_rand *h) {
    if (!h) return;
    if (h->ctx) {
        (void)hipSetDevice(h->ctx->device);
        (void)hipStreamSynchronize(h->ctx->stream);  // a _dev call may still read the schedules
    }
    rand_release(h);
}

int gc_rand_info(const gc_rand *h, size_t *S, size_t *keylen, uint64_t *pos) {
    if (!h) return GC_E_ARG;
    if (S) *S = h->S;
    if (keylen) *keylen = h->keylen;
    if (pos) *pos = h->pos;
    return GC_OK;
}

int gc_rand_seek(gc_rand *h, uint64_t pos) {
    if (!h) return GC_E_ARG;
    h->pos = pos;
    return GC_OK;
}

int gc_rand_fill_dev(gc_rand *h, size_t nbytes, void *d_out, size_t stride) {
    if (!h) return GC_E_ARG;
    if (nbytes == 0) return GC_OK;
    if (!d_out) return GC_E_ARG;
    int rc = draw_args(h, nbytes, stride);
    if (rc != GC_OK) return rc;
    GC_HIP(hipSetDevice(h->ctx->device));
    rc = fill_run(h, nbytes, d_out, stride);
    if (rc == GC_OK) h->pos += nbytes;
    return rc;
}

int gc_rand_fill(gc_rand *h, size_t nbytes, uint8_t *out, size_t stride) try {
    if (!h) return GC_E_ARG;
    if (nbytes == 0) return GC_OK;
    if (!out) return GC_E_ARG;
    int rc = draw_args(h, nbytes, stride);
    if (rc != GC_OK || h->S > SIZE_MAX / nbytes) return GC_E_ARG;
    gc_ctx *ctx = h->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    // the device copy is packed [S][nbytes]; a host array with gaps gets its rows one by one, the gaps untouched
    const bool packed = stride == nbytes;
    Staged io[] = {{nullptr, packed ? out : nullptr, packed ? h->S * nbytes : 0, h->S * nbytes}};
    rc = stage_in(io, 1, ctx->stream);
    if (rc == GC_OK) rc = fill_run(h, nbytes, io[0].d.p, nbytes);
    if (rc == GC_OK && !packed)
        GC_HIP(hipMemcpy2DAsync(out, stride, io[0].d.p, nbytes, nbytes, h->S, hipMemcpyDeviceToHost, ctx->stream));
    if (rc == GC_OK) rc = stage_out(io, 1, ctx->stream);
    if (rc == GC_OK) h->pos += nbytes;
    return rc;
} catch (...) {
    return gc::on_exception();
}

int gc_rand_gmw_shares_dev(gc_rand *h, size_t words, void *d_a, void *d_b) {
    if (!h) return GC_E_ARG;
    if (words == 0) return GC_OK;
    if (!d_a || !d_b || (h->pos & 15u) || words > SIZE_MAX / 16) return GC_E_ARG;
    int rc = draw_args(h, 16 * (uint64_t)words, 16 * words);
    if (rc != GC_OK) return rc;
    GC_HIP(hipSetDevice(h->ctx->device));
    GC_HIP(launch_rand_gmw_shares(h->rounds, h->d_rk, h->d_iv, h->S, h->pos, words, (uint64_t *)d_a, (uint64_t *)d_b,
                                  h->ctx->d_te0, h->ctx->stream));
    h->pos += 16 * (uint64_t)words;
    return GC_OK;
}

int gc_rand_cur_set_dev(gc_rand *h, void *d_cur, uint64_t pos) {
    if (!h || !d_cur || misaligned8(d_cur)) return GC_E_ARG;
    GC_HIP(hipSetDevice(h->ctx->device));
    GC_HIP(launch_rand_cur_set((uint64_t *)d_cur, h->S, pos, h->ctx->stream));
    return GC_OK;
}

int gc_rand_fill_cur_dev(gc_rand *h, void *d_cur, size_t nbytes, void *d_out, size_t stride, void *d_status) {
    if (!h) return GC_E_ARG;
    if (nbytes == 0) return GC_OK;
    int rc = fill_cur_args(h, d_cur, nbytes, d_out, stride, d_status, true);
    if (rc != GC_OK) return rc;
    GC_HIP(hipSetDevice(h->ctx->device));
    return fill_cur_run(h, d_cur, nbytes, d_out, stride, d_status);
}

int gc_rand_scalars_cur_dev(gc_rand *h, void *d_cur, const uint8_t max[32], size_t count, void *d_out, void *d_status) {
    if (!h) return GC_E_ARG;
    if (count == 0) return GC_OK;
    RandIntShape shape;
    int rc = scalars_cur_args(h, d_cur, max, count, d_out, d_status, true, shape);
    if (rc != GC_OK) return rc;
    GC_HIP(hipSetDevice(h->ctx->device));
    return scalars_cur_run(h, d_cur, shape, count, d_out, d_status);
}

int gc_rand_fill_cur(gc_rand *h, uint64_t *cur, size_t nbytes, uint8_t *out, size_t stride, size_t *bad_session) try {
    if (!h) return GC_E_ARG;
    if (nbytes == 0) return GC_OK;
    int rc = fill_cur_args(h, cur, nbytes, out, stride, nullptr, false);
    if (rc != GC_OK) return rc;
    return cur_host_form(h, cur, out, (h->S - 1) * stride + nbytes, bad_session, [&](void *d_cur, void *d_out, void *d_status) {
        return fill_cur_run(h, d_cur, nbytes, d_out, stride, d_status);
    });
} catch (...) {
    return gc::on_exception();
}

int gc_rand_scalars_cur(gc_rand *h, uint64_t *cur, const uint8_t max[32], size_t count, uint8_t *out, size_t *bad_session) try {
    if (!h) return GC_E_ARG;
    if (count == 0) return GC_OK;
    RandIntShape shape;
    int rc = scalars_cur_args(h, cur, max, count, out, nullptr, false, shape);
    if (rc != GC_OK) return rc;
    return cur_host_form(h, cur, out, h->S * count * 32, bad_session, [&](void *d_cur, void *d_out, void *d_status) {
        return scalars_cur_run(h, d_cur, shape, count, d_out, d_status);
    });
} catch (...) {
    return gc::on_exception();
}

}  // extern "C"
