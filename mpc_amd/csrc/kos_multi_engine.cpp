// kos_multi_engine.cpp — C ABI of the multi-session KOS check (gc_kos_multi_*): the tags and the check of the malicious IKNP
// variant for S sessions of `per` OTs each, session-major, one kernel per call (kos_multi_kernels.hip; layouts: kos_multi.h).
// The _dev forms only reset the status block and launch: no allocation, no wait, nothing copied to the host, so they may be
// captured.  A host form is staging (host_staging.h) around the operation of its _dev form.
#include <algorithm>
#include <iterator>
#include <new>
#include <vector>

#include "engine.h"
#include "kos_multi.h"

using namespace gc;

namespace {

constexpr size_t kLabel = sizeof(gc_label);

// the byte counts of a call; false: one of them does not fit size_t
struct KosSizes {
    size_t n, choice_row;  // S * per; bytes of one session's packed choice bits
};
bool kos_sizes(size_t S, size_t per, KosSizes *z) {
    if (per && S > SIZE_MAX / per) return false;
    z->n = S * per;
    if (z->n > SIZE_MAX / 64 || S > SIZE_MAX / (64 * kKosCvLabels)) return false;  // labels, tags and the choice vectors
    z->choice_row = (size_t)kos_multi_choice_row(per);
    if (z->choice_row && S > SIZE_MAX / z->choice_row) return false;
    return true;
}

bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int tags_run(gc_ctx *ctx, const void *d_seed2, const void *d_result, const void *d_choice, const void *d_cv, const void *d_bcv,
             size_t S, size_t per, void *d_tags) {
    GC_HIP(launch_kos_multi_tags((const uint4 *)d_seed2, (const uint4 *)d_result, (const uint8_t *)d_choice, (const uint4 *)d_cv,
                                 (const uint8_t *)d_bcv, S, per, (uint4 *)d_tags, ctx->d_te0, ctx->stream));
    return GC_OK;
}

int check_run(gc_ctx *ctx, const void *d_seed2, const void *d_result, const void *d_cv, const void *d_delta, const void *d_tags,
              size_t S, size_t per, void *d_ok, void *d_status) {
    // the status block before the kernel: {0, ~0}
    GC_HIP(hipMemsetAsync(d_status, 0, 8, ctx->stream));
    GC_HIP(hipMemsetAsync((uint8_t *)d_status + 8, 0xff, 8, ctx->stream));
    GC_HIP(launch_kos_multi_check((const uint4 *)d_seed2, (const uint4 *)d_result, (const uint4 *)d_cv, (const uint4 *)d_delta,
                                  (const uint4 *)d_tags, S, per, (uint8_t *)d_ok, (unsigned long long *)d_status, ctx->d_te0,
                                  ctx->stream));
    return GC_OK;
}

}  // namespace

extern "C" {

int gc_kos_multi_receiver_tags_dev(gc_ctx *ctx, const void *d_seed2, const void *d_result, const void *d_choice_packed,
                                   const void *d_choice_vec, const void *d_bcv_packed, size_t S, size_t per, void *d_tags_out) {
    KosSizes z;
    if (!ctx || !kos_sizes(S, per, &z)) return GC_E_ARG;
    if (S == 0) return GC_OK;
    if (!d_seed2 || !d_choice_vec || !d_bcv_packed || !d_tags_out || (per && (!d_result || !d_choice_packed))) return GC_E_ARG;
    if (!aligned(d_seed2, 16) || !aligned(d_result, 16) || !aligned(d_choice_vec, 16) || !aligned(d_tags_out, 16))
        return GC_E_ARG;
    GC_HIP(hipSetDevice(ctx->device));
    return tags_run(ctx, d_seed2, d_result, d_choice_packed, d_choice_vec, d_bcv_packed, S, per, d_tags_out);
}

int gc_kos_multi_sender_check_dev(gc_ctx *ctx, const void *d_seed2, const void *d_result, const void *d_choice_vec,
                                  const void *d_delta, const void *d_tags, size_t S, size_t per, void *d_ok, void *d_status) {
    KosSizes z;
    if (!ctx || !kos_sizes(S, per, &z)) return GC_E_ARG;
    if (S == 0) return GC_OK;
    if (!d_seed2 || !d_choice_vec || !d_delta || !d_tags || !d_ok || !d_status || (per && !d_result)) return GC_E_ARG;
    if (!aligned(d_seed2, 16) || !aligned(d_result, 16) || !aligned(d_choice_vec, 16) || !aligned(d_delta, 16) ||
        !aligned(d_tags, 16) || !aligned(d_status, 8))
        return GC_E_ARG;
    GC_HIP(hipSetDevice(ctx->device));
    return check_run(ctx, d_seed2, d_result, d_choice_vec, d_delta, d_tags, S, per, d_ok, d_status);
}

int gc_kos_multi_receiver_tags(gc_ctx *ctx, const gc_label *seed2, const gc_label *result, const uint8_t *b,
                               const gc_label *choice_vec, const uint8_t *bcv, size_t S, size_t per, gc_label *tags_out) try {
    KosSizes z;
    if (!ctx || !kos_sizes(S, per, &z)) return GC_E_ARG;
    if (S == 0) return GC_OK;
    if (!seed2 || !choice_vec || !bcv || !tags_out || (per && (!result || !b))) return GC_E_ARG;
    if (ctx->capturing) return GC_E_ARG;  // allocates and waits
    const std::vector<uint8_t> bits = pack_rows(b, S, per, z.choice_row), cbits = pack_rows(bcv, S, kKosCvLabels, kKosBcvRow);
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    Staged io[] = {{seed2, nullptr, S * kLabel}, {result, nullptr, z.n * kLabel}, {bits.data(), nullptr, bits.size()},
                   {choice_vec, nullptr, S * kKosCvLabels * kLabel}, {cbits.data(), nullptr, cbits.size()},
                   {nullptr, tags_out, S * 3 * kLabel}};
    int rc = stage_in(io, std::size(io), ctx->stream);
    if (rc == GC_OK) rc = tags_run(ctx, io[0].d.p, io[1].d.p, io[2].d.p, io[3].d.p, io[4].d.p, S, per, io[5].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), ctx->stream);
    return rc;
} catch (...) {
    return gc::on_exception();
}

int gc_kos_multi_sender_check(gc_ctx *ctx, const gc_label *seed2, const gc_label *result, const gc_label *choice_vec,
                              const gc_label *delta, const gc_label *tags, size_t S, size_t per, uint8_t *ok_out,
                              size_t *bad_session) try {
    KosSizes z;
    if (!ctx || !kos_sizes(S, per, &z)) return GC_E_ARG;
    if (S == 0) return GC_OK;
    if (!seed2 || !choice_vec || !delta || !tags || (!ok_out && !bad_session) || (per && !result)) return GC_E_ARG;
    if (ctx->capturing) return GC_E_ARG;  // allocates and waits
    std::vector<uint8_t> ok(S, 0);
    uint64_t status[2] = {0, 0};
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    Staged io[] = {{seed2, nullptr, S * kLabel}, {result, nullptr, z.n * kLabel},
                   {choice_vec, nullptr, S * kKosCvLabels * kLabel}, {delta, nullptr, S * kLabel},
                   {tags, nullptr, S * 3 * kLabel}, {nullptr, ok.data(), S}, {nullptr, status, sizeof status}};
    int rc = stage_in(io, std::size(io), ctx->stream);
    if (rc == GC_OK) rc = check_run(ctx, io[0].d.p, io[1].d.p, io[2].d.p, io[3].d.p, io[4].d.p, S, per, io[5].d.p, io[6].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), ctx->stream);
    if (rc != GC_OK) return rc;
    if (ok_out) std::copy(ok.begin(), ok.end(), ok_out);
    if (bad_session) *bad_session = status[0] ? (size_t)status[1] : (size_t)-1;
    return GC_OK;
} catch (...) {
    return gc::on_exception();
}

}  // extern "C"
