// vole_engine.cpp — C ABI of the packed-IKNP VOLE (gcengine.h: gc_vole_*): the per-label work of (*Sender).Mul
// (vole/vole.go:58-97) and the reduction of (*Receiver).Mul (vole.go:182-187).  The IKNP calls, the p2p messages and
// their length checks stay with the caller; vole_kernels.hip is the device side.  A host form is staging (host_staging.h)
// around the operation of its _dev form.
#include <iterator>
#include <new>

#include "engine.h"

using namespace gc;

namespace {

// m elements of 32 bytes: refuse an m whose byte count does not fit size_t
bool bytes_fit(size_t m) { return m <= SIZE_MAX / 32; }

// The operations on device pointers, the device set: what a _dev form does behind its argument checks
int sender_run(gc_ctx *ctx, const VoleMod &mod, const void *d_labels, const void *d_x, const void *d_y_msg, size_t m,
               void *d_r_out, void *d_u_msg_out) {
    GC_HIP(launch_vole_sender(mod, (const uint4 *)d_labels, (const uint4 *)d_x, (const uint4 *)d_y_msg, m, (uint4 *)d_r_out,
                              (uint4 *)d_u_msg_out, ctx->d_te0, ctx->stream));
    return GC_OK;
}
int receiver_run(gc_ctx *ctx, const VoleMod &mod, const void *d_u_msg, size_t m, void *d_u_out) {
    GC_HIP(launch_vole_receiver(mod, (const uint4 *)d_u_msg, m, (uint4 *)d_u_out, ctx->stream));
    return GC_OK;
}

}  // namespace

extern "C" {

int gc_vole_sender_mul_dev(gc_ctx *ctx, const uint8_t *p, const void *d_labels, const void *d_x, const void *d_y_msg,
                           size_t m, void *d_r_out, void *d_u_msg_out) {
    if (!ctx || !p || (m && (!d_labels || !d_x || !d_y_msg || !d_r_out || !d_u_msg_out)) || !bytes_fit(m)) return GC_E_ARG;
    VoleMod mod;
    if (!vole_mod_init(p, &mod)) return GC_E_ARG;
    if (m == 0) return GC_OK;
    GC_HIP(hipSetDevice(ctx->device));
    return sender_run(ctx, mod, d_labels, d_x, d_y_msg, m, d_r_out, d_u_msg_out);
}

int gc_vole_receiver_reduce_dev(gc_ctx *ctx, const uint8_t *p, const void *d_u_msg, size_t m, void *d_u_out) {
    if (!ctx || !p || (m && (!d_u_msg || !d_u_out)) || !bytes_fit(m)) return GC_E_ARG;
    VoleMod mod;
    if (!vole_mod_init(p, &mod)) return GC_E_ARG;
    if (m == 0) return GC_OK;
    GC_HIP(hipSetDevice(ctx->device));
    return receiver_run(ctx, mod, d_u_msg, m, d_u_out);
}

int gc_vole_sender_mul(gc_ctx *ctx, const uint8_t *p, const gc_label *labels, const uint8_t *x, const uint8_t *y_msg,
                       size_t m, uint8_t *r_out, uint8_t *u_msg_out) try {
    if (!ctx || !p || (m && (!labels || !x || !y_msg || !r_out || !u_msg_out)) || !bytes_fit(m)) return GC_E_ARG;
    VoleMod mod;
    if (!vole_mod_init(p, &mod)) return GC_E_ARG;
    if (m == 0) return GC_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    Staged io[] = {{labels, nullptr, m * 16}, {x, nullptr, m * 32}, {y_msg, nullptr, m * 32}, {nullptr, r_out, m * 32},
                   {nullptr, u_msg_out, m * 32}};
    int rc = stage_in(io, std::size(io), ctx->stream);
    if (rc == GC_OK) rc = sender_run(ctx, mod, io[0].d.p, io[1].d.p, io[2].d.p, m, io[3].d.p, io[4].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), ctx->stream);
    return rc;
} catch (...) {
    return gc::on_exception();
}

int gc_vole_receiver_reduce(gc_ctx *ctx, const uint8_t *p, const uint8_t *u_msg, size_t m, uint8_t *u_out) try {
    if (!ctx || !p || (m && (!u_msg || !u_out)) || !bytes_fit(m)) return GC_E_ARG;
    VoleMod mod;
    if (!vole_mod_init(p, &mod)) return GC_E_ARG;
    if (m == 0) return GC_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    Staged io[] = {{u_msg, u_out, m * 32}};  // reduced in place
    int rc = stage_in(io, std::size(io), ctx->stream);
    if (rc == GC_OK) rc = receiver_run(ctx, mod, io[0].d.p, m, io[0].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), ctx->stream);
    return rc;
} catch (...) {
    return gc::on_exception();
}

}  // extern "C"
