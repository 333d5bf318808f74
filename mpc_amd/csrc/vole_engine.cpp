// vole_engine.cpp — C ABI of the packed-IKNP VOLE (gcengine.h: gc_vole_*): the per-label work of (*Sender).Mul
// (vole/vole.go:58-97) and the reduction of (*Receiver).Mul (vole.go:182-187).  The IKNP calls, the p2p messages and
// their length checks stay with the caller; vole_kernels.hip is the device side.
#include <new>

#include "engine.h"

using namespace gc;

namespace {

// m elements of 32 bytes: refuse an m whose byte count does not fit size_t
bool bytes_fit(size_t m) { return m <= SIZE_MAX / 32; }

}  // namespace

extern "C" {

int gc_vole_sender_mul_dev(gc_ctx *ctx, const uint8_t *p, const void *d_labels, const void *d_x, const void *d_y_msg,
                           size_t m, void *d_r_out, void *d_u_msg_out) {
    if (!ctx || !p || (m && (!d_labels || !d_x || !d_y_msg || !d_r_out || !d_u_msg_out)) || !bytes_fit(m)) return GC_E_ARG;
    VoleMod mod;
    if (!vole_mod_init(p, &mod)) return GC_E_ARG;
    if (m == 0) return GC_OK;
    GC_HIP(hipSetDevice(ctx->device));
    launch_vole_sender(mod, (const uint4 *)d_labels, (const uint4 *)d_x, (const uint4 *)d_y_msg, m, (uint4 *)d_r_out,
                       (uint4 *)d_u_msg_out, ctx->d_te0, ctx->stream);
    GC_HIP(hipGetLastError());
    return GC_OK;
}

int gc_vole_receiver_reduce_dev(gc_ctx *ctx, const uint8_t *p, const void *d_u_msg, size_t m, void *d_u_out) {
    if (!ctx || !p || (m && (!d_u_msg || !d_u_out)) || !bytes_fit(m)) return GC_E_ARG;
    VoleMod mod;
    if (!vole_mod_init(p, &mod)) return GC_E_ARG;
    if (m == 0) return GC_OK;
    GC_HIP(hipSetDevice(ctx->device));
    launch_vole_receiver(mod, (const uint4 *)d_u_msg, m, (uint4 *)d_u_out, ctx->stream);
    GC_HIP(hipGetLastError());
    return GC_OK;
}

int gc_vole_sender_mul(gc_ctx *ctx, const uint8_t *p, const gc_label *labels, const uint8_t *x, const uint8_t *y_msg,
                       size_t m, uint8_t *r_out, uint8_t *u_msg_out) try {
    if (!ctx || !p || (m && (!labels || !x || !y_msg || !r_out || !u_msg_out)) || !bytes_fit(m)) return GC_E_ARG;
    VoleMod mod;
    if (!vole_mod_init(p, &mod)) return GC_E_ARG;
    if (m == 0) return GC_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    DevBuf d_lab, d_x, d_y, d_r, d_u;
    GC_HIP(d_lab.alloc(m * 16));
    GC_HIP(d_x.alloc(m * 32));
    GC_HIP(d_y.alloc(m * 32));
    GC_HIP(d_r.alloc(m * 32));
    GC_HIP(d_u.alloc(m * 32));
    hipStream_t s = ctx->stream;
    GC_HIP(hipMemcpyAsync(d_lab.p, labels, m * 16, hipMemcpyHostToDevice, s));
    GC_HIP(hipMemcpyAsync(d_x.p, x, m * 32, hipMemcpyHostToDevice, s));
    GC_HIP(hipMemcpyAsync(d_y.p, y_msg, m * 32, hipMemcpyHostToDevice, s));
    launch_vole_sender(mod, (const uint4 *)d_lab.p, (const uint4 *)d_x.p, (const uint4 *)d_y.p, m, (uint4 *)d_r.p,
                       (uint4 *)d_u.p, ctx->d_te0, s);
    GC_HIP(hipGetLastError());
    GC_HIP(hipMemcpyAsync(r_out, d_r.p, m * 32, hipMemcpyDeviceToHost, s));
    GC_HIP(hipMemcpyAsync(u_msg_out, d_u.p, m * 32, hipMemcpyDeviceToHost, s));
    GC_HIP(hipStreamSynchronize(s));
    return GC_OK;
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
    DevBuf d_u;
    GC_HIP(d_u.alloc(m * 32));
    hipStream_t s = ctx->stream;
    GC_HIP(hipMemcpyAsync(d_u.p, u_msg, m * 32, hipMemcpyHostToDevice, s));
    launch_vole_receiver(mod, (const uint4 *)d_u.p, m, (uint4 *)d_u.p, s);
    GC_HIP(hipGetLastError());
    GC_HIP(hipMemcpyAsync(u_out, d_u.p, m * 32, hipMemcpyDeviceToHost, s));
    GC_HIP(hipStreamSynchronize(s));
    return GC_OK;
} catch (...) {
    return gc::on_exception();
}

}  // extern "C"
