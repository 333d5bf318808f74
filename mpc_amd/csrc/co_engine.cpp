// co_engine.cpp — C ABI of the Chou-Orlandi base OT on P-256 (gcengine.h: gc_co_*): the per-OT work of ot/co_helpers.go
// (GenerateCOSenderSetup :77-101, EncryptCOCiphertexts :104-137, BuildCOChoices :140-177, DecryptCOCiphertexts :191-219).
// crand.Int, the framing and the p2p messages stay with the caller, who passes the scalars it drew; co_kernels.hip is the
// device side.  The session constants (a, A, AaInv) are host pointers in every form and are prepared here, on the host, with
// the arithmetic of p256.h that the kernels run: gc_co_sender_setup is two scalar multiplications per SESSION, not worth a
// launch.
//
// gc_co_base_*: the receiver's side of one session behind a handle that owns A's window table (co_table.h).  The tables are
// built here, on the host, for the reason above: the 252 dependent doublings of a table are a lone wave's work on the
// device, about 2 ms, and a fraction of that on a CPU core.  G's table is built once per process and uploaded once per ctx.
//
// gc_co_multi_*: S sessions per call (co_multi_kernels.hip).  The session constants are ARRAYS in device memory there, and
// the sender's setup runs on the device, one lane per session, from G's table.
#define GC_CO_TABLE_BUILD 1  // co_table.h: the host-side table build as well

#include <cstring>
#include <iterator>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "engine.h"
#include "sha2pc.h"

using namespace gc;

namespace {

// n OTs of at most 64 bytes per array: refuse an n whose byte count does not fit size_t
bool bytes_fit(size_t n) { return n <= SIZE_MAX / 64; }

// bytes per OT (or per session) of the arrays at the boundary
constexpr size_t kScalarBytes = 32, kPointBytes = sizeof(gc_p256_point), kWireBytes = sizeof(gc_wire), kCtBytes = 32,
                 kLabelBytes = sizeof(gc_label);

// the verdict on the launch just made
int launched() {
    GC_HIP(hipGetLastError());
    return GC_OK;
}

// A host form is staging (host_staging.h: Staged, stage_in, stage_out) around the operation of its _dev form.

Fe load_fe(const uint8_t *b) {
    Fe f;
    vole_load_be(b, f.v);
    return f;
}

// a point of the boundary -> Montgomery affine; false: not on the curve (infinity included)
bool load_point(const gc_p256_point *pt, Aff *q) { return pt_on_curve(load_fe(pt->x), load_fe(pt->y), *q); }

void store_point(const Jac &p, gc_p256_point *out) {
    Fe x, y;
    pt_to_affine(p, fe_inv(p.z), x, y);
    vole_store_be(x.v, out->x);
    vole_store_be(y.v, out->y);
}

Aff generator() {
    Aff g;
    g.x = fe_to_mont(p256_gx());
    g.y = fe_to_mont(p256_gy());
    g.inf = 0;
    return g;
}

// the sender's scalar mod N; false: a = 0 mod N
bool load_sender_scalar(const uint8_t *a, Fe *k) {
    *k = sc_reduce(load_fe(a));
    return !fe_is_zero(*k);
}

int sender_session(const uint8_t *a, const gc_p256_point *ainv, CoSender *ses) {
    Fe k;
    if (!load_sender_scalar(a, &k)) return GC_E_ARG;
    if (!load_point(ainv, &ses->ainv)) return GC_E_ARG;  // the caller's own constant, not a peer's point
    for (int j = 0; j < kVoleLimbs; j++) ses->a[j] = k.v[j];
    return GC_OK;
}

int receiver_session(const gc_p256_point *A, CoBase *base) {
    base->g = generator();
    return load_point(A, &base->a) ? GC_OK : GC_E_POINT;  // ensureOnCurve(Ax, Ay), co_helpers.go:144
}

// the status block of gc_co_sender_encrypt_dev before the kernel: {0, ~0}
hipError_t reset_status(void *d_status, hipStream_t s) {
    hipError_t e = hipMemsetAsync(d_status, 0, 8, s);
    if (e != hipSuccess) return e;
    return hipMemsetAsync((uint8_t *)d_status + 8, 0xff, 8, s);
}

// the generator's table, built by the first handle of the process
const std::vector<CoTabEntry> &g_table() {
    static std::vector<CoTabEntry> tab;
    static std::once_flag once;
    std::call_once(once, [] {
        std::vector<CoTabEntry> t(co_tab_entries(kCoTabWidthG));
        co_tab_build<kCoTabWidthG>(generator(), t.data());
        tab.swap(t);
    });
    return tab;
}

// a table into device memory, complete when the call returns (the source is pageable host memory)
int upload_table(gc_ctx *ctx, const std::vector<CoTabEntry> &tab, CoTabEntry **d_out) {
    void *d = nullptr;
    GC_HIP(hipMalloc(&d, tab.size() * sizeof(CoTabEntry)));
    hipError_t e = hipMemcpyAsync(d, tab.data(), tab.size() * sizeof(CoTabEntry), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipFree(d);
        GC_HIP(e);
    }
    *d_out = (CoTabEntry *)d;
    return GC_OK;
}

// G's table in the memory of this ctx: uploaded by the first caller (ctx->mu held, the device set), then kept until the ctx
// goes.  g: g_table(), built before the lock is taken
int ensure_g_table(gc_ctx *ctx, const std::vector<CoTabEntry> &g) {
    if (ctx->d_co_g_tab) return GC_OK;
    return upload_table(ctx, g, &ctx->d_co_g_tab);
}

}  // namespace

struct gc_co_base {
    gc_ctx *ctx = nullptr;
    Aff a;                      // the sender's point, for B = b * G + A
    CoTabEntry *d_tab = nullptr;  // A's table, width kCoTabWidthA
};

namespace {

int co_base_init(gc_co_base *h, gc_ctx *ctx) {
    std::vector<CoTabEntry> tab(co_tab_entries(kCoTabWidthA));
    co_tab_build<kCoTabWidthA>(h->a, tab.data());
    const std::vector<CoTabEntry> &g = g_table();
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    const int rc = ensure_g_table(ctx, g);
    if (rc != GC_OK) return rc;
    h->ctx = ctx;
    return upload_table(ctx, tab, &h->d_tab);
}

bool base_args(const gc_co_base *h, size_t n, bool pointers) { return h && (n == 0 || pointers) && bytes_fit(n); }

// The operations of the handle on device pointers, the device set: what a _dev form does behind its argument checks
int base_choices_run(gc_co_base *h, const void *d_scalars, const void *d_choice, size_t n, void *d_points_out) {
    launch_co_choices_tab(h->ctx->d_co_g_tab, h->a, (const uint4 *)d_scalars, (const uint8_t *)d_choice, n, (uint4 *)d_points_out,
                          h->ctx->stream);
    return launched();
}
int base_decrypt_run(gc_co_base *h, const void *d_scalars, const void *d_choice, const void *d_ct, size_t n, uint64_t id0,
                     void *d_labels_out) {
    launch_co_decrypt_tab(h->d_tab, (const uint4 *)d_scalars, (const uint8_t *)d_choice, (const uint4 *)d_ct, n, id0,
                          (uint4 *)d_labels_out, h->ctx->stream);
    return launched();
}

}  // namespace

extern "C" {

gc_co_base *gc_co_base_create(gc_ctx *ctx, const gc_p256_point *A, int *status) try {
    int rc = GC_OK;
    std::unique_ptr<gc_co_base> h;
    if (!ctx || !A) {
        rc = GC_E_ARG;
    } else if (ctx->capturing) {
        rc = GC_E_ARG;  // allocates and waits for the stream: not between gc_ctx_capture_begin and _end
    } else {
        h.reset(new gc_co_base);
        if (!load_point(A, &h->a)) rc = GC_E_POINT;  // ensureOnCurve(Ax, Ay), co_helpers.go:144
        if (rc == GC_OK) rc = co_base_init(h.get(), ctx);
    }
    if (status) *status = rc;
    return rc == GC_OK ? h.release() : nullptr;
} catch (...) {
    const int rc__ = gc::on_exception();
    if (status) *status = rc__;
    return nullptr;
}

void gc_co_base_free(gc_co_base *h) {
    if (!h) return;
    if (h->ctx) {
        (void)hipSetDevice(h->ctx->device);
        (void)hipStreamSynchronize(h->ctx->stream);  // a _dev call may still read the table
    }
    if (h->d_tab) (void)hipFree(h->d_tab);
    delete h;
}

int gc_co_base_choices_dev(gc_co_base *h, const void *d_scalars, const void *d_choice, size_t n, void *d_points_out) {
    if (!base_args(h, n, d_scalars && d_choice && d_points_out)) return GC_E_ARG;
    if (n == 0) return GC_OK;
    GC_HIP(hipSetDevice(h->ctx->device));
    return base_choices_run(h, d_scalars, d_choice, n, d_points_out);
}

int gc_co_base_decrypt_dev(gc_co_base *h, const void *d_scalars, const void *d_choice, const void *d_ct, size_t n,
                           uint64_t id0, void *d_labels_out) {
    if (!base_args(h, n, d_scalars && d_choice && d_ct && d_labels_out)) return GC_E_ARG;
    if (n == 0) return GC_OK;
    GC_HIP(hipSetDevice(h->ctx->device));
    return base_decrypt_run(h, d_scalars, d_choice, d_ct, n, id0, d_labels_out);
}

int gc_co_base_choices(gc_co_base *h, const uint8_t *scalars, const uint8_t *choice, size_t n, gc_p256_point *points_out) try {
    if (!base_args(h, n, scalars && choice && points_out)) return GC_E_ARG;
    if (n == 0) return GC_OK;
    gc_ctx *ctx = h->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    Staged io[] = {{scalars, nullptr, n * kScalarBytes}, {choice, nullptr, n}, {nullptr, points_out, n * kPointBytes}};
    int rc = stage_in(io, std::size(io), ctx->stream);
    if (rc == GC_OK) rc = base_choices_run(h, io[0].d.p, io[1].d.p, n, io[2].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), ctx->stream);
    return rc;
} catch (...) {
    return gc::on_exception();
}

int gc_co_base_decrypt(gc_co_base *h, const uint8_t *scalars, const uint8_t *choice, const uint8_t *ct, size_t n, uint64_t id0,
                       gc_label *labels_out) try {
    if (!base_args(h, n, scalars && choice && ct && labels_out)) return GC_E_ARG;
    if (n == 0) return GC_OK;
    gc_ctx *ctx = h->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    Staged io[] = {{scalars, nullptr, n * kScalarBytes}, {choice, nullptr, n}, {ct, nullptr, n * kCtBytes},
                   {nullptr, labels_out, n * kLabelBytes}};
    int rc = stage_in(io, std::size(io), ctx->stream);
    if (rc == GC_OK) rc = base_decrypt_run(h, io[0].d.p, io[1].d.p, io[2].d.p, n, id0, io[3].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), ctx->stream);
    return rc;
} catch (...) {
    return gc::on_exception();
}

int gc_co_sender_setup(const uint8_t *a, gc_p256_point *A_out, gc_p256_point *AaInv_out) {
    if (!a || !A_out || !AaInv_out) return GC_E_ARG;
    Fe k;
    if (!load_sender_scalar(a, &k)) return GC_E_ARG;
    store_point(pt_mul(k, generator()), A_out);  // A = a * G
    Aff A;
    if (!load_point(A_out, &A)) return GC_E_ARG;  // (cannot be: a != 0 mod N)
    const Jac aa = pt_mul(k, A);                  // a * A
    Fe x, y;
    pt_to_affine(aa, fe_inv(aa.z), x, y);
    vole_store_be(x.v, AaInv_out->x);
    vole_store_be(fe_neg(y).v, AaInv_out->y);     // p - y (co_helpers.go:90-91); y != 0 on a curve of odd order
    return GC_OK;
}

}  // extern "C"

namespace {

// The one-session operations on device pointers, the device set: what a _dev form does behind its checks
int encrypt_run(gc_ctx *ctx, const CoSender &ses, const void *d_points, const void *d_wires, size_t n, uint64_t id0, void *d_ct,
                void *d_status) {
    GC_HIP(reset_status(d_status, ctx->stream));
    launch_co_encrypt(ses, (const uint4 *)d_points, (const uint4 *)d_wires, n, id0, (uint4 *)d_ct,
                      (unsigned long long *)d_status, ctx->stream);
    return launched();
}
int choices_run(gc_ctx *ctx, const CoBase &base, const void *d_scalars, const void *d_choice, size_t n, void *d_points_out) {
    launch_co_choices(base, (const uint4 *)d_scalars, (const uint8_t *)d_choice, n, (uint4 *)d_points_out, ctx->stream);
    return launched();
}
int decrypt_run(gc_ctx *ctx, const CoBase &base, const void *d_scalars, const void *d_choice, const void *d_ct, size_t n,
                uint64_t id0, void *d_labels_out) {
    launch_co_decrypt(base, (const uint4 *)d_scalars, (const uint8_t *)d_choice, (const uint4 *)d_ct, n, id0,
                      (uint4 *)d_labels_out, ctx->stream);
    return launched();
}

}  // namespace

extern "C" {

int gc_co_sender_encrypt_dev(gc_ctx *ctx, const uint8_t *a, const gc_p256_point *AaInv, const void *d_points,
                             const void *d_wires, size_t n, uint64_t id0, void *d_ct, void *d_status) {
    if (!ctx || !a || !AaInv || (n && (!d_points || !d_wires || !d_ct || !d_status)) || !bytes_fit(n)) return GC_E_ARG;
    CoSender ses;
    const int rc = sender_session(a, AaInv, &ses);
    if (rc != GC_OK) return rc;
    if (n == 0) return GC_OK;
    GC_HIP(hipSetDevice(ctx->device));
    return encrypt_run(ctx, ses, d_points, d_wires, n, id0, d_ct, d_status);
}

int gc_co_receiver_choices_dev(gc_ctx *ctx, const gc_p256_point *A, const void *d_scalars, const void *d_choice, size_t n,
                               void *d_points_out) {
    if (!ctx || !A || (n && (!d_scalars || !d_choice || !d_points_out)) || !bytes_fit(n)) return GC_E_ARG;
    CoBase base;
    const int rc = receiver_session(A, &base);
    if (rc != GC_OK) return rc;
    if (n == 0) return GC_OK;
    GC_HIP(hipSetDevice(ctx->device));
    return choices_run(ctx, base, d_scalars, d_choice, n, d_points_out);
}

int gc_co_receiver_decrypt_dev(gc_ctx *ctx, const gc_p256_point *A, const void *d_scalars, const void *d_choice,
                               const void *d_ct, size_t n, uint64_t id0, void *d_labels_out) {
    if (!ctx || !A || (n && (!d_scalars || !d_choice || !d_ct || !d_labels_out)) || !bytes_fit(n)) return GC_E_ARG;
    CoBase base;
    const int rc = receiver_session(A, &base);
    if (rc != GC_OK) return rc;
    if (n == 0) return GC_OK;
    GC_HIP(hipSetDevice(ctx->device));
    return decrypt_run(ctx, base, d_scalars, d_choice, d_ct, n, id0, d_labels_out);
}

int gc_co_sender_encrypt(gc_ctx *ctx, const uint8_t *a, const gc_p256_point *AaInv, const gc_p256_point *points,
                         const gc_wire *wires, size_t n, uint64_t id0, uint8_t *ct, size_t *bad_index) try {
    if (!ctx || !a || !AaInv || (n && (!points || !wires || !ct)) || !bytes_fit(n)) return GC_E_ARG;
    CoSender ses;
    int rc = sender_session(a, AaInv, &ses);
    if (rc != GC_OK) return rc;
    if (n == 0) return GC_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    uint64_t status[2] = {0, 0};
    Staged io[] = {{points, nullptr, n * kPointBytes}, {wires, nullptr, n * kWireBytes}, {nullptr, ct, n * kCtBytes},
                   {nullptr, status, sizeof status}};
    rc = stage_in(io, std::size(io), ctx->stream);
    if (rc == GC_OK) rc = encrypt_run(ctx, ses, io[0].d.p, io[1].d.p, n, id0, io[2].d.p, io[3].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), ctx->stream);
    if (rc != GC_OK || !status[0]) return rc;
    if (bad_index) *bad_index = (size_t)status[1];
    return GC_E_POINT;  // ErrPointNotOnCurve (co_helpers.go:119-121)
} catch (...) {
    return gc::on_exception();
}

int gc_co_receiver_choices(gc_ctx *ctx, const gc_p256_point *A, const uint8_t *scalars, const uint8_t *choice, size_t n,
                           gc_p256_point *points_out) try {
    if (!ctx || !A || (n && (!scalars || !choice || !points_out)) || !bytes_fit(n)) return GC_E_ARG;
    CoBase base;
    int rc = receiver_session(A, &base);
    if (rc != GC_OK) return rc;
    if (n == 0) return GC_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    Staged io[] = {{scalars, nullptr, n * kScalarBytes}, {choice, nullptr, n}, {nullptr, points_out, n * kPointBytes}};
    rc = stage_in(io, std::size(io), ctx->stream);
    if (rc == GC_OK) rc = choices_run(ctx, base, io[0].d.p, io[1].d.p, n, io[2].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), ctx->stream);
    return rc;
} catch (...) {
    return gc::on_exception();
}

int gc_co_receiver_decrypt(gc_ctx *ctx, const gc_p256_point *A, const uint8_t *scalars, const uint8_t *choice,
                           const uint8_t *ct, size_t n, uint64_t id0, gc_label *labels_out) try {
    if (!ctx || !A || (n && (!scalars || !choice || !ct || !labels_out)) || !bytes_fit(n)) return GC_E_ARG;
    CoBase base;
    int rc = receiver_session(A, &base);
    if (rc != GC_OK) return rc;
    if (n == 0) return GC_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    Staged io[] = {{scalars, nullptr, n * kScalarBytes}, {choice, nullptr, n}, {ct, nullptr, n * kCtBytes},
                   {nullptr, labels_out, n * kLabelBytes}};
    rc = stage_in(io, std::size(io), ctx->stream);
    if (rc == GC_OK) rc = decrypt_run(ctx, base, io[0].d.p, io[1].d.p, io[2].d.p, n, id0, io[3].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), ctx->stream);
    return rc;
} catch (...) {
    return gc::on_exception();
}

}  // extern "C"

// ---- several sessions per call (gc_co_multi_*, co_multi_kernels.hip) ----------------------------------------------------

namespace {

// the constants of the group order N, for the a^2 mod N of k_co_multi_setup
const VoleMod &order_mod() {
    static const VoleMod mod = [] {
        uint8_t n_be[32];
        vole_store_be(p256_n().v, n_be);
        VoleMod m;
        (void)vole_mod_init(n_be, &m);  // N is odd and above 2
        return m;
    }();
    return mod;
}

// S sessions of per OTs each: false when S * per, or its byte count at 64 bytes per OT, does not fit size_t
bool multi_count(size_t S, size_t per, size_t *n) {
    if (per && S > SIZE_MAX / per) return false;
    *n = S * per;
    return bytes_fit(*n);
}

// the status block of the gc_co_multi_*_dev calls before the kernel: {0, ~0, 0, ~0}
hipError_t reset_status4(void *d_status, hipStream_t s) {
    hipError_t e = hipMemsetAsync(d_status, 0, 32, s);
    if (e == hipSuccess) e = hipMemsetAsync((uint8_t *)d_status + 8, 0xff, 8, s);
    if (e == hipSuccess) e = hipMemsetAsync((uint8_t *)d_status + 24, 0xff, 8, s);
    return e;
}

// G's table for a multi call, ctx->mu held and the device set: the first such call of a ctx uploads it, synchronously, which
// cannot happen between gc_ctx_capture_begin and _end
int multi_g_table_locked(gc_ctx *ctx, const std::vector<CoTabEntry> &g) {
    if (!ctx->d_co_g_tab && ctx->capturing) return GC_E_ARG;
    return ensure_g_table(ctx, g);
}
int multi_g_table(gc_ctx *ctx) {
    const std::vector<CoTabEntry> &g = g_table();
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    return multi_g_table_locked(ctx, g);
}

// the status block of a host form -> its return code.  A bad session wins over a bad point.
int multi_status(const uint64_t (&st)[4], int session_code, size_t *bad_index, size_t *bad_session) {
    if (st[0] && bad_index) *bad_index = (size_t)st[1];
    if (st[2]) {
        if (bad_session) *bad_session = (size_t)st[3];
        return session_code;
    }
    return st[0] ? GC_E_POINT : GC_OK;  // ErrPointNotOnCurve (co_helpers.go:119-121)
}

// The multi operations on device pointers, the device set and (setup, choices) G's table there: what a _dev form does behind
// its checks
int multi_setup_run(gc_ctx *ctx, const void *d_a, size_t S, void *d_A_out, void *d_AaInv_out, void *d_status) {
    GC_HIP(reset_status4(d_status, ctx->stream));
    launch_co_multi_setup(order_mod(), ctx->d_co_g_tab, (const uint4 *)d_a, S, (uint4 *)d_A_out, (uint4 *)d_AaInv_out,
                          (unsigned long long *)d_status, ctx->stream);
    return launched();
}
int multi_encrypt_run(gc_ctx *ctx, const void *d_a, const void *d_AaInv, const void *d_points, const void *d_wires, size_t S,
                      size_t per, uint64_t id0, void *d_ct, void *d_status) {
    GC_HIP(reset_status4(d_status, ctx->stream));
    launch_co_multi_encrypt((const uint4 *)d_a, (const uint4 *)d_AaInv, (const uint4 *)d_points, (const uint4 *)d_wires, S, per,
                            id0, (uint4 *)d_ct, (unsigned long long *)d_status, ctx->stream);
    return launched();
}
int multi_choices_run(gc_ctx *ctx, const void *d_A, const void *d_scalars, const void *d_choice, size_t S, size_t per,
                      void *d_points_out, void *d_status) {
    GC_HIP(reset_status4(d_status, ctx->stream));
    launch_co_multi_choices(ctx->d_co_g_tab, (const uint4 *)d_A, (const uint4 *)d_scalars, (const uint8_t *)d_choice, S, per,
                            (uint4 *)d_points_out, (unsigned long long *)d_status, ctx->stream);
    return launched();
}
int multi_decrypt_run(gc_ctx *ctx, const void *d_A, const void *d_scalars, const void *d_choice, const void *d_ct, size_t S,
                      size_t per, uint64_t id0, void *d_labels_out, void *d_status) {
    GC_HIP(reset_status4(d_status, ctx->stream));
    launch_co_multi_decrypt((const uint4 *)d_A, (const uint4 *)d_scalars, (const uint8_t *)d_choice, (const uint4 *)d_ct, S, per,
                            id0, (uint4 *)d_labels_out, (unsigned long long *)d_status, ctx->stream);
    return launched();
}

}  // namespace

// sha2pc.h: G's table on the device before the first round of a gc_sha2pc_* handle
int gc::co_multi_prepare(gc_ctx *ctx) try {
    return ctx ? multi_g_table(ctx) : GC_E_ARG;
} catch (...) {
    return gc::on_exception();
}

extern "C" {

int gc_co_multi_sender_setup_dev(gc_ctx *ctx, const void *d_a, size_t S, void *d_A_out, void *d_AaInv_out, void *d_status) try {
    if (!ctx || (S && (!d_a || !d_A_out || !d_AaInv_out || !d_status)) || !bytes_fit(S)) return GC_E_ARG;
    if (S == 0) return GC_OK;
    const int rc = multi_g_table(ctx);
    if (rc != GC_OK) return rc;
    return multi_setup_run(ctx, d_a, S, d_A_out, d_AaInv_out, d_status);
} catch (...) {
    return gc::on_exception();
}

int gc_co_multi_sender_encrypt_dev(gc_ctx *ctx, const void *d_a, const void *d_AaInv, const void *d_points, const void *d_wires,
                                   size_t S, size_t per, uint64_t id0, void *d_ct, void *d_status) {
    size_t n = 0;
    if (!ctx || !multi_count(S, per, &n) || (n && (!d_a || !d_AaInv || !d_points || !d_wires || !d_ct || !d_status)))
        return GC_E_ARG;
    if (n == 0) return GC_OK;
    GC_HIP(hipSetDevice(ctx->device));
    return multi_encrypt_run(ctx, d_a, d_AaInv, d_points, d_wires, S, per, id0, d_ct, d_status);
}

int gc_co_multi_receiver_choices_dev(gc_ctx *ctx, const void *d_A, const void *d_scalars, const void *d_choice, size_t S,
                                     size_t per, void *d_points_out, void *d_status) try {
    size_t n = 0;
    if (!ctx || !multi_count(S, per, &n) || (n && (!d_A || !d_scalars || !d_choice || !d_points_out || !d_status)))
        return GC_E_ARG;
    if (n == 0) return GC_OK;
    const int rc = multi_g_table(ctx);
    if (rc != GC_OK) return rc;
    return multi_choices_run(ctx, d_A, d_scalars, d_choice, S, per, d_points_out, d_status);
} catch (...) {
    return gc::on_exception();
}

int gc_co_multi_receiver_decrypt_dev(gc_ctx *ctx, const void *d_A, const void *d_scalars, const void *d_choice, const void *d_ct,
                                     size_t S, size_t per, uint64_t id0, void *d_labels_out, void *d_status) {
    size_t n = 0;
    if (!ctx || !multi_count(S, per, &n) || (n && (!d_A || !d_scalars || !d_choice || !d_ct || !d_labels_out || !d_status)))
        return GC_E_ARG;
    if (n == 0) return GC_OK;
    GC_HIP(hipSetDevice(ctx->device));
    return multi_decrypt_run(ctx, d_A, d_scalars, d_choice, d_ct, S, per, id0, d_labels_out, d_status);
}

int gc_co_multi_sender_setup(gc_ctx *ctx, const uint8_t *a, size_t S, gc_p256_point *A_out, gc_p256_point *AaInv_out,
                             size_t *bad_session) try {
    if (!ctx || (S && (!a || !A_out || !AaInv_out)) || !bytes_fit(S)) return GC_E_ARG;
    if (S == 0) return GC_OK;
    const std::vector<CoTabEntry> &g = g_table();
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    int rc = multi_g_table_locked(ctx, g);
    if (rc != GC_OK) return rc;
    uint64_t status[4] = {0, 0, 0, 0};
    Staged io[] = {{a, nullptr, S * kScalarBytes}, {nullptr, A_out, S * kPointBytes}, {nullptr, AaInv_out, S * kPointBytes},
                   {nullptr, status, sizeof status}};
    rc = stage_in(io, std::size(io), ctx->stream);
    if (rc == GC_OK) rc = multi_setup_run(ctx, io[0].d.p, S, io[1].d.p, io[2].d.p, io[3].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), ctx->stream);
    return rc == GC_OK ? multi_status(status, GC_E_ARG, nullptr, bad_session) : rc;
} catch (...) {
    return gc::on_exception();
}

int gc_co_multi_sender_encrypt(gc_ctx *ctx, const uint8_t *a, const gc_p256_point *AaInv, const gc_p256_point *points,
                               const gc_wire *wires, size_t S, size_t per, uint64_t id0, uint8_t *ct, size_t *bad_index,
                               size_t *bad_session) try {
    size_t n = 0;
    if (!ctx || !multi_count(S, per, &n) || (n && (!a || !AaInv || !points || !wires || !ct))) return GC_E_ARG;
    if (n == 0) return GC_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    uint64_t status[4] = {0, 0, 0, 0};
    Staged io[] = {{a, nullptr, S * kScalarBytes}, {AaInv, nullptr, S * kPointBytes}, {points, nullptr, n * kPointBytes},
                   {wires, nullptr, n * kWireBytes}, {nullptr, ct, n * kCtBytes}, {nullptr, status, sizeof status}};
    int rc = stage_in(io, std::size(io), ctx->stream);
    if (rc == GC_OK) rc = multi_encrypt_run(ctx, io[0].d.p, io[1].d.p, io[2].d.p, io[3].d.p, S, per, id0, io[4].d.p, io[5].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), ctx->stream);
    return rc == GC_OK ? multi_status(status, GC_E_ARG, bad_index, bad_session) : rc;
} catch (...) {
    return gc::on_exception();
}

int gc_co_multi_receiver_choices(gc_ctx *ctx, const gc_p256_point *A, const uint8_t *scalars, const uint8_t *choice, size_t S,
                                 size_t per, gc_p256_point *points_out, size_t *bad_session) try {
    size_t n = 0;
    if (!ctx || !multi_count(S, per, &n) || (n && (!A || !scalars || !choice || !points_out))) return GC_E_ARG;
    if (n == 0) return GC_OK;
    const std::vector<CoTabEntry> &g = g_table();
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    int rc = multi_g_table_locked(ctx, g);
    if (rc != GC_OK) return rc;
    uint64_t status[4] = {0, 0, 0, 0};
    Staged io[] = {{A, nullptr, S * kPointBytes}, {scalars, nullptr, n * kScalarBytes}, {choice, nullptr, n},
                   {nullptr, points_out, n * kPointBytes}, {nullptr, status, sizeof status}};
    rc = stage_in(io, std::size(io), ctx->stream);
    if (rc == GC_OK) rc = multi_choices_run(ctx, io[0].d.p, io[1].d.p, io[2].d.p, S, per, io[3].d.p, io[4].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), ctx->stream);
    return rc == GC_OK ? multi_status(status, GC_E_POINT, nullptr, bad_session) : rc;
} catch (...) {
    return gc::on_exception();
}

int gc_co_multi_receiver_decrypt(gc_ctx *ctx, const gc_p256_point *A, const uint8_t *scalars, const uint8_t *choice,
                                 const uint8_t *ct, size_t S, size_t per, uint64_t id0, gc_label *labels_out,
                                 size_t *bad_session) try {
    size_t n = 0;
    if (!ctx || !multi_count(S, per, &n) || (n && (!A || !scalars || !choice || !ct || !labels_out))) return GC_E_ARG;
    if (n == 0) return GC_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    uint64_t status[4] = {0, 0, 0, 0};
    Staged io[] = {{A, nullptr, S * kPointBytes}, {scalars, nullptr, n * kScalarBytes}, {choice, nullptr, n},
                   {ct, nullptr, n * kCtBytes}, {nullptr, labels_out, n * kLabelBytes}, {nullptr, status, sizeof status}};
    int rc = stage_in(io, std::size(io), ctx->stream);
    if (rc == GC_OK) rc = multi_decrypt_run(ctx, io[0].d.p, io[1].d.p, io[2].d.p, io[3].d.p, S, per, id0, io[4].d.p, io[5].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), ctx->stream);
    return rc == GC_OK ? multi_status(status, GC_E_POINT, nullptr, bad_session) : rc;
} catch (...) {
    return gc::on_exception();
}

}  // extern "C"

// ---- the multi receiver behind a handle: per-session window tables built on the device (gc_co_multi_base_*,
// co_multi_base_kernels.hip) ------------------------------------------------------------------------------------------------

struct gc_co_multi_base {
    gc_ctx *ctx = nullptr;
    size_t S = 0;
    CoTabEntry *d_tabs = nullptr;  // [S][960], width kCoTabWidthA; a bad session's part is never written or read
    uint32_t *d_good = nullptr;    // [S]: 1 = A_s is a point of the curve
    size_t bad = 0, lowest_bad = SIZE_MAX;
};

namespace {

constexpr size_t kTabBytes = co_tab_entries(kCoTabWidthA) * sizeof(CoTabEntry);  // 61 440 per session

void multi_base_release(gc_co_multi_base *h) {
    if (h->d_tabs) (void)hipFree(h->d_tabs);
    if (h->d_good) (void)hipFree(h->d_good);
    delete h;
}

int multi_base_alloc(void **p, size_t bytes) {
    GC_HIP(hipMalloc(p, bytes));  // (out of memory: GC_E_NOMEM)
    return GC_OK;
}

// A: S points in host memory (d_A NULL) or in device memory; the tables of the good sessions, complete on return
int multi_base_build(gc_co_multi_base *h, gc_ctx *ctx, const gc_p256_point *A, const void *d_A, size_t S) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    h->ctx = ctx;
    h->S = S;
    int rc = multi_base_alloc((void **)&h->d_tabs, S * kTabBytes);
    if (rc == GC_OK) rc = multi_base_alloc((void **)&h->d_good, S * sizeof(uint32_t));
    if (rc != GC_OK) return rc;
    const size_t chunk = std::min<size_t>(S, kCoMultiTabChunk);
    DevBuf d_pts, d_bases, d_zs;  // the build's workspace: freed before create returns
    void **ws[3] = {&d_bases.p, &d_zs.p, &d_pts.p};
    const size_t ws_bytes[3] = {S * co_tab_windows(kCoTabWidthA) * sizeof(CoTabBase),
                                chunk * co_tab_entries(kCoTabWidthA) * sizeof(CoTabZ), d_A ? 0 : S * sizeof(gc_p256_point)};
    for (int k = 0; k < 3; k++) {
        if (!ws_bytes[k]) continue;
        rc = multi_base_alloc(ws[k], ws_bytes[k]);
        if (rc != GC_OK) return rc;
    }
    hipStream_t s = ctx->stream;
    if (!d_A) {
        GC_HIP(hipMemcpyAsync(d_pts.p, A, S * sizeof(gc_p256_point), hipMemcpyHostToDevice, s));
        d_A = d_pts.p;
    }
    launch_co_multi_tab_bases((const uint4 *)d_A, S, h->d_good, (CoTabBase *)d_bases.p, s);
    GC_HIP(hipGetLastError());
    for (size_t s0 = 0; s0 < S; s0 += chunk) {  // (the launches of one stream run in order: one chunk's workspace serves all)
        launch_co_multi_tab_rows(h->d_good, (const CoTabBase *)d_bases.p, s0, std::min(chunk, S - s0), h->d_tabs,
                                 (CoTabZ *)d_zs.p, s);
        GC_HIP(hipGetLastError());
    }
    std::vector<uint32_t> good(S);
    GC_HIP(hipMemcpyAsync(good.data(), h->d_good, S * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    GC_HIP(hipStreamSynchronize(s));
    for (size_t k = S; k-- > 0;)
        if (!good[k]) {
            h->bad++;
            h->lowest_bad = k;
        }
    return GC_OK;
}

gc_co_multi_base *multi_base_create(gc_ctx *ctx, const gc_p256_point *A, const void *d_A, size_t S, int *status) try {
    int rc = GC_OK;
    gc_co_multi_base *h = nullptr;
    if (!ctx || (!A && !d_A) || S == 0 || S > SIZE_MAX / kTabBytes) {
        rc = GC_E_ARG;
    } else if (ctx->capturing) {
        rc = GC_E_ARG;  // allocates and waits for the stream: not between gc_ctx_capture_begin and _end
    } else {
        h = new gc_co_multi_base;
        try {
            rc = multi_base_build(h, ctx, A, d_A, S);
        } catch (...) {
            multi_base_release(h);
            throw;
        }
        if (rc != GC_OK) {
            (void)hipStreamSynchronize(ctx->stream);  // a build kernel may be queued on what is freed next
            multi_base_release(h);
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

// the arguments of a decrypt; *n = S * per
bool multi_base_args(const gc_co_multi_base *h, size_t per, bool pointers, size_t *n) {
    return h && multi_count(h->S, per, n) && (*n == 0 || pointers);
}

// the decrypt on device pointers, the device set: what the _dev form does behind its checks
int multi_base_decrypt_run(gc_co_multi_base *h, const void *d_scalars, const void *d_choice, const void *d_ct, size_t per,
                           uint64_t id0, void *d_labels_out, void *d_status) {
    GC_HIP(reset_status4(d_status, h->ctx->stream));
    launch_co_multi_decrypt_tab(h->d_tabs, h->d_good, (const uint4 *)d_scalars, (const uint8_t *)d_choice, (const uint4 *)d_ct,
                                h->S, per, id0, (uint4 *)d_labels_out, (unsigned long long *)d_status, h->ctx->stream);
    return launched();
}

}  // namespace

extern "C" {

gc_co_multi_base *gc_co_multi_base_create(gc_ctx *ctx, const gc_p256_point *A, size_t S, int *status) {
    return multi_base_create(ctx, A, nullptr, S, status);
}

gc_co_multi_base *gc_co_multi_base_create_dev(gc_ctx *ctx, const void *d_A, size_t S, int *status) {
    return multi_base_create(ctx, nullptr, d_A, S, status);
}

void gc_co_multi_base_free(gc_co_multi_base *h) {
    if (!h) return;
    if (h->ctx) {
        (void)hipSetDevice(h->ctx->device);
        (void)hipStreamSynchronize(h->ctx->stream);  // a _dev call may still read the tables
    }
    multi_base_release(h);
}

int gc_co_multi_base_info(const gc_co_multi_base *h, size_t *S, size_t *bad_sessions, size_t *lowest_bad) {
    if (!h) return GC_E_ARG;
    if (S) *S = h->S;
    if (bad_sessions) *bad_sessions = h->bad;
    if (lowest_bad) *lowest_bad = h->lowest_bad;  // all ones: none
    return GC_OK;
}

int gc_co_multi_base_decrypt_dev(gc_co_multi_base *h, const void *d_scalars, const void *d_choice, const void *d_ct, size_t per,
                                 uint64_t id0, void *d_labels_out, void *d_status) {
    size_t n = 0;
    if (!multi_base_args(h, per, d_scalars && d_choice && d_ct && d_labels_out && d_status, &n)) return GC_E_ARG;
    if (n == 0) return GC_OK;
    GC_HIP(hipSetDevice(h->ctx->device));
    return multi_base_decrypt_run(h, d_scalars, d_choice, d_ct, per, id0, d_labels_out, d_status);
}

int gc_co_multi_base_decrypt(gc_co_multi_base *h, const uint8_t *scalars, const uint8_t *choice, const uint8_t *ct, size_t per,
                             uint64_t id0, gc_label *labels_out, size_t *bad_session) try {
    size_t n = 0;
    if (!multi_base_args(h, per, scalars && choice && ct && labels_out, &n)) return GC_E_ARG;
    if (n == 0) return GC_OK;
    gc_ctx *ctx = h->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GC_HIP(hipSetDevice(ctx->device));
    uint64_t status[4] = {0, 0, 0, 0};
    Staged io[] = {{scalars, nullptr, n * kScalarBytes}, {choice, nullptr, n}, {ct, nullptr, n * kCtBytes},
                   {nullptr, labels_out, n * kLabelBytes}, {nullptr, status, sizeof status}};
    int rc = stage_in(io, std::size(io), ctx->stream);
    if (rc == GC_OK) rc = multi_base_decrypt_run(h, io[0].d.p, io[1].d.p, io[2].d.p, per, id0, io[3].d.p, io[4].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), ctx->stream);
    return rc == GC_OK ? multi_status(status, GC_E_POINT, nullptr, bad_session) : rc;
} catch (...) {
    return gc::on_exception();
}

}  // extern "C"
