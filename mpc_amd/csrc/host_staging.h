// host_staging.h — what the host form of an OT-family primitive is made of: the _dev operation run between staged copies in
// and out.  Depends on the HIP runtime, the status codes of gcengine.h and gc::set_error only — no gc_ctx,
// no kernels — so that a CPU test compiles it on its own against a stand-in runtime (tests/test_host_staging.py).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/gcengine.h"

namespace gc {
void set_error(const char *what, hipError_t e);

// a temporary device buffer, freed on scope exit
struct DevBuf {
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
};
}  // namespace gc

#define GC_HIP(expr)                                                   \
    do {                                                               \
        hipError_t e__ = (expr);                                       \
        if (e__ != hipSuccess) {                                       \
            gc::set_error(#expr, e__);                                 \
            return e__ == hipErrorOutOfMemory ? GC_E_NOMEM : GC_E_HIP; \
        }                                                              \
    } while (0)

namespace gc {

// One Staged per array of the operation, in the order of its arguments; the operation gets d.p.  The rule on failure: every
// allocation precedes the first copy, and once anything may be queued on the stream no device copy is freed, and the host
// form does not return, before the stream has been waited for — on success by stage_out's one wait, on any other way out by
// ~Staged, which runs before d is freed.
struct Staged {
    const void *in;        // copied to the device before the operation, or NULL
    void *out;             // copied back behind it, or NULL (both: an array updated in place)
    size_t bytes;          // of either copy; 0: no copy, d.p is still a valid pointer
    size_t dev_bytes = 0;  // the device copy where it is larger than `bytes`; 0: as `bytes`
    DevBuf d{};
    hipStream_t busy = nullptr;  // the stream that may hold work on d, from stage_in until it has been waited for
    ~Staged() {
        if (busy) (void)hipStreamSynchronize(busy);
    }
};

inline int stage_in(Staged *io, size_t k, hipStream_t s) {
    for (size_t j = 0; j < k; j++) GC_HIP(io[j].d.alloc(io[j].dev_bytes ? io[j].dev_bytes : io[j].bytes));
    for (size_t j = 0; j < k; j++) io[j].busy = s;  // the caller queues the operation even where no input is copied
    for (size_t j = 0; j < k; j++)
        if (io[j].in && io[j].bytes) GC_HIP(hipMemcpyAsync(io[j].d.p, io[j].in, io[j].bytes, hipMemcpyHostToDevice, s));
    return GC_OK;
}

// the outputs (a status block is one of them), then the one wait of the call
inline int stage_out(Staged *io, size_t k, hipStream_t s) {
    for (size_t j = 0; j < k; j++)
        if (io[j].out && io[j].bytes) GC_HIP(hipMemcpyAsync(io[j].out, io[j].d.p, io[j].bytes, hipMemcpyDeviceToHost, s));
    GC_HIP(hipStreamSynchronize(s));
    for (size_t j = 0; j < k; j++) io[j].busy = nullptr;
    return GC_OK;
}

// one byte per choice, S rows of `per` -> S rows of row_bytes >= ceil(per / 8) bytes, packed LSB first (iknp.go:472-477) and
// zero-padded
inline std::vector<uint8_t> pack_rows(const uint8_t *src, size_t S, size_t per, size_t row_bytes) {
    std::vector<uint8_t> out(S * row_bytes, 0);
    for (size_t s = 0; s < S; s++)
        for (size_t j = 0; j < per; j++)
            if (src[s * per + j]) out[s * row_bytes + j / 8] |= (uint8_t)(1u << (j % 8));
    return out;
}

}  // namespace gc
