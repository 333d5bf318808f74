// host_transfer.h — a [row][instance] device array to or from a caller's [instance][n] host array, in chunks of instances through
// staging buffers that a transpose kernel fills or empties.  Depends on the HIP runtime, the status codes of
// gcengine.h and gc::set_error only — no gc_ctx, no gc_batch, no kernels: the kernel of a chunk comes in as a callable — so that
// a CPU test compiles it on its own against a stand-in runtime (tests/test_host_transfer.py).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "host_staging.h"  // GC_HIP, gc::set_error

namespace gc {

// what one direction of a chunked transfer may hold in staging memory: per buffer of the pinned form (long enough for the full
// PCIe rate, short enough that the first chunk's transpose hides nothing big), and for the one buffer of the pageable form
constexpr size_t kPipeChunkBytes = (size_t)32 << 20, kPageableChunkBytes = (size_t)64 << 20;

// The chunk rule: as many instances as the budget holds, at least 32 and no more than the batch, in whole groups of 32 (the
// transpose kernels work on 32 instances at a time); a staging buffer holds one chunk, or the whole batch where that is less.
struct Chunks {
    uint32_t chunk;      // instances per chunk
    size_t stage_bytes;  // of one staging buffer
};
inline Chunks chunk_rule(uint32_t batch, size_t per_inst, size_t budget) {
    uint32_t chunk = (uint32_t)std::max<size_t>(32, std::min<size_t>(batch, budget / per_inst));
    chunk = (chunk + 31u) & ~31u;
    return Chunks{chunk, (size_t)std::min<uint32_t>(chunk, (batch + 31u) & ~31u) * per_inst};
}

// What the transfers of one work stream share, created at first use: a stream for the copies of the pinned form, whose DMA of
// chunk k then runs beside the kernel of chunk k + 1 on the other buffer, the events between the two streams, and two staging
// buffers (the pageable form uses stage[0]).
struct TransferPipe {
    hipStream_t work = nullptr;  // the kernels' stream; not owned
    hipStream_t copy = nullptr;
    hipEvent_t ev_k[2] = {nullptr, nullptr};  // kernel on stage[b] done
    hipEvent_t ev_c[2] = {nullptr, nullptr};  // copy from / to stage[b] done
    void *stage[2] = {nullptr, nullptr};
    size_t stage_cap = 0;

    // the copy stream, the events and staging buffers of at least `bytes` each; both streams are idle before a buffer is freed
    int ensure(size_t bytes) {
        if (!copy) GC_HIP(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking));
        for (int b = 0; b < 2; b++) {
            if (!ev_k[b]) GC_HIP(hipEventCreateWithFlags(&ev_k[b], hipEventDisableTiming));
            if (!ev_c[b]) GC_HIP(hipEventCreateWithFlags(&ev_c[b], hipEventDisableTiming));
        }
        if (bytes <= stage_cap) return GC_OK;
        GC_HIP(hipStreamSynchronize(work));
        GC_HIP(hipStreamSynchronize(copy));
        for (int b = 0; b < 2; b++) {
            if (stage[b]) (void)hipFree(stage[b]);
            stage[b] = nullptr;
        }
        stage_cap = 0;
        for (int b = 0; b < 2; b++) GC_HIP(hipMalloc(&stage[b], bytes));
        stage_cap = bytes;
        return GC_OK;
    }
    // when the owner goes, with nothing left on either stream
    void release() {
        for (int b = 0; b < 2; b++) {
            if (stage[b]) (void)hipFree(stage[b]);
            if (ev_k[b]) (void)hipEventDestroy(ev_k[b]);
            if (ev_c[b]) (void)hipEventDestroy(ev_c[b]);
            stage[b] = nullptr;
            ev_k[b] = ev_c[b] = nullptr;
        }
        if (copy) (void)hipStreamDestroy(copy);
        copy = nullptr;
        stage_cap = 0;
    }
};

// The rule on failure: once a transfer has queued anything it does not return before both streams have been waited for — the
// DMA may be reading or writing the caller's memory, a kernel the staging buffer that the next call reuses.  The status is the
// first failure's, whatever those waits say, and no staging buffer is freed.  (GC_XFER: a step of the loops below; the loop
// ends at the first that fails.)
#define GC_XFER(expr)                \
    do {                             \
        hipError_t e__ = (expr);     \
        if (e__ != hipSuccess) {     \
            *what = #expr;           \
            return e__;              \
        }                            \
    } while (0)

inline int transfer_end(TransferPipe &p, hipError_t e, const char *what) {
    if (e == hipSuccess) return GC_OK;
    (void)hipStreamSynchronize(p.work);
    (void)hipStreamSynchronize(p.copy);
    set_error(what, e);
    return e == hipErrorOutOfMemory ? GC_E_NOMEM : GC_E_HIP;
}

// gather(stage, i0, cnt) -> hipError_t queues on p.work the kernel that puts instances [i0, i0 + cnt) into `stage`, dense.
// pinned: the copy to the host on the copy stream, behind the kernel by ev_k and ahead of the buffer's next kernel by ev_c; one
// wait, of the copy stream, at the end.  Otherwise kernel and copy on p.work, one buffer, a wait per chunk.
template <class Gather>
hipError_t download_chunks(TransferPipe &p, bool pinned, uint32_t batch, uint32_t chunk, size_t per_inst, uint8_t *host,
                           Gather &gather, const char **what) {
    const hipStream_t cs = pinned ? p.copy : p.work;
    uint32_t k = 0;
    for (uint32_t i0 = 0; i0 < batch; i0 += chunk, k++) {
        const int sb = pinned ? (int)(k & 1) : 0;
        const uint32_t cnt = std::min(chunk, batch - i0);
        if (pinned && k >= 2) GC_XFER(hipStreamWaitEvent(p.work, p.ev_c[sb], 0));  // the buffer's previous DMA is done
        GC_XFER(gather(p.stage[sb], i0, cnt));
        if (pinned) {
            GC_XFER(hipEventRecord(p.ev_k[sb], p.work));
            GC_XFER(hipStreamWaitEvent(cs, p.ev_k[sb], 0));
        }
        GC_XFER(hipMemcpyAsync(host + (size_t)i0 * per_inst, p.stage[sb], (size_t)cnt * per_inst, hipMemcpyDeviceToHost, cs));
        GC_XFER(pinned ? hipEventRecord(p.ev_c[sb], cs) : hipStreamSynchronize(cs));
    }
    if (pinned) GC_XFER(hipStreamSynchronize(cs));
    return hipSuccess;
}

// device -> host [batch][per_inst bytes]
template <class Gather>
int download(TransferPipe &p, bool pinned, uint32_t batch, size_t per_inst, size_t budget, void *host, Gather gather) {
    const Chunks c = chunk_rule(batch, per_inst, budget);
    const int rc = p.ensure(c.stage_bytes);
    if (rc != GC_OK) return rc;
    const char *what = "";
    return transfer_end(p, download_chunks(p, pinned, batch, c.chunk, per_inst, (uint8_t *)host, gather, &what), what);
}

// scatter(stage, i0, cnt) -> hipError_t queues on p.work the kernel that takes instances [i0, i0 + cnt) out of `stage`.
// pinned: the copy from the host on the copy stream, behind the buffer's previous kernel by ev_k and ahead of its own by ev_c;
// one wait, of p.work, at the end.  Otherwise copy and kernel on p.work, one buffer, a wait per chunk.
template <class Scatter>
hipError_t upload_chunks(TransferPipe &p, bool pinned, uint32_t batch, uint32_t chunk, size_t per_inst, const uint8_t *host,
                         size_t pitch, Scatter &scatter, const char **what) {
    const hipStream_t cs = pinned ? p.copy : p.work;
    if (pinned) {  // what is already queued on p.work may still read the staging buffers (an earlier pipelined call)
        GC_XFER(hipEventRecord(p.ev_k[0], p.work));
        GC_XFER(hipStreamWaitEvent(cs, p.ev_k[0], 0));
    }
    uint32_t k = 0;
    for (uint32_t i0 = 0; i0 < batch; i0 += chunk, k++) {
        const int sb = pinned ? (int)(k & 1) : 0;
        const uint32_t cnt = std::min(chunk, batch - i0);
        const uint8_t *src = host + (size_t)i0 * pitch;
        if (pinned && k >= 2) GC_XFER(hipStreamWaitEvent(cs, p.ev_k[sb], 0));  // the buffer's previous scatter is done
        if (pitch == per_inst)
            GC_XFER(hipMemcpyAsync(p.stage[sb], src, (size_t)cnt * per_inst, hipMemcpyHostToDevice, cs));
        else
            GC_XFER(hipMemcpy2DAsync(p.stage[sb], per_inst, src, pitch, per_inst, cnt, hipMemcpyHostToDevice, cs));
        if (pinned) {
            GC_XFER(hipEventRecord(p.ev_c[sb], cs));
            GC_XFER(hipStreamWaitEvent(p.work, p.ev_c[sb], 0));
        }
        GC_XFER(scatter((const void *)p.stage[sb], i0, cnt));
        GC_XFER(pinned ? hipEventRecord(p.ev_k[sb], p.work) : hipStreamSynchronize(cs));
    }
    if (pinned) GC_XFER(hipStreamSynchronize(p.work));
    return hipSuccess;
}

// host -> device: instance i is the per_inst bytes at host + i * pitch (pitch > per_inst: a column range of a wider array)
template <class Scatter>
int upload(TransferPipe &p, bool pinned, uint32_t batch, size_t per_inst, size_t budget, const void *host, size_t pitch,
           Scatter scatter) {
    const Chunks c = chunk_rule(batch, per_inst, budget);
    const int rc = p.ensure(c.stage_bytes);
    if (rc != GC_OK) return rc;
    const char *what = "";
    return transfer_end(p, upload_chunks(p, pinned, batch, c.chunk, per_inst, (const uint8_t *)host, pitch, scatter, &what), what);
}

#undef GC_XFER

}  // namespace gc
