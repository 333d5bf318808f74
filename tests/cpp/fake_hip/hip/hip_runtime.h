// Stand-in for <hip/hip_runtime.h>, for the stand-alone programs of tests/cpp that check a header of mpc_amd/csrc on the CPU
// (host_staging_check.cpp, host_transfer_check.cpp): the runtime calls of those headers on host memory.  Device memory, streams
// and events are malloc'ed (so AddressSanitizer sees bounds, leaks and double frees), a copy is a memcpy at once, every call is
// appended to a log with the stream it names, and the k-th fallible call (allocation, creation, copy, record, wait; hipFree and
// the destroy calls never fail) can be told to fail.
#pragma once

#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2, hipErrorUnknown = 999 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
typedef struct fake_hip_stream *hipStream_t;
typedef struct fake_hip_event *hipEvent_t;
struct fake_hip_stream {
    int unused;
};
struct fake_hip_event {
    int unused;
};
constexpr unsigned hipStreamNonBlocking = 1, hipEventDisableTiming = 2;

namespace fake_hip {

enum Op { kMalloc, kFree, kCopyIn, kCopyOut, kWait, kOperation, kStreamCreate, kStreamDestroy, kEventCreate, kEventDestroy, kRecord, kWaitEvent };
struct Event {
    Op op;
    const void *dev;  // the device pointer of an allocation, a free or a copy; the staging buffer of a logged kernel
    size_t bytes;
    bool ok;
    hipStream_t stream = nullptr;  // of a copy, a wait, a record, a wait for an event, a logged kernel; the one created / destroyed
    hipEvent_t event = nullptr;    // of a record or a wait for it; the one created / destroyed
};
struct State {
    std::vector<Event> log;
    long calls = 0;     // fallible calls so far
    long fail_at = -1;  // the index of the fallible call that fails, once
    hipError_t fail_code = hipErrorUnknown;
};
inline State &state() {
    static State s;
    return s;
}
inline void reset(long fail_at = -1, hipError_t code = hipErrorUnknown) {
    state() = State();
    state().fail_at = fail_at;
    state().fail_code = code;
}
// logs the call; hipSuccess, or the code this call was told to fail with
inline hipError_t call(Op op, const void *dev, size_t bytes, hipStream_t stream = nullptr, hipEvent_t event = nullptr) {
    State &s = state();
    const bool ok = s.calls++ != s.fail_at;
    s.log.push_back(Event{op, dev, bytes, ok, stream, event});
    return ok ? hipSuccess : s.fail_code;
}
// the operation between stage_in and stage_out puts itself into the log with this
inline void note_operation() { state().log.push_back(Event{kOperation, nullptr, 0, true}); }

}  // namespace fake_hip

inline hipError_t hipMalloc(void **p, size_t bytes) {
    const hipError_t e = fake_hip::call(fake_hip::kMalloc, nullptr, bytes);
    if (e != hipSuccess) return e;
    *p = std::malloc(bytes);
    fake_hip::state().log.back().dev = *p;
    return hipSuccess;
}

inline hipError_t hipFree(void *p) {
    fake_hip::state().log.push_back(fake_hip::Event{fake_hip::kFree, p, 0, true});
    std::free(p);
    return hipSuccess;
}

inline hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    const bool in = kind == hipMemcpyHostToDevice;
    const hipError_t e = fake_hip::call(in ? fake_hip::kCopyIn : fake_hip::kCopyOut, in ? dst : src, bytes, s);
    if (e == hipSuccess) std::memcpy(dst, src, bytes);
    return e;
}

// `height` rows of `width` bytes, the rows `spitch` / `dpitch` bytes apart
inline hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height,
                                   hipMemcpyKind kind, hipStream_t s) {
    const bool in = kind == hipMemcpyHostToDevice;
    const hipError_t e = fake_hip::call(in ? fake_hip::kCopyIn : fake_hip::kCopyOut, in ? dst : src, width * height, s);
    for (size_t r = 0; e == hipSuccess && r < height; r++)
        std::memcpy((char *)dst + r * dpitch, (const char *)src + r * spitch, width);
    return e;
}

inline hipError_t hipStreamSynchronize(hipStream_t s) { return fake_hip::call(fake_hip::kWait, nullptr, 0, s); }

inline hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) {
    const hipError_t e = fake_hip::call(fake_hip::kStreamCreate, nullptr, 0);
    if (e != hipSuccess) return e;
    *s = (hipStream_t)std::malloc(sizeof(fake_hip_stream));
    fake_hip::state().log.back().stream = *s;
    return hipSuccess;
}

inline hipError_t hipStreamDestroy(hipStream_t s) {
    fake_hip::state().log.push_back(fake_hip::Event{fake_hip::kStreamDestroy, nullptr, 0, true, s});
    std::free(s);
    return hipSuccess;
}

inline hipError_t hipEventCreateWithFlags(hipEvent_t *ev, unsigned) {
    const hipError_t e = fake_hip::call(fake_hip::kEventCreate, nullptr, 0);
    if (e != hipSuccess) return e;
    *ev = (hipEvent_t)std::malloc(sizeof(fake_hip_event));
    fake_hip::state().log.back().event = *ev;
    return hipSuccess;
}

inline hipError_t hipEventDestroy(hipEvent_t ev) {
    fake_hip::state().log.push_back(fake_hip::Event{fake_hip::kEventDestroy, nullptr, 0, true, nullptr, ev});
    std::free(ev);
    return hipSuccess;
}

// the event takes the place of everything queued on `s` so far
inline hipError_t hipEventRecord(hipEvent_t ev, hipStream_t s) { return fake_hip::call(fake_hip::kRecord, nullptr, 0, s, ev); }

// what is queued on `s` from here on runs behind the last record of the event
inline hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t ev, unsigned) { return fake_hip::call(fake_hip::kWaitEvent, nullptr, 0, s, ev); }
