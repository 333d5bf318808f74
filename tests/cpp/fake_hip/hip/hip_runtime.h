// Stand-in for <hip/hip_runtime.h>, for tests/cpp/host_staging_check.cpp only: the four calls of mpc_amd/csrc/host_staging.h on
// host memory.  Device memory is malloc'ed (so AddressSanitizer sees its bounds, leaks and double frees), a copy is a memcpy at
// once, every call is appended to a log, and the k-th fallible call (allocation, copy or wait; hipFree never fails) can be
// told to fail.
#pragma once

#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorUnknown = 999 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
typedef struct fake_hip_stream *hipStream_t;

namespace fake_hip {

enum Op { kMalloc, kFree, kCopyIn, kCopyOut, kWait, kOperation };
struct Event {
    Op op;
    const void *dev;  // the device pointer of an allocation, a free or a copy
    size_t bytes;
    bool ok;
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
inline hipError_t call(Op op, const void *dev, size_t bytes) {
    State &s = state();
    const bool ok = s.calls++ != s.fail_at;
    s.log.push_back(Event{op, dev, bytes, ok});
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

inline hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
    const bool in = kind == hipMemcpyHostToDevice;
    const hipError_t e = fake_hip::call(in ? fake_hip::kCopyIn : fake_hip::kCopyOut, in ? dst : src, bytes);
    if (e == hipSuccess) std::memcpy(dst, src, bytes);
    return e;
}

inline hipError_t hipStreamSynchronize(hipStream_t) { return fake_hip::call(fake_hip::kWait, nullptr, 0); }
