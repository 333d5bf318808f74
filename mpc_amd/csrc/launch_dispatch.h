// launch_dispatch.h — from run-time values to kernel builds, and the two ways a kernel is launched.
//
// Every garbling kernel is a template over the AES round count (10 / 12 / 14 for keys of 16 / 24 / 32 bytes) and some over
// a flag or two.  A launcher names its build once, inside generic lambdas that receive the run-time values as types:
//
//     return with_rounds(a.rounds, [&](auto nr) {
//         return with_flag(a.prof != nullptr, [&](auto prof) {
//             return launch_kernel(k_garble_fused<nr(), prof()>, grid, block, s, ...);
//         });
//     });
//
// A build is instantiated for every combination the nesting spans, so a launcher that selects from fewer builds branches on
// the run-time value outside instead of nesting with_flag.  The dispatch helpers are plain C++17 (a host compiler can
// include this header without HIP); the launchers need hipcc.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>

namespace gc {

// f(std::integral_constant<int, rounds>{}) for rounds 10, 12 or 14; any other value: hipErrorInvalidValue, f is not called.
// (The ABI refuses every other key length with GC_E_KEYSIZE long before a launch.)
template <typename F>
hipError_t with_rounds(int rounds, F &&f) {
    if (rounds == 10) return f(std::integral_constant<int, 10>{});
    if (rounds == 12) return f(std::integral_constant<int, 12>{});
    if (rounds == 14) return f(std::integral_constant<int, 14>{});
    return hipErrorInvalidValue;
}

// f(std::true_type{}) or f(std::false_type{})
template <typename F>
auto with_flag(bool b, F &&f) -> decltype(f(std::true_type{})) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}

#if defined(__HIPCC__)
// a kernel without dynamic LDS: launch, return the launch's error
template <typename K, typename... A>
hipError_t launch_kernel(K kern, dim3 grid, dim3 block, hipStream_t s, A... args) {
    hipLaunchKernelGGL(kern, grid, block, 0, s, args...);
    return hipGetLastError();
}

// a kernel with `lds` bytes of dynamic LDS: set the size, launch, return the first error
template <typename K, typename... A>
hipError_t launch_with_lds(K kern, dim3 grid, dim3 block, size_t lds, hipStream_t s, A... args) {
    hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, block, lds, s, args...);
    return hipGetLastError();
}
#endif

}  // namespace gc
