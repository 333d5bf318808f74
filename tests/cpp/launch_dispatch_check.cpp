// Stand-alone check of the dispatch helpers of mpc_amd/csrc/launch_dispatch.h (tests/test_launch_dispatch.py), built with the
// host compiler against the stand-in <hip/hip_runtime.h> of tests/cpp/fake_hip: no HIP, so the launchers are not in it.
#include <cstdio>
#include <type_traits>

#include "launch_dispatch.h"

namespace {

int failures = 0;
void expect(bool ok, const char *what) {
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s\n", what);
        failures++;
    }
}

// what a kernel template would be: the round count has to be a constant expression to name one
template <int NR>
struct Build {
    static constexpr int rounds = NR;
};

void rounds_are_compile_time_constants() {
    for (int rounds : {10, 12, 14}) {
        int calls = 0, seen = 0;
        const hipError_t e = gc::with_rounds(rounds, [&](auto nr) {
            constexpr int NR = decltype(nr)::value;
            static_assert(NR == 10 || NR == 12 || NR == 14, "only the three AES round counts are instantiated");
            static_assert(std::is_same<decltype(nr), std::integral_constant<int, NR>>::value, "an integral_constant<int, NR>");
            calls++;
            seen = Build<NR>::rounds;
            return hipSuccess;
        });
        expect(e == hipSuccess && calls == 1 && seen == rounds, "with_rounds hands 10 / 12 / 14 on, once");
    }
    // ... and returns what the callback returns
    expect(gc::with_rounds(12, [](auto) { return hipErrorOutOfMemory; }) == hipErrorOutOfMemory, "with_rounds returns f's result");
}

void other_rounds_are_refused() {
    for (int rounds : {0, 11, 13, 15, -1}) {
        int calls = 0;
        const hipError_t e = gc::with_rounds(rounds, [&](auto) {
            calls++;
            return hipSuccess;
        });
        expect(e == hipErrorInvalidValue && calls == 0, "any other round count: hipErrorInvalidValue, no call");
    }
}

void flags_are_forwarded() {
    for (bool b : {false, true}) {
        int calls = 0;
        const int got = gc::with_flag(b, [&](auto flag) {
            constexpr bool FLAG = decltype(flag)::value;
            static_assert(std::is_same<decltype(flag), std::integral_constant<bool, FLAG>>::value, "true_type or false_type");
            calls++;
            return FLAG ? 7 : 3;
        });
        expect(calls == 1 && got == (b ? 7 : 3), "with_flag forwards the value");
    }
}

void nested_use_returns_the_inner_result() {
    for (int rounds : {10, 12, 14})
        for (bool a : {false, true})
            for (bool b : {false, true}) {
                const hipError_t e = gc::with_rounds(rounds, [&](auto nr) {
                    return gc::with_flag(a, [&](auto fa) {
                        return gc::with_flag(b, [&](auto fb) {
                            constexpr int NR = decltype(nr)::value;
                            constexpr bool A = decltype(fa)::value, B = decltype(fb)::value;
                            // the inner result names the build it was given
                            return NR == rounds && A == a && B == b ? hipErrorOutOfMemory : hipErrorUnknown;
                        });
                    });
                });
                expect(e == hipErrorOutOfMemory, "nested: the innermost callback's result, for the build the values name");
            }
    int calls = 0;
    const hipError_t e = gc::with_rounds(13, [&](auto) {
        return gc::with_flag(true, [&](auto) {
            calls++;
            return hipSuccess;
        });
    });
    expect(e == hipErrorInvalidValue && calls == 0, "nested: a refused round count reaches no callback");
}

}  // namespace

int main() {
    rounds_are_compile_time_constants();
    other_rounds_are_refused();
    flags_are_forwarded();
    nested_use_returns_the_inner_result();
    if (failures) return 1;
    std::puts("launch_dispatch: ok");
    return 0;
}
