// host_staging_check.cpp — mpc_amd/csrc/host_staging.h on the CPU, against the stand-in runtime of tests/cpp/fake_hip
// (tests/test_host_staging.py compiles and runs this under AddressSanitizer and UBSan).  A host form of five arrays — an
// input, an output, one updated in place, one of zero bytes and one whose device copy is larger than what is copied — is run
// clean and with a failure injected at every call; argv[1] names the check, the exit status is 0 when it holds.
#include <cstdio>
#include <cstring>
#include <iterator>
#include <map>
#include <string>

#include "host_staging.h"

using namespace gc;
using namespace fake_hip;

static int g_errors = 0;  // calls of gc::set_error
namespace gc {
void set_error(const char *, hipError_t) { g_errors++; }
}  // namespace gc

#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

namespace {

constexpr size_t kA = 24, kB = 40, kC = 9, kE = 10, kEDev = 64;
const hipStream_t kStream = (hipStream_t)0x1000;

struct Arrays {
    uint8_t a[kA], b[kB], c[kC], e[kE];
    bool zero_ptr = false;  // the operation saw a device pointer for the zero-byte array
    Arrays() {
        for (size_t i = 0; i < kA; i++) a[i] = (uint8_t)(3 * i + 1);
        std::memset(b, 0xee, kB);
        for (size_t i = 0; i < kC; i++) c[i] = (uint8_t)(100 + i);
        for (size_t i = 0; i < kE; i++) e[i] = (uint8_t)(7 * i);
    }
};

// on device pointers: b[i] = a[i % kA] ^ e[i % kE], c[i] += 1, and every byte of e's device copy is written
int operation(const uint8_t *d_a, uint8_t *d_b, uint8_t *d_c, const void *d_zero, uint8_t *d_e, Arrays *h) {
    note_operation();
    h->zero_ptr = d_zero != nullptr;
    for (size_t i = 0; i < kB; i++) d_b[i] = d_a[i % kA] ^ d_e[i % kE];
    for (size_t i = 0; i < kC; i++) d_c[i]++;
    std::memset(d_e, 0, kEDev);
    return GC_OK;
}

int host_form(Arrays *h) {
    Staged io[] = {{h->a, nullptr, kA}, {nullptr, h->b, kB}, {h->c, h->c, kC}, {nullptr, nullptr, 0}, {h->e, nullptr, kE, kEDev}};
    int rc = stage_in(io, std::size(io), kStream);
    if (rc == GC_OK)
        rc = operation((const uint8_t *)io[0].d.p, (uint8_t *)io[1].d.p, (uint8_t *)io[2].d.p, io[3].d.p, (uint8_t *)io[4].d.p, h);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), kStream);
    return rc;
}

// what holds for the log of every run, clean or not: nothing is freed while a copy or the operation may be queued, and every
// allocation is freed exactly once
int check_log_rules() {
    bool queued = false;
    std::map<const void *, int> live;
    for (const Event &ev : state().log) switch (ev.op) {
            case kMalloc:
                if (ev.ok) CHECK(live[ev.dev]++ == 0);
                break;
            case kCopyIn:
            case kCopyOut:
            case kOperation:
                queued = true;  // (a copy that failed may have been queued in part)
                break;
            case kWait:
                if (ev.ok) queued = false;
                break;
            case kFree:
                CHECK(!queued);
                CHECK(live[ev.dev]-- == 1);
                break;
            default:  // (streams and events: host_staging.h creates none)
                CHECK(false);
        }
    for (const auto &kv : live) CHECK(kv.second == 0);
    return 0;
}

// 1. the order of a clean run, and 2. its data
int check_clean_run() {
    reset();
    Arrays h;
    CHECK(host_form(&h) == GC_OK && g_errors == 0);
    const std::vector<Event> &log = state().log;
    const Op want[] = {kMalloc, kMalloc, kMalloc,  kMalloc,  kMalloc, kCopyIn, kCopyIn, kCopyIn, kOperation,
                       kCopyOut, kCopyOut, kWait, kFree, kFree, kFree, kFree, kFree};
    CHECK(log.size() == std::size(want));
    for (size_t i = 0; i < log.size(); i++) CHECK(log[i].op == want[i] && log[i].ok);
    // allocations in array order, at the device size; the zero-byte entry is a real allocation
    const size_t dev_bytes[] = {kA, kB, kC, 16, kEDev};
    for (size_t j = 0; j < 5; j++) CHECK(log[j].bytes == dev_bytes[j] && log[j].dev != nullptr);
    // inputs in array order (a, c, e), outputs in array order (b, c), each at `bytes`; none for the zero-byte entry
    CHECK(log[5].dev == log[0].dev && log[5].bytes == kA);
    CHECK(log[6].dev == log[2].dev && log[6].bytes == kC);
    CHECK(log[7].dev == log[4].dev && log[7].bytes == kE);
    CHECK(log[9].dev == log[1].dev && log[9].bytes == kB);
    CHECK(log[10].dev == log[2].dev && log[10].bytes == kC);
    CHECK(check_log_rules() == 0);
    // the data
    const Arrays fresh;
    CHECK(h.zero_ptr);
    for (size_t i = 0; i < kB; i++) CHECK(h.b[i] == (uint8_t)(fresh.a[i % kA] ^ fresh.e[i % kE]));
    for (size_t i = 0; i < kC; i++) CHECK(h.c[i] == (uint8_t)(fresh.c[i] + 1));
    CHECK(!std::memcmp(h.a, fresh.a, kA) && !std::memcmp(h.e, fresh.e, kE));  // inputs are not copied back
    return 0;
}

// 3. a failure at every fallible call, from the first allocation to the wait
int check_failures() {
    reset();
    Arrays clean;
    CHECK(host_form(&clean) == GC_OK);
    const long calls = state().calls;
    CHECK(calls == 11);  // 5 allocations, 3 copies in, 2 copies out, the wait
    for (long at = 0; at < calls; at++)
        for (hipError_t code : {hipErrorOutOfMemory, hipErrorUnknown}) {
            reset(at, code);
            g_errors = 0;
            Arrays h;
            const int rc = host_form(&h);
            CHECK(rc == (code == hipErrorOutOfMemory ? GC_E_NOMEM : GC_E_HIP));
            CHECK(g_errors == 1);
            CHECK(check_log_rules() == 0);
            size_t copies = 0, failed = 0;
            for (const Event &ev : state().log) {
                copies += ev.op == kCopyIn || ev.op == kCopyOut;
                failed += !ev.ok;
            }
            CHECK(failed == 1);
            if (at < 5) CHECK(copies == 0 && state().log.size() == (size_t)(2 * at + 1));  // at allocations, 1 failure, at frees
        }
    return 0;
}

// 4. pack_rows against the definition, bit by bit
int check_pack_rows() {
    for (size_t per : {0, 1, 7, 8, 9, 511, 512, 513})
        for (size_t S : {1, 3})
            for (size_t extra : {0, 1, 16}) {
                const size_t row = (per + 7) / 8 + extra;
                std::vector<uint8_t> src(S * per);
                uint32_t x = (uint32_t)(per * 31 + S);
                for (uint8_t &v : src) {
                    x = x * 1664525u + 1013904223u;
                    v = (x >> 24) % 3 == 0 ? 0 : (uint8_t)(x >> 16);  // any non-zero byte is a set choice
                }
                const std::vector<uint8_t> got = pack_rows(src.data(), S, per, row);
                CHECK(got.size() == S * row);
                for (size_t s = 0; s < S; s++)
                    for (size_t bit = 0; bit < row * 8; bit++) {
                        const bool want = bit < per && src[s * per + bit] != 0;
                        CHECK((((got[s * row + bit / 8] >> (bit % 8)) & 1) != 0) == want);
                    }
            }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    const std::string which = argc == 2 ? argv[1] : "";
    if (which == "clean") return check_clean_run();
    if (which == "failures") return check_failures();
    if (which == "pack_rows") return check_pack_rows();
    return 2;
}
