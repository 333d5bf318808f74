// host_transfer_check.cpp — mpc_amd/csrc/host_transfer.h on the CPU, against the stand-in runtime of tests/cpp/fake_hip
// (tests/test_host_transfer.py compiles and runs this under AddressSanitizer and UBSan).  The kernel of a chunk is a host
// transpose that puts itself into the log; the budget is 32 instances of 3 labels, so that every chunk is 32 instances.
// argv[1] names the check, the exit status is 0 when it holds.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "host_transfer.h"

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

struct Label {
    uint64_t lo, hi;
    bool operator==(const Label &o) const { return lo == o.lo && hi == o.hi; }
};
Label operator^(Label a, Label b) { return Label{a.lo ^ b.lo, a.hi ^ b.hi}; }

constexpr uint32_t kN = 3;                              // labels of an instance
constexpr size_t kBudget = 32 * kN * sizeof(Label);     // a chunk of 32 instances (16 in wire mode, rounded up to 32)
constexpr uint32_t kBatches[] = {1, 31, 32, 33, 64, 65, 97};
constexpr size_t kStride = 7, kCol0 = 2;                // the strided source: labels [kCol0, kCol0 + kN) of rows of kStride

enum Case { kReadLabels, kReadWires, kWriteDense, kWriteStrided, kCases };

// the device side: an array [row][instance] with `bstride` instances to the row, and R of every instance
struct Device {
    uint32_t batch, bstride;
    std::vector<Label> W, R;
    explicit Device(uint32_t b) : batch(b), bstride((b + 31u) & ~31u), W((size_t)kN * bstride), R(bstride) {}
    void fill() {
        uint64_t x = 0x9e3779b97f4a7c15ull * (batch + 1);
        for (Label &l : W) l = Label{x += 0x632be59bd9b4e019ull, x * 3};
        for (Label &l : R) l = Label{x += 0x632be59bd9b4e019ull, x * 5};
    }
};

// what the pipe was given, for one run
struct Run {
    hipStream_t work = (hipStream_t)std::malloc(sizeof(fake_hip_stream));
    TransferPipe pipe;
    Run() { pipe.work = work; }
    ~Run() {
        pipe.release();
        std::free(work);
    }
    Run(const Run &) = delete;
    Run &operator=(const Run &) = delete;
};

size_t elems_of(Case c) { return c == kReadWires ? 2 * kN : kN; }

// one transfer of case `c`; `host` is the caller's array (read: written; write: read)
int transfer(Run &r, Case c, bool pinned, Device &d, std::vector<Label> &host) {
    const size_t elems = elems_of(c), per_inst = elems * sizeof(Label);
    if (c == kReadLabels || c == kReadWires)
        return download(r.pipe, pinned, d.batch, per_inst, kBudget, host.data(), [&](void *stage, uint32_t i0, uint32_t cnt) {
            const hipError_t e = call(kOperation, stage, cnt * per_inst, r.work);
            if (e != hipSuccess) return e;
            Label *st = (Label *)stage;
            for (uint32_t i = 0; i < cnt; i++)
                for (uint32_t w = 0; w < kN; w++) {
                    const Label l0 = d.W[(size_t)w * d.bstride + i0 + i];
                    if (c == kReadLabels) st[i * elems + w] = l0;
                    else st[i * elems + 2 * w] = l0, st[i * elems + 2 * w + 1] = l0 ^ d.R[i0 + i];
                }
            return hipSuccess;
        });
    const size_t stride = c == kWriteStrided ? kStride : kN;
    const Label *src = host.data() + (c == kWriteStrided ? kCol0 : 0);
    return upload(r.pipe, pinned, d.batch, per_inst, kBudget, src, stride * sizeof(Label), [&](const void *stage, uint32_t i0, uint32_t cnt) {
        const hipError_t e = call(kOperation, stage, cnt * per_inst, r.work);
        if (e != hipSuccess) return e;
        const Label *st = (const Label *)stage;
        for (uint32_t i = 0; i < cnt; i++)
            for (uint32_t w = 0; w < kN; w++) d.W[(size_t)w * d.bstride + i0 + i] = st[i * kN + w];
        return hipSuccess;
    });
}

// the caller's array of a case, sized exactly (ASan sees a copy past it); a write case's is filled
std::vector<Label> host_array(Case c, uint32_t batch) {
    const size_t stride = c == kWriteStrided ? kStride : elems_of(c);
    std::vector<Label> h((size_t)batch * stride);
    uint64_t x = 77 + batch;
    if (c == kWriteDense || c == kWriteStrided)
        for (Label &l : h) l = Label{x += 0x2545f4914f6cdd1dull, x * 7};
    return h;
}

// host bytes against the direct transpose
int check_data(Case c, const Device &d, const std::vector<Label> &host) {
    const size_t stride = c == kWriteStrided ? kStride : elems_of(c), col0 = c == kWriteStrided ? kCol0 : 0;
    for (uint32_t i = 0; i < d.batch; i++)
        for (uint32_t w = 0; w < kN; w++) {
            const Label dev = d.W[(size_t)w * d.bstride + i];
            if (c == kReadWires) {
                CHECK(host[i * stride + 2 * w] == dev);
                CHECK(host[i * stride + 2 * w + 1] == (dev ^ d.R[i]));
            } else {
                CHECK(host[i * stride + col0 + w] == dev);
            }
        }
    return 0;
}

bool enqueues(Op op) { return op == kCopyIn || op == kCopyOut || op == kOperation || op == kRecord || op == kWaitEvent; }

// The order that the log's streams and event edges give.  before[i][s] is the last entry on stream s (0 work, 1 copy) that
// has run when entry i, an entry on a stream, runs: its own stream's entries up to itself, and what an event it waited for had
// seen when it was recorded.  -1: none.
struct Order {
    std::vector<long> before[2];
    int err = 0;
    Order(const Run &r, size_t first) {
        const std::vector<Event> &log = state().log;
        long now[2][2] = {{-1, -1}, {-1, -1}};  // [stream][of stream]
        std::map<hipEvent_t, std::pair<long, long>> recorded;
        before[0].assign(log.size(), -1);
        before[1].assign(log.size(), -1);
        for (size_t i = first; i < log.size(); i++) {
            const Event &ev = log[i];
            if (!enqueues(ev.op) && ev.op != kWait) continue;
            if (ev.stream != r.work && ev.stream != r.pipe.copy) {
                err = 1;
                return;
            }
            const int s = ev.stream == r.pipe.copy;
            if (ev.op == kWaitEvent) {
                if (!recorded.count(ev.event)) {  // (a wait for an event never recorded orders nothing)
                    err = 1;
                    return;
                }
                now[s][0] = std::max(now[s][0], recorded[ev.event].first);
                now[s][1] = std::max(now[s][1], recorded[ev.event].second);
            }
            now[s][s] = (long)i;
            if (ev.op == kRecord) recorded[ev.event] = {now[s][0], now[s][1]};
            before[0][i] = now[s][0];
            before[1][i] = now[s][1];
        }
    }
};

// the last entry of kind `op` on buffer `dev` ahead of entry i; -1: none
long last_on(Op op, const void *dev, size_t first, size_t i) {
    for (size_t j = i; j-- > first;)
        if (state().log[j].op == op && state().log[j].dev == dev) return (long)j;
    return -1;
}

// the log of a clean transfer from entry `first` (behind ensure's entries)
int check_order(const Run &r, Case c, bool pinned, uint32_t batch, size_t first) {
    const std::vector<Event> &log = state().log;
    const bool read = c == kReadLabels || c == kReadWires;
    const Op copy_op = read ? kCopyOut : kCopyIn;
    const hipStream_t work = r.work, copy = r.pipe.copy;
    const size_t chunks = (batch + 31) / 32;
    for (const Event &ev : log) CHECK(ev.ok);
    size_t kernels = 0, copies = 0, waits = 0, edges = 0, copied = 0;
    for (size_t i = first; i < log.size(); i++) {
        const Event &ev = log[i];
        CHECK(ev.op != kMalloc && ev.op != kFree);
        kernels += ev.op == kOperation;
        copies += ev.op == copy_op;
        waits += ev.op == kWait;
        edges += ev.op == kRecord || ev.op == kWaitEvent;
        if (ev.op == copy_op) {
            CHECK(ev.bytes == std::min<size_t>(32, batch - 32 * (copies - 1)) * elems_of(c) * sizeof(Label));
            copied += ev.bytes;
        }
        CHECK(ev.op != (read ? kCopyIn : kCopyOut));
    }
    CHECK(kernels == chunks && copies == chunks && copied == (size_t)batch * elems_of(c) * sizeof(Label));
    if (!pinned) {  // kernel and copy on the work stream, one buffer, a wait behind every chunk
        CHECK(edges == 0 && waits == chunks && log.size() == first + 3 * chunks);
        for (size_t k = 0; k < chunks; k++) {
            const Event *e = &log[first + 3 * k];
            CHECK(e[read ? 0 : 1].op == kOperation && e[read ? 1 : 0].op == copy_op && e[2].op == kWait);
            for (int j = 0; j < 3; j++) CHECK(e[j].stream == work);
            CHECK(e[0].dev == r.pipe.stage[0] && e[1].dev == r.pipe.stage[0]);
        }
        return 0;
    }
    const Order o(r, first);
    CHECK(o.err == 0);
    CHECK(waits == 1 && log.back().op == kWait && log.back().stream == (read ? copy : work));  // the one wait, at the end
    if (!read) {  // the guard at the head: what the work stream holds so far is ahead of the first copy
        CHECK(log[first].op == kRecord && log[first].stream == work);
        CHECK(log[first + 1].op == kWaitEvent && log[first + 1].stream == copy && log[first + 1].event == log[first].event);
    }
    size_t k_kernel = 0, k_copy = 0;
    for (size_t i = first; i < log.size(); i++) {
        const Event &ev = log[i];
        if (ev.op == kOperation) {
            CHECK(ev.stream == work && ev.dev == r.pipe.stage[k_kernel & 1]);
            const long c_prev = last_on(copy_op, ev.dev, first, i);
            if (read) {  // behind the previous copy out of its buffer
                CHECK((c_prev >= 0) == (k_kernel >= 2));
                CHECK(o.before[1][i] >= c_prev);
            } else {  // behind its own copy
                CHECK(c_prev >= 0 && o.before[1][i] >= c_prev);
                CHECK(last_on(kOperation, ev.dev, first, i) < c_prev);
            }
            k_kernel++;
        } else if (ev.op == copy_op) {
            CHECK(ev.stream == copy && ev.dev == r.pipe.stage[k_copy & 1]);
            const long k_prev = last_on(kOperation, ev.dev, first, i);
            if (read) {  // behind its own kernel
                CHECK(k_prev >= 0 && o.before[0][i] >= k_prev);
                CHECK(last_on(copy_op, ev.dev, first, i) < k_prev);
            } else {  // behind the previous scatter of its buffer
                CHECK((k_prev >= 0) == (k_copy >= 2));
                CHECK(o.before[0][i] >= k_prev);
            }
            k_copy++;
        }
    }
    return 0;
}

// 1. the chunk rule, from its definition: max(32, min(batch, budget / per_inst)) rounded up to 32, and a staging buffer of
// min(chunk, batch rounded up to 32) instances
int check_chunk_rule() {
    struct {
        uint32_t batch;
        size_t per_inst, budget;
        uint32_t chunk;
        size_t stage_inst;
    } want[] = {
        {300, 14887 * 16, (size_t)32 << 20, 160, 160},  // 140 fit
        {300, 36663 * 16, (size_t)32 << 20, 64, 64},    // 57 fit
        {300, 36663 * 16, (size_t)64 << 20, 128, 128},  // 114 fit
        {300, 16, (size_t)64 << 20, 320, 320},          // the batch fits: one chunk
        {1, 48, 32 * 48, 32, 32},
        {31, 48, 32 * 48, 32, 32},
        {32, 48, 32 * 48, 32, 32},
        {33, 48, 32 * 48, 32, 32},
        {97, 48, 32 * 48, 32, 32},
        {97, 96, 32 * 48, 32, 32},                      // 16 fit: no fewer than 32
        {97, 48, (size_t)1 << 20, 128, 128},
        {33, 48, 64 * 48, 64, 64},                      // 64 fit, 33 asked
        {40, 48, 33 * 48, 64, 64},                      // 33 fit: up to the next 32
        {5, (size_t)100 << 20, (size_t)64 << 20, 32, 32},  // not one fits
        {1000, 1 << 20, (size_t)64 << 20, 64, 64},
        {64, 1 << 20, (size_t)128 << 20, 64, 64},
        {33, 1 << 20, (size_t)128 << 20, 64, 64},
        {4097, 16, (size_t)1 << 16, 4096, 4096},
        {4000, 16, (size_t)1 << 16, 4000, 4000},  // 125 * 32: whole already
    };
    for (const auto &w : want) {
        const Chunks c = chunk_rule(w.batch, w.per_inst, w.budget);
        CHECK(c.chunk == w.chunk);
        CHECK(c.stage_bytes == w.stage_inst * w.per_inst);
    }
    return 0;
}

// 2. data and 3. order of a clean run: every case, both forms, every batch; the second transfer on the same pipe creates
// nothing and allocates nothing
int check_clean_runs() {
    for (uint32_t batch : kBatches)
        for (int ci = 0; ci < kCases; ci++)
            for (bool pinned : {false, true}) {
                const Case c = (Case)ci;
                reset();
                g_errors = 0;
                Run r;
                Device d(batch);
                if (c == kReadLabels || c == kReadWires) d.fill();
                std::vector<Label> host = host_array(c, batch);
                CHECK(transfer(r, c, pinned, d, host) == GC_OK && g_errors == 0);
                CHECK(check_data(c, d, host) == 0);
                const size_t made = 9;  // the copy stream, four events, (two waits,) two buffers
                CHECK(state().log.size() > made && state().log[made - 1].op == kMalloc && state().log[made].op != kMalloc);
                CHECK(state().log[made - 1].bytes == 32 * elems_of(c) * sizeof(Label));
                CHECK(check_order(r, c, pinned, batch, made) == 0);
                const size_t first = state().log.size();
                CHECK(transfer(r, c, pinned, d, host) == GC_OK && check_data(c, d, host) == 0);
                CHECK(check_order(r, c, pinned, batch, first) == 0);
            }
    return 0;
}

// 4. ensure and release
int check_ensure() {
    reset();
    {
        Run r;
        CHECK(r.pipe.ensure(100) == GC_OK);
        const std::vector<Event> &log = state().log;
        const Op made[] = {kStreamCreate, kEventCreate, kEventCreate, kEventCreate, kEventCreate, kWait, kWait, kMalloc, kMalloc};
        CHECK(log.size() == 9);
        for (size_t i = 0; i < 9; i++) CHECK(log[i].op == made[i] && log[i].ok);
        CHECK(log[7].bytes == 100 && log[8].bytes == 100 && r.pipe.stage_cap == 100);
        const void *old0 = r.pipe.stage[0], *old1 = r.pipe.stage[1];
        CHECK(r.pipe.ensure(100) == GC_OK && r.pipe.ensure(1) == GC_OK && log.size() == 9);  // no growth: no call at all
        CHECK(r.pipe.ensure(101) == GC_OK && r.pipe.stage_cap == 101);
        const Op grown[] = {kWait, kWait, kFree, kFree, kMalloc, kMalloc};  // both streams, then the frees
        CHECK(log.size() == 15);
        for (size_t i = 0; i < 6; i++) CHECK(log[9 + i].op == grown[i]);
        CHECK(log[9].stream == r.work && log[10].stream == r.pipe.copy);
        CHECK(log[11].dev == old0 && log[12].dev == old1 && log[13].bytes == 101 && log[14].bytes == 101);
    }
    // the release: every buffer, event and stream once
    std::map<const void *, int> live;
    for (const Event &ev : state().log) {
        if (ev.op == kMalloc) live[ev.dev]++;
        if (ev.op == kStreamCreate) live[ev.stream]++;
        if (ev.op == kEventCreate) live[ev.event]++;
        if (ev.op == kFree) CHECK(live[ev.dev]-- == 1);
        if (ev.op == kStreamDestroy) CHECK(live[ev.stream]-- == 1);
        if (ev.op == kEventDestroy) CHECK(live[ev.event]-- == 1);
    }
    CHECK(live.size() == 9);
    for (const auto &kv : live) CHECK(kv.second == 0);
    // a failure at every call of a first ensure and of a growth: the status, one set_error, and (ASan) no leak behind release
    for (long at = 0; at < 9 + 4; at++)
        for (hipError_t code : {hipErrorOutOfMemory, hipErrorUnknown}) {
            reset(at, code);
            g_errors = 0;
            Run r;
            const int rc1 = r.pipe.ensure(100), rc2 = rc1 == GC_OK ? r.pipe.ensure(200) : GC_OK;
            CHECK((at < 9 ? rc1 : rc2) == (code == hipErrorOutOfMemory ? GC_E_NOMEM : GC_E_HIP));
            CHECK((at < 9 ? rc2 : rc1) == GC_OK && g_errors == 1);
            if (at >= 9 && at < 11) CHECK(r.pipe.stage_cap == 100);  // a wait failed: the buffers stay
            if (at >= 11) CHECK(r.pipe.stage_cap == 0);
            CHECK(r.pipe.ensure(300) == GC_OK && r.pipe.stage_cap == 300);  // and the pipe recovers
        }
    return 0;
}

// 5. a failure at every fallible call of every clean run above (ensure's calls included)
int check_failures() {
    for (uint32_t batch : kBatches)
        for (int ci = 0; ci < kCases; ci++)
            for (bool pinned : {false, true}) {
                const Case c = (Case)ci;
                long calls;
                {
                    reset();
                    Run r;
                    Device d(batch);
                    std::vector<Label> host = host_array(c, batch);
                    CHECK(transfer(r, c, pinned, d, host) == GC_OK);
                    calls = state().calls;
                }
                for (long at = 0; at < calls; at++)
                    for (hipError_t code : {hipErrorOutOfMemory, hipErrorUnknown}) {
                        reset(at, code);
                        g_errors = 0;
                        Run r;
                        Device d(batch);
                        std::vector<Label> host = host_array(c, batch);
                        CHECK(transfer(r, c, pinned, d, host) == (code == hipErrorOutOfMemory ? GC_E_NOMEM : GC_E_HIP));
                        CHECK(g_errors == 1);
                        // for each stream: nothing is queued on it behind its last wait; no buffer is freed
                        const std::vector<Event> &log = state().log;
                        long last_wait[2] = {-1, -1}, last_queued[2] = {-1, -1};
                        size_t failed = 0;
                        for (size_t i = 0; i < log.size(); i++) {
                            const Event &ev = log[i];
                            failed += !ev.ok;
                            CHECK(ev.op != kFree);
                            if (!enqueues(ev.op) && ev.op != kWait) continue;
                            CHECK(ev.stream == r.work || ev.stream == r.pipe.copy);
                            long *what = ev.op == kWait ? last_wait : last_queued;
                            if (ev.op != kWait || ev.ok) what[ev.stream == r.pipe.copy] = (long)i;
                        }
                        CHECK(failed == 1);
                        for (int s = 0; s < 2; s++) CHECK(last_queued[s] < 0 || last_wait[s] > last_queued[s]);
                        // the pipe serves the next call
                        Device d2(batch);
                        if (c == kReadLabels || c == kReadWires) d2.fill();
                        std::vector<Label> host2 = host_array(c, batch);
                        CHECK(transfer(r, c, pinned, d2, host2) == GC_OK && check_data(c, d2, host2) == 0);
                    }  // (~Run: the release; ASan reports what it leaves)
            }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    const std::string which = argc == 2 ? argv[1] : "";
    if (which == "chunk_rule") return check_chunk_rule();
    if (which == "clean") return check_clean_runs();
    if (which == "ensure") return check_ensure();
    if (which == "failures") return check_failures();
    return 2;
}
