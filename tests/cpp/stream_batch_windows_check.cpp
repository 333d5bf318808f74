// stream_batch_windows_check.cpp — drives mpc_amd/csrc/stream_batch_windows.h, the ring state of gc_stream_batch_out_*, the
// way stream_batch.cpp drives it (plan, then commit; a busy answer is only counted), without any device: a script of
// events on stdin, one line of outcome and full ring state per event on stdout.  tests/test_stream_batch_windows.py holds
// the model the lines are compared with.  Built with AddressSanitizer and UBSan.
//   i <window_bytes> <nwindows>   a new ring        s <n>   a step of n bytes     f   flush     n   next     r   release
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "stream_batch_windows.h"

using gcsb::WindowRing;

static void state(const WindowRing &r) {
    const uint32_t f = r.filling();
    std::printf(" | %d %zu %u %u | %llu %llu %llu %llu |", f == WindowRing::kNoWindow ? -1 : (int)f, r.off, r.n_out, r.n_sealed,
                (unsigned long long)r.sealed, (unsigned long long)r.bytes_per_session, (unsigned long long)r.grown,
                (unsigned long long)r.busy);
    for (uint32_t k = 0; k < r.count(); k++) std::printf(" %zu", r.cap[k]);
    std::printf(" |");
    for (uint32_t k = 0; k < r.count(); k++) std::printf(" %zu", r.len[k]);
    std::printf("\n");
}

int main() {
    WindowRing r;
    char ev = 0;
    bool have = false;
    while (std::scanf(" %c", &ev) == 1) {
        if (ev == 'i') {
            unsigned long long wb = 0;
            unsigned nw = 0;
            if (std::scanf("%llu %u", &wb, &nw) != 2) return 2;
            have = r.init((size_t)wb, nw);
            std::printf("i %s", have ? "ok" : "refused");
            if (have) state(r);
            else std::printf("\n");
            continue;
        }
        if (!have) return 3;
        if (ev == 's') {
            unsigned long long n = 0;
            if (std::scanf("%llu", &n) != 1 || n == 0) return 2;
            const WindowRing before = r;
            const WindowRing::Step p = r.plan_step((size_t)n);
            // planning changes nothing
            if (before.cap != r.cap || before.len != r.len || before.off != r.off || before.first != r.first || before.n_out != r.n_out ||
                before.n_sealed != r.n_sealed || before.sealed != r.sealed || before.grown != r.grown || before.busy != r.busy)
                return 4;
            if (p.is_busy) {
                r.note_busy();
                std::printf("s busy");
            } else {
                if (p.grow_to && (p.at != 0 || p.grow_to % 4096 != 0 || p.grow_to < n || p.grow_to <= before.cap[p.win])) return 5;
                if (p.at + n > (p.grow_to ? p.grow_to : r.cap[p.win])) return 6;  // the step lies inside its window
                r.commit(p, (size_t)n);
                std::printf("s ok %u %zu %zu", p.win, p.at, p.grow_to);
                if (p.seal_before != WindowRing::kNoWindow) std::printf(" (%u %zu)", p.seal_before, p.seal_len);
                if (p.seal_after) std::printf(" (%u %zu)", p.win, p.at + (size_t)n);
            }
        } else if (ev == 'f') {
            size_t n = 0;
            const uint32_t w = r.plan_flush(&n);
            if (w == WindowRing::kNoWindow) {
                std::printf("f none");
            } else {
                r.commit_flush();
                std::printf("f (%u %zu)", w, n);
            }
        } else if (ev == 'n') {
            size_t n = 0;
            const uint32_t w = r.next(&n);
            if (w == WindowRing::kNoWindow) std::printf("n none");
            else std::printf("n (%u %zu)", w, n);
        } else if (ev == 'r') {
            const uint32_t w = r.release();
            if (w == WindowRing::kNoWindow) std::printf("r none");
            else std::printf("r %u", w);
        } else {
            return 2;
        }
        state(r);
    }
    return 0;
}
