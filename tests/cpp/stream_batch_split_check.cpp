// stream_batch_split_check.cpp — drives the split rule of mpc_amd/csrc/stream_batch_windows.h (plan_split / commit_split, the
// ring state of gc_stream_batch_out_create_split) the way stream_batch.cpp drives it: plan, then commit; a busy answer is only
// counted, a step that is too large leaves nothing.  A script of events on stdin, one line of outcome and full ring state per
// event on stdout; tests/test_stream_batch_split_windows.py holds the model the lines are compared with.  Built with
// AddressSanitizer and UBSan.
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

static bool same(const WindowRing &a, const WindowRing &b) {
    return a.cap == b.cap && a.len == b.len && a.off == b.off && a.first == b.first && a.n_out == b.n_out && a.n_sealed == b.n_sealed &&
           a.sealed == b.sealed && a.bytes_per_session == b.bytes_per_session && a.grown == b.grown && a.busy == b.busy;
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
            const WindowRing::Split p = r.plan_split((size_t)n);
            if (!same(before, r)) return 4;  // planning changes nothing
            if (p.too_large) {
                std::printf("s large");
            } else if (p.is_busy) {
                r.note_busy();
                std::printf("s busy");
            } else {
                const size_t cap = r.cap[0];
                // the segments tile [0, n), each lies inside its window, and every window but the first is written from byte 0
                if (p.nwin == 0 || p.nwin > r.count() || p.nsealed > p.nwin || p.nsealed + 1 < p.nwin) return 5;
                if (p.begin(0, n, cap) != 0 || p.begin(p.nwin, n, cap) != n) return 6;
                for (uint32_t j = 0; j < p.nwin; j++) {
                    const size_t b0 = p.begin(j, n, cap), b1 = p.begin(j + 1, n, cap), at = j ? 0 : p.at;
                    if (b1 <= b0 || at + (b1 - b0) > cap) return 7;
                    if ((at + (b1 - b0) == cap) != (j < p.nsealed)) return 8;
                }
                r.commit_split(p, (size_t)n);
                std::printf("s ok %u %zu %u", p.win, p.at, p.nwin);
                for (uint32_t j = 0; j < p.nsealed; j++) std::printf(" (%u %zu)", (p.win + j) % r.count(), cap);
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
