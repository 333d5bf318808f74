// stream_batch_windows.h — the ring of output windows behind gc_stream_batch_out_* (DESIGN.md §18), as plain host state:
// which window fills and at what offset, what a step of n bytes does, which windows are sealed / handed out / free, growth
// and the four counters.  No HIP call and no lock in here: stream_batch.cpp wraps the events, copies and allocations
// around it under the handle's lock, and tests/cpp/stream_batch_windows_check.cpp drives it on a CPU.
//
// All sessions write the same bytes per step, so one offset serves every session.  The windows are used in index order and
// come back in the order they were sealed, so in cyclic order from `first` the ring always reads
//     [handed out ...][sealed ...][filling][free ...]
// and three numbers describe it.  A step is planned first (plan_step changes nothing) and committed once the engine has
// made what the plan asks for — a larger window — so that a failed allocation or a full ring leaves no trace.
// A handle made by gc_stream_batch_out_create_split uses plan_split / commit_split instead of plan_step / commit (never both
// on one ring): the same state, the same flush / next / release, and a step that is cut over the windows.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace gcsb {

struct WindowRing {
    static constexpr uint32_t kNoWindow = 0xffffffffu;
    static size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }
    static size_t up4096(size_t n) { return (n + 4095) & ~(size_t)4095; }

    std::vector<size_t> cap;  // per window (a grown window keeps its size)
    std::vector<size_t> len;  // bytes per session of a sealed or handed-out window; the filling window's are `off`
    uint32_t first = 0;       // the oldest window that is not free
    uint32_t n_out = 0, n_sealed = 0;
    size_t off = 0;           // bytes per session in the filling window
    uint64_t sealed = 0, bytes_per_session = 0, grown = 0, busy = 0;

    // false: fewer than two windows
    bool init(size_t window_bytes, uint32_t nwindows) {
        if (nwindows < 2) return false;
        cap.assign(nwindows, up16(window_bytes));
        len.assign(nwindows, 0);
        first = n_out = n_sealed = 0, off = 0;
        sealed = bytes_per_session = grown = busy = 0;
        return true;
    }
    uint32_t count() const { return (uint32_t)cap.size(); }
    // the window a step would write into, or kNoWindow when every window is sealed or handed out
    uint32_t filling() const { return n_out + n_sealed < count() ? (first + n_out + n_sealed) % count() : kNoWindow; }

    struct Step {
        bool is_busy = false;
        uint32_t seal_before = kNoWindow;  // sealed (at seal_len bytes) ahead of the step: the step does not fit behind them
        size_t seal_len = 0;
        uint32_t win = kNoWindow;  // where the step's bytes go, at offset `at`
        size_t at = 0;
        size_t grow_to = 0;        // not 0: `win` is empty and smaller than the step; it must have this size first
        bool seal_after = false;   // the step fills `win` exactly
    };

    // what a step of n > 0 bytes per session does; changes nothing
    Step plan_step(size_t n) const {
        Step p;
        uint32_t w = filling();
        size_t at = off;
        if (w == kNoWindow) {
            p.is_busy = true;
            return p;
        }
        if (at != 0 && at + n > cap[w]) {  // seal what is there and go on in the next window, if one is free
            if (n_out + n_sealed + 1 >= count()) {
                p.is_busy = true;
                return p;
            }
            p.seal_before = w, p.seal_len = at;
            w = (w + 1) % count(), at = 0;
        }
        if (at == 0 && n > cap[w]) p.grow_to = up4096(n);
        p.win = w, p.at = at;
        p.seal_after = at + n == (p.grow_to ? p.grow_to : cap[w]);
        return p;
    }
    void note_busy() { busy++; }
    // the plan has been carried out (the window grown, the events recorded by the caller)
    void commit(const Step &p, size_t n) {
        if (p.seal_before != kNoWindow) seal(p.seal_before, p.seal_len);
        if (p.grow_to) cap[p.win] = p.grow_to, grown++;
        off = p.at + n;
        bytes_per_session += n;
        if (p.seal_after) seal(p.win, off);
    }
    // ---- the split rule (gc_stream_batch_out_create_split): a step goes behind what the filling window holds and
    // on into the windows after it from their byte 0; no window is sealed short and none grows.  Every window has init's size.
    struct Split {
        bool is_busy = false;    // the filling window or one of the nwin - 1 behind it is sealed or handed out
        bool too_large = false;  // n > (count - 1) * cap: no number of releases guarantees the room (off < cap)
        uint32_t win = kNoWindow;  // the first window, written from offset `at`; window j of the step is (win + j) % count
        size_t at = 0;
        uint32_t nwin = 0;       // windows the step touches: ceil((at + n) / cap)
        uint32_t nsealed = 0;    // the first nsealed of them become exactly full: nwin, or nwin - 1 when the last one does not
        // segment j: bytes [begin(j), begin(j + 1)) of the step, written at offset (j ? 0 : at) of window j
        size_t begin(uint32_t j, size_t n, size_t cap_) const { return j == 0 ? 0 : j >= nwin ? n : (size_t)j * cap_ - at; }
    };

    // what a step of n > 0 bytes per session does under the split rule; changes nothing
    Split plan_split(size_t n) const {
        Split p;
        const size_t c = cap[0];
        if (n > (size_t)(count() - 1) * c) {
            p.too_large = true;
            return p;
        }
        const uint32_t w = filling();
        if (w == kNoWindow) {
            p.is_busy = true;
            return p;
        }
        const size_t end = off + n;
        const uint32_t k = (uint32_t)((end + c - 1) / c);
        if (n_out + n_sealed + k > count()) {
            p.is_busy = true;
            return p;
        }
        p.win = w, p.at = off, p.nwin = k;
        p.nsealed = end % c == 0 ? k : k - 1;
        return p;
    }
    // the plan has been carried out (every segment launched, the seals' events recorded by the caller)
    void commit_split(const Split &p, size_t n) {
        const size_t c = cap[0];
        for (uint32_t j = 0; j < p.nsealed; j++) seal((p.win + j) % count(), c);
        off = p.at + n - (size_t)p.nsealed * c;
        bytes_per_session += n;
    }

    // flush: the filling window if it holds any byte, else kNoWindow; *n = its bytes
    uint32_t plan_flush(size_t *n) const {
        const uint32_t w = filling();
        if (w == kNoWindow || off == 0) return kNoWindow;
        *n = off;
        return w;
    }
    void commit_flush() { seal(filling(), off); }
    // the oldest sealed window not yet handed out becomes handed out; kNoWindow: nothing is sealed
    uint32_t next(size_t *n) {
        if (n_sealed == 0) return kNoWindow;
        const uint32_t w = (first + n_out) % count();
        n_out++, n_sealed--;
        *n = len[w];
        return w;
    }
    // the oldest handed-out window becomes free; kNoWindow: nothing is handed out
    uint32_t release() {
        if (n_out == 0) return kNoWindow;
        const uint32_t w = first;
        len[w] = 0;
        first = (first + 1) % count(), n_out--;
        return w;
    }

private:
    void seal(uint32_t w, size_t n) {
        len[w] = n;
        n_sealed++, sealed++;
        off = 0;
    }
};

}  // namespace gcsb
