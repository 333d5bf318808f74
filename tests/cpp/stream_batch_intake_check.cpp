// stream_batch_intake_check.cpp — drives mpc_amd/csrc/stream_batch_intake.h, the framing state of gc_stream_eval_batch_in_*, the
// way stream_batch.cpp drives it (plan a feed, put the chunk behind the kept tail, frame() / apply() over the messages,
// commit), without any device: a script on stdin, one line per feed on stdout.  tests/test_stream_batch_intake.py holds the
// model the lines are compared with.  Built with AddressSanitizer and UBSan.
//   i <max_message_bytes>            a new intake and an empty stream
//   M <len> <numGates>               appends an OpCircuit message of len >= 20 bytes: step = its index, numTmpWires = len - 20
//                                    (this driver's "block parser": the block is as long as numTmpWires says)
//   F <op> <len>                     appends a foreign message: the op word and len - 4 bytes that the CALLER reads
//   c <n>                            feeds the next n bytes of the stream (fewer at its end)
// A line: rc taken next_op held | steps bytes uploads carried | offset:len:step of every message evaluated.  Behind a stop
// the driver goes on behind the foreign message, behind a refusal behind the refused message — as a caller would.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "stream_batch_intake.h"

using gcsb::Intake;

struct Item {
    size_t start, len;
};

static void put32(std::vector<uint8_t> &s, uint32_t v) {
    for (int k = 3; k >= 0; k--) s.push_back((uint8_t)(v >> (8 * k)));
}

int main() {
    Intake in;
    bool have = false;
    std::vector<uint8_t> stream, tail;
    std::vector<Item> items;
    size_t pos = 0;
    char ev = 0;
    while (std::scanf(" %c", &ev) == 1) {
        if (ev == 'i') {
            unsigned long long cap = 0;
            if (std::scanf("%llu", &cap) != 1) return 2;
            have = in.init((size_t)cap);
            stream.clear(), tail.clear(), items.clear(), pos = 0;
            std::printf("i %s\n", have ? "ok" : "refused");
            continue;
        }
        if (!have) return 3;
        if (ev == 'M' || ev == 'F') {
            unsigned long long a = 0, b = 0;
            if (std::scanf("%llu %llu", &a, &b) != 2) return 2;
            const size_t len = (size_t)(ev == 'M' ? a : b);
            if (len < (ev == 'M' ? Intake::kHeader : 4)) return 2;
            items.push_back(Item{stream.size(), len});
            if (ev == 'M') {
                put32(stream, Intake::kOpCircuit), put32(stream, (uint32_t)items.size() - 1), put32(stream, (uint32_t)b);
                put32(stream, (uint32_t)(len - Intake::kHeader)), put32(stream, 0);
            } else {
                put32(stream, (uint32_t)a);
            }
            while (stream.size() < items.back().start + len) stream.push_back((uint8_t)(0xC0 + stream.size() % 61));
            continue;
        }
        if (ev != 'c') return 2;
        unsigned long long want = 0;
        if (std::scanf("%llu", &want) != 1) return 2;
        const size_t n = want < stream.size() - pos ? (size_t)want : stream.size() - pos;
        if (n == 0) {
            std::printf("c end\n");
            continue;
        }
        const Intake before = in;
        Intake::Feed f = in.plan_feed(n);
        // planning changes nothing
        if (before.held != in.held || before.steps != in.steps || before.bytes_per_session != in.bytes_per_session ||
            before.uploads != in.uploads || before.carried_bytes != in.carried_bytes)
            return 4;
        if (f.keep != tail.size() || f.width != tail.size() + n) return 5;
        std::vector<uint8_t> buf(tail);  // (a buffer of exactly the planned width: the sanitizer sees a byte too many)
        buf.insert(buf.end(), stream.begin() + (long)pos, stream.begin() + (long)(pos + n));
        const size_t buf_abs = pos - tail.size();
        std::vector<Item> seen;
        std::vector<uint32_t> seen_step;
        for (;;) {
            Intake::Header h;
            Intake::Found x = in.frame(buf.data() + f.at, Intake::avail(f), &h);
            if (x.kind == Intake::kMessage) {
                if (Intake::avail(f) < Intake::kHeader + (size_t)h.ntmp) x.kind = Intake::kMore;
                else x.len = Intake::kHeader + h.ntmp, seen.push_back(Item{buf_abs + f.at, x.len}), seen_step.push_back(h.step);
            }
            if (!in.apply(f, x)) break;
            if (f.at > f.width) return 6;
        }
        if (f.taken > n || f.carry > Intake::avail(f) || f.carry > in.max_message) return 7;
        in.commit(f, true);
        tail.assign(buf.begin() + (long)f.at, buf.begin() + (long)(f.at + f.carry));
        std::printf("%d %zu %u %zu | %llu %llu %llu %llu |", f.rc, f.taken, f.next_op, in.held, (unsigned long long)in.steps,
                    (unsigned long long)in.bytes_per_session, (unsigned long long)in.uploads, (unsigned long long)in.carried_bytes);
        for (size_t k = 0; k < seen.size(); k++) std::printf(" %zu:%zu:%u", seen[k].start, seen[k].len, seen_step[k]);
        std::printf("\n");
        pos += f.taken;
        if (f.rc != GC_OK || f.next_op != Intake::kOpCircuit) {  // the caller steps over what the feed stopped in front of
            const size_t at = buf_abs + f.at;
            bool found = false;
            for (const Item &it : items)
                if (it.start == at) pos = it.start + it.len, found = true;
            if (!found) return 8;
        }
    }
    return 0;
}
