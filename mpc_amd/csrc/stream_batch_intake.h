// stream_batch_intake.h — the framing state behind gc_stream_eval_batch_in_* (DESIGN.md §20), as plain host state: how many
// bytes of an unfinished message are held, where the next message starts, what a feed of n bytes does, carry growth and its
// cap, the stop in front of an op that is not OpCircuit, and the four counters.  No HIP call and no lock in here:
// stream_batch.cpp wraps the uploads, the copies and the evaluation around it, and tests/cpp/stream_batch_intake_check.cpp
// drives it on a CPU.
//
// All sessions of a handle run one program and write the same number of bytes per step, so one offset serves every session
// and only the REFERENCE session's bytes are ever looked at on the host.  A feed is planned first (plan_feed changes
// nothing); the engine makes the buffer the plan asks for — [the kept tail | the new chunk] —, then walks the messages in it
// (frame() says what stands at an offset, apply() moves the plan on), and commits at the end, so that a failed allocation
// leaves no trace.  The loop is the one of circuit/stream_evaluator.go:227-249: BE32 op, and for OpCircuit BE32 step,
// numGates, numTmpWires, numWires in front of the block.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/gcengine.h"

namespace gcsb {

struct Intake {
    static constexpr uint32_t kOpCircuit = 1;
    static constexpr size_t kHeader = 20;

    size_t max_message = 0;  // the most bytes of one message (header included) the handle holds
    size_t held = 0;         // bytes per session of the open message: the front of the buffer the last feed filled
    uint64_t steps = 0, bytes_per_session = 0, uploads = 0, carried_bytes = 0;

    // false: a cap below one header
    bool init(size_t max_message_bytes) {
        if (max_message_bytes < kHeader) return false;
        max_message = max_message_bytes, held = 0;
        steps = bytes_per_session = uploads = carried_bytes = 0;
        return true;
    }

    static uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

    struct Header {
        uint32_t step = 0, ngates = 0, ntmp = 0, nwires = 0;
    };

    // what stands at an offset of the held bytes
    enum Kind {
        kMessage,  // a complete OpCircuit message of `len` bytes (from frame(): its header is complete, the block is the parser's)
        kMore,     // the bytes end inside it
        kForeign,  // a complete op word `op` that is not OpCircuit
        kRefused   // `rc`: the parser's refusal, or a message that cannot fit under the cap
    };
    struct Found {
        Kind kind = kMore;
        size_t len = 0;
        uint32_t op = kOpCircuit;
        int rc = GC_OK;
    };

    // The framing of the message at p, of which `avail` bytes are there.  A header that claims more gates than the cap has
    // room for (a gate is 5 bytes at the least, as gc_stream_eval_circuit counts) is refused at once: the handle never buffers
    // towards a size the peer only claims.  kMessage: *h is complete and the block starts at p + kHeader.
    Found frame(const uint8_t *p, size_t avail, Header *h) const {
        Found x;
        if (avail < 4) return x;
        x.op = be32(p);
        if (x.op != kOpCircuit) {
            x.kind = kForeign;
            return x;
        }
        if (avail < kHeader) return x;
        h->step = be32(p + 4), h->ngates = be32(p + 8), h->ntmp = be32(p + 12), h->nwires = be32(p + 16);
        if ((uint64_t)h->ngates * 5u + kHeader > (uint64_t)max_message) {
            x.kind = kRefused, x.rc = GC_E_ROWS;
            return x;
        }
        x.kind = kMessage;
        return x;
    }

    struct Feed {
        size_t keep = 0, n = 0, width = 0;  // the buffer reads [keep bytes of the last feed | n new bytes] = width
        size_t at = 0;                      // where the next message starts
        uint64_t steps = 0;                 // complete messages so far, all evaluated
        // the outcome, once apply() has returned false
        size_t taken = 0, carry = 0;
        uint32_t next_op = kOpCircuit;
        int rc = GC_OK;
    };

    // a feed of n bytes per session; changes nothing
    Feed plan_feed(size_t n) const {
        Feed f;
        f.keep = held, f.n = n, f.width = held + n;
        return f;
    }
    static size_t avail(const Feed &f) { return f.width - f.at; }

    // What was found at f.at.  true: a message has been passed, look at f.at again.  false: the feed is over —
    //   kMore     all n bytes are taken and avail() of them are carried; a carry beyond the cap is GC_E_ROWS instead
    //   kForeign  f.next_op = the op; the feed stops in front of the word
    //   kRefused  f.rc = the code; the feed stops in front of the message
    // A stopped feed takes the bytes of this chunk in front of f.at and carries nothing: if the word or message began in an
    // earlier chunk (f.at < f.keep) that is 0 bytes, and the held ones are dropped.
    bool apply(Feed &f, const Found &x) const {
        if (x.kind == kMessage) {
            f.at += x.len, f.steps++;
            return true;
        }
        if (x.kind == kMore && avail(f) <= max_message) {
            f.taken = f.n, f.carry = avail(f);
            return false;
        }
        f.taken = f.at > f.keep ? f.at - f.keep : 0, f.carry = 0;
        if (x.kind == kForeign) f.next_op = x.op;
        else f.rc = x.kind == kMore ? GC_E_ROWS : x.rc;
        return false;
    }

    // the plan has been carried out: `uploaded` says whether the chunk went to the device (an empty chunk does not)
    void commit(const Feed &f, bool uploaded) {
        steps += f.steps, bytes_per_session += f.at;
        held = f.carry, carried_bytes += f.carry;
        if (uploaded) uploads++;
    }
};

}  // namespace gcsb
