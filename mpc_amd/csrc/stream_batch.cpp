// stream_batch.cpp — S sessions of ONE streamed program per call (gc_stream_batch_*, gc_stream_eval_batch_*).
// Every session runs the same SSA step on the same circuit with the same in[] / out[]; they differ in key, R and labels.  A
// step is therefore one keyed batch pass over S instances (gc_batch_garble_keyed / gc_batch_eval_keyed) between a gather from
// and a scatter into a device-resident wire store [wire id][bstride], and its bytes are one skeleton for all sessions — the
// op | flag bytes and wire ids of circuit/stream_garble.go:391-441 — plus per-session table rows.  Steps are serial on the ctx
// stream (program order there IS the reference's loop, stream_garble.go:161-192); only the sessions are parallel.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <unordered_map>
#include <vector>

#include "engine.h"
#include "stream_batch.h"
#include "stream_batch_intake.h"
#include "stream_batch_windows.h"
#include "stream_wire.h"

namespace gcs {
uint32_t stream_max_wires();  // stream_eval.cpp (GC_STREAM_MAX_WIRES)
}

using namespace gc;

namespace {

constexpr uint32_t kNone = 0xffffffffu;
constexpr int kRing = 4;  // steps whose constants may be on their way to the device at once

size_t cache_budget() {
    static const size_t v = [] {
        const char *e = std::getenv("GC_STREAM_BATCH_CACHE_BYTES");
        const unsigned long long n = e ? std::strtoull(e, nullptr, 0) : 0;
        return n ? (size_t)n : (size_t)1 << 30;
    }();
    return v;
}

int refuse(const char *what, const char *why) {
    std::snprintf(gc::tls_error, sizeof gc::tls_error, "%s: %s", what, why);
    return GC_E_ARG;
}

inline size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

// ---- the bytes of a step that are the same for every session ---------------------------------------------------------
// (*Streaming).Garble's gate loop (stream_garble.go:385-449) without the labels: op | flags, the wire ids through in[] / out[]
// in their 16- or 32-bit form, and 16 zero bytes per table row.  bytes / row_off may be null (the size alone).
size_t step_skeleton(const gc_gate *gates, uint32_t ngates, uint32_t nwires, const uint32_t *in, uint32_t nin, const uint32_t *out,
                     uint32_t nout, std::vector<uint8_t> *bytes, std::vector<uint32_t> *row_off) {
    size_t pos = 0;
    for (uint32_t g = 0; g < ngates; g++) {
        const gc_gate &q = gates[g];
        const gcw::GateForm f = gcw::gate_form(q.op, q.in0, q.in1, q.out, nin, nwires - nout, in, out);
        if (bytes) {
            bytes->resize(pos + f.size, 0);
            const size_t row0 = (size_t)(gcw::put_gate_head(bytes->data() + pos, f) - bytes->data());
            for (uint32_t r = 0; r < f.rows; r++) row_off->push_back((uint32_t)(row0 + 16u * r));
        }
        pos += f.size;
    }
    return pos;
}

// what every garbler step is checked for before anything is touched; nullptr, or the reason
const char *step_refused(const gc_gate *gates, uint32_t ngates, uint32_t nwires, uint32_t nin, uint32_t nout, int *rc) {
    *rc = GC_E_ARG;
    if (nin > nwires || nout > nwires) return "more inputs or outputs than wires";
    if (nwires - nout < nin) return "the circuit's output range overlaps its input range (nwires - nout < nin)";
    for (uint32_t g = 0; g < ngates; g++) {
        const gc_gate &q = gates[g];
        if (q.op > GC_INV) {
            *rc = GC_E_GATE;
            return "invalid gate type";
        }
        if (q.in0 >= nwires || q.out >= nwires || (q.op != GC_INV && q.in1 >= nwires)) {
            *rc = GC_E_WIRE;
            return "wire id >= nwires";
        }
        if (q.out < nin) return "a gate writes an input-mapped wire";
    }
    return nullptr;
}

// ---- circuits of a handle, recognised by gate-list content -----------------------------------------------------------
struct SbCirc {
    std::vector<gc_gate> gates;  // {in0, in1, out, op}, the rest zero
    uint32_t nwires = 0, nin = 0, nout = 0;
    uint64_t hash = 0, last_use = 0;
    gc_circ *circ = nullptr;
    gc_batch *batch = nullptr;
    size_t dev_bytes = 0;
};

uint64_t content_hash(const gc_gate *g, uint32_t n, uint32_t nwires, uint32_t nin, uint32_t nout) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](uint64_t v) { h = (h ^ v) * 1099511628211ull; };
    mix(n), mix(nwires), mix(nin), mix(nout);
    for (uint32_t i = 0; i < n; i++) mix(((uint64_t)g[i].in0 << 32) | g[i].in1), mix(((uint64_t)g[i].out << 8) | g[i].op);
    return h ^ (h >> 29);
}

struct SbStage {  // the constants of one step: pinned host copy, device copy, and when the device is done with them
    uint8_t *pin = nullptr, *dev = nullptr;
    size_t cap = 0;
    hipEvent_t done = nullptr;
    bool used = false;
};

struct SbCore {
    gc_ctx *ctx = nullptr;
    uint32_t S = 0, bstride = 0;
    size_t keylen = 0;
    uint8_t *d_keys = nullptr;
    uint4 *d_store = nullptr;  // [rows][bstride]: L0 (garbler) / the active label (evaluator); zero = never set
    uint32_t rows = 0;
    std::vector<std::unique_ptr<SbCirc>> cache;
    size_t cache_bytes = 0;
    uint64_t tick = 0;
    uint64_t n_loads = 0, n_evictions = 0;  // misses that ended with an entry kept / entries the budget loop freed
    bool fallback = false;  // gc_stream_*batch_set_fallback: a circuit kept out by the key table alone is loaded on path 2
    SbStage ring[kRing];
    uint32_t next = 0;

    Layout store_layout() const { return Layout{31, 0x7fffffffu, bstride, 0}; }

    ~SbCore() {
        if (ctx) {
            (void)hipSetDevice(ctx->device);
            (void)hipStreamSynchronize(ctx->stream);
        }
        for (auto &e : cache) {
            gc_batch_free(e->batch);
            gc_circ_free(e->circ);
        }
        for (auto &r : ring) {
            if (r.pin) (void)hipHostFree(r.pin);
            if (r.dev) (void)hipFree(r.dev);
            if (r.done) (void)hipEventDestroy(r.done);
        }
        if (d_keys) (void)hipFree(d_keys);
        if (d_store) (void)hipFree(d_store);
    }

    int init(gc_ctx *c, uint32_t sessions, const void *keys, size_t kl) {
        if (!c || sessions == 0 || sessions > 65535u || !keys) return GC_E_ARG;  // (a session is a grid row of the serialiser)
        if (kl != 16 && kl != 24 && kl != 32) return GC_E_KEYSIZE;
        ctx = c, S = sessions, bstride = (sessions + 63u) & ~63u, keylen = kl;
        GC_HIP(hipSetDevice(ctx->device));
        GC_HIP(hipMalloc((void **)&d_keys, (size_t)S * keylen));
        GC_HIP(hipMemcpyAsync(d_keys, keys, (size_t)S * keylen, hipMemcpyDeviceToDevice, ctx->stream));
        return GC_OK;
    }

    // the store holds wire ids [0, max_id]; new rows are zero
    int ensure(uint32_t max_id) {
        if (max_id < rows) return GC_OK;
        const uint64_t want = std::min<uint64_t>(std::max<uint64_t>({(uint64_t)max_id + 1, 2ull * rows, 1024}), gcs::stream_max_wires());
        uint4 *nw = nullptr;
        GC_HIP(hipMalloc((void **)&nw, (size_t)want * bstride * sizeof(uint4)));
        hipError_t e = hipMemsetAsync(nw + (size_t)rows * bstride, 0, (size_t)(want - rows) * bstride * sizeof(uint4), ctx->stream);
        if (e == hipSuccess && rows)
            e = hipMemcpyAsync(nw, d_store, (size_t)rows * bstride * sizeof(uint4), hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            (void)hipFree(nw);
            GC_HIP(e);
        }
        if (d_store) (void)hipFree(d_store);
        d_store = nw, rows = (uint32_t)want;
        return GC_OK;
    }

    // the circuit + batch of S instances for this gate list; a batch outside the keyed scope is refused (and not kept)
    int find_or_load(const gc_gate *gates, uint32_t ngates, uint32_t nwires, uint32_t nin, uint32_t nout, const char *what,
                     SbCirc **out) {
        const uint64_t h = content_hash(gates, ngates, nwires, nin, nout);
        for (auto &e : cache) {
            if (e->hash != h || e->gates.size() != ngates || e->nwires != nwires || e->nin != nin || e->nout != nout) continue;
            bool same = true;
            for (uint32_t i = 0; i < ngates && same; i++)
                same = e->gates[i].in0 == gates[i].in0 && e->gates[i].in1 == gates[i].in1 && e->gates[i].out == gates[i].out &&
                       e->gates[i].op == gates[i].op;
            if (!same) continue;
            e->last_use = ++tick;
            *out = e.get();
            return GC_OK;
        }
        std::unique_ptr<SbCirc> e(new SbCirc);
        e->gates.assign(ngates, gc_gate{});
        for (uint32_t i = 0; i < ngates; i++)
            e->gates[i].in0 = gates[i].in0, e->gates[i].in1 = gates[i].in1, e->gates[i].out = gates[i].out, e->gates[i].op = gates[i].op;
        e->nwires = nwires, e->nin = nin, e->nout = nout, e->hash = h;
        int st = GC_OK;
        e->circ = gc_circ_load(ctx, e->gates.data(), ngates, nwires, nin, nout, &st);
        if (!e->circ) return st;
        e->batch = gc_batch_create(e->circ, S, &st);
        // (path 1 with the wires in LDS, path 2 with the wires in HBM; a batch whose wires are in LDS and whose key table does not
        // fit is sent to path 2 when the handle's fallback is on — its arrays hold every wire slot whatever the kernel, so the
        // movers around the pass read the slots they read on path 1 — and refused otherwise)
        if (e->batch && gc_batch_keyed_path(e->batch) == 0) {
            if (fallback && gc::keyed_refused_for_key_table_only(e->batch))
                st = gc_batch_set_keyed_path(e->batch, 2);
            else
                st = refuse(what, "the step's circuit is outside gc_batch_keyed_supported at this number of sessions (its wires are in "
                                  "LDS and the tile's key table does not fit)");
        }
        if (!e->batch || st != GC_OK) {
            if (e->batch) gc_batch_free(e->batch);
            gc_circ_free(e->circ);
            return st;
        }
        const gc_plan_info &pi = e->circ->plan.p.info;
        const size_t bs = gc_batch_stride(e->batch);
        e->dev_bytes = ((size_t)pi.nslots + std::max<uint32_t>(pi.slab_rows, 1) + 1) * bs * sizeof(uint4) + (size_t)S * 240;
        // bounded in device bytes, least recently used first (gc_batch_free waits for the ctx stream: nothing uses them then)
        while (!cache.empty() && cache_bytes + e->dev_bytes > cache_budget()) {
            size_t lru = 0;
            for (size_t i = 1; i < cache.size(); i++)
                if (cache[i]->last_use < cache[lru]->last_use) lru = i;
            gc_batch_free(cache[lru]->batch);
            gc_circ_free(cache[lru]->circ);
            cache_bytes -= cache[lru]->dev_bytes;
            cache.erase(cache.begin() + (long)lru);
            n_evictions++;
        }
        cache_bytes += e->dev_bytes;
        n_loads++;
        e->last_use = ++tick;
        *out = e.get();
        cache.push_back(std::move(e));
        return GC_OK;
    }

    int stage(size_t need, SbStage **out) {
        SbStage &r = ring[next++ % kRing];
        if (!r.done) GC_HIP(hipEventCreateWithFlags(&r.done, hipEventDisableTiming));
        if (r.used) GC_HIP(hipEventSynchronize(r.done));
        r.used = false;
        if (r.cap < need) {
            if (r.pin) (void)hipHostFree(r.pin);
            if (r.dev) (void)hipFree(r.dev);
            r.pin = r.dev = nullptr, r.cap = 0;
            const size_t cap = std::max<size_t>(need + need / 2, (size_t)1 << 16);
            GC_HIP(hipHostMalloc((void **)&r.pin, cap, hipHostMallocDefault));
            GC_HIP(hipMalloc((void **)&r.dev, cap));
            r.cap = cap;
        }
        *out = &r;
        return GC_OK;
    }
};

// One step's constants as one blob: in ids | out ids | row offsets | first row per piece | skeleton (zero-padded)
struct StepBlob {
    size_t o_in = 0, o_out = 0, o_row = 0, o_piece = 0, o_skel = 0, total = 0;
    uint32_t npieces = 0;
    void plan(uint32_t nin, uint32_t nout, size_t nrows, size_t nbytes) {
        npieces = (uint32_t)((nbytes + gcsb::kPieceBytes - 1) / gcsb::kPieceBytes);
        o_in = 0;
        o_out = up16(o_in + 4 * (size_t)nin);
        o_row = up16(o_out + 4 * (size_t)nout);
        o_piece = up16(o_row + 4 * nrows);
        o_skel = up16(o_piece + 4 * (size_t)npieces);
        total = o_skel + up16(nbytes) + 16;
    }
};

// lays the blob out (b), fills the stage, sends it, and describes it to the kernels
int send_step(SbCore &c, StepBlob &b, const uint32_t *in, uint32_t nin, const uint32_t *out, uint32_t nout,
              const std::vector<uint32_t> &row_off, const uint8_t *skel, size_t nbytes, SbStage **stp, gcsb::StepDev *dev) {
    b.plan(nin, nout, row_off.size(), nbytes);
    SbStage *st = nullptr;
    int rc = c.stage(b.total, &st);
    if (rc != GC_OK) return rc;
    std::memset(st->pin, 0, b.total);
    if (nin) std::memcpy(st->pin + b.o_in, in, 4 * (size_t)nin);
    if (nout) std::memcpy(st->pin + b.o_out, out, 4 * (size_t)nout);
    if (!row_off.empty()) std::memcpy(st->pin + b.o_row, row_off.data(), 4 * row_off.size());
    uint32_t *piece = (uint32_t *)(st->pin + b.o_piece);
    size_t r = 0;
    for (uint32_t p = 0; p < b.npieces; p++) {
        while (r < row_off.size() && (size_t)row_off[r] + 16 <= (size_t)p * gcsb::kPieceBytes) r++;
        piece[p] = (uint32_t)r;
    }
    if (nbytes) std::memcpy(st->pin + b.o_skel, skel, nbytes);
    GC_HIP(hipMemcpyAsync(st->dev, st->pin, b.total, hipMemcpyHostToDevice, c.ctx->stream));
    st->used = true;  // (from here on the event must be recorded before the stage is reused: step_sent)
    dev->skel = st->dev + b.o_skel;
    dev->row_off = (const uint32_t *)(st->dev + b.o_row);
    dev->piece_row = (const uint32_t *)(st->dev + b.o_piece);
    dev->nbytes = (uint32_t)nbytes, dev->nrows = (uint32_t)row_off.size(), dev->npieces = b.npieces, dev->pad_ = 0;
    *stp = st;
    return GC_OK;
}
int step_sent(SbCore &c, SbStage *st) {
    GC_HIP(hipEventRecord(st->done, c.ctx->stream));
    return GC_OK;
}
// behind the one launch of a call that sent only ids (io_ids): the launch's error, and the stage's event whatever it was
int ids_launched(SbCore &c, SbStage *st) {
    const hipError_t e = hipGetLastError();
    const int rc = step_sent(c, st);
    GC_HIP(e);
    return rc;
}

// out[] with all but the LAST of equal ids marked "not stored" (Set in order: the last one wins)
void last_wins(const uint32_t *ids, uint32_t n, std::vector<uint32_t> *marked) {
    marked->assign(ids, ids + n);
    std::unordered_map<uint32_t, uint32_t> seen;
    for (uint32_t j = n; j-- > 0;)
        if (!seen.emplace(ids[j], j).second) (*marked)[j] = kNone;
}

}  // namespace

struct gc_stream_batch : SbCore {
    uint4 *d_R = nullptr;    // [bstride]
    uint4 *d_rnd = nullptr;  // a step's inputs in the d_rnd form of gc_batch_garble_keyed, [S][1 + nin]
    size_t rnd_cap = 0;
    std::vector<gc_gate> rewritten;
    std::vector<uint8_t> skel;
    std::vector<uint32_t> row_off, out_marked;
    ~gc_stream_batch() {
        if (ctx) {
            (void)hipSetDevice(ctx->device);
            (void)hipStreamSynchronize(ctx->stream);
        }
        if (d_R) (void)hipFree(d_R);
        if (d_rnd) (void)hipFree(d_rnd);
    }
};

struct gc_stream_eval_batch : SbCore {
    std::vector<gc_gate> gates;
    std::vector<uint8_t> skel;
    std::vector<uint32_t> row_off, out_ids;
    gcw::WireStamps stamps;  // who wrote a (tmp / global) wire last
    gcw::BlockIo io;         // the block's inputs (io.inputs: the in[] of its step) and global writers
    // ---- gc_stream_eval_batch_circuit_host: blocks from host memory (all lazily made)
    struct BlockBuf {  // one device block buffer [S][pitch] and the pinned staging for pageable callers
        uint8_t *dev = nullptr, *pin = nullptr;
        size_t dev_cap = 0, pin_cap = 0;
        hipEvent_t uploaded = nullptr, consumed = nullptr;  // on the upload stream / on the ctx stream
        bool in_flight = false, in_use = false;             // `uploaded` / `consumed` has been recorded
    };
    static constexpr int kBlockBufs = 2;  // block k + 1 uploads while block k evaluates
    BlockBuf blk[kBlockBufs];
    hipStream_t up = nullptr;
    uint32_t nblk = 0;
    uint32_t *d_badsum = nullptr;  // [S]: differing structure bytes since create
    ~gc_stream_eval_batch() {
        if (ctx) {
            (void)hipSetDevice(ctx->device);
            if (up) (void)hipStreamSynchronize(up);
            (void)hipStreamSynchronize(ctx->stream);
        }
        for (auto &b : blk) {
            if (b.dev) (void)hipFree(b.dev);
            if (b.pin) (void)hipHostFree(b.pin);
            if (b.uploaded) (void)hipEventDestroy(b.uploaded);
            if (b.consumed) (void)hipEventDestroy(b.consumed);
        }
        if (up) (void)hipStreamDestroy(up);
        if (d_badsum) (void)hipFree(d_badsum);
    }
};

namespace {

// in[] / out[] naming the same GLOBAL wire (an in-place update), or out[] naming one twice: the reference resolves
// stream.wire(index) per gate (stream_garble.go:131-157), so a gate that reads such a wire — through its input-mapped or
// through any of its output-mapped circuit wires — after a gate Set it sees the label of the LATEST Set, and the store keeps
// what the last GATE Set, whatever its index in out[].  The pass garbles from a snapshot of the inputs: such reads are
// redirected to the circuit wire of the latest Set (an output-mapped wire read before any Set: to the input-mapped wire of
// the same id, if there is one) — the same global id and flags on the wire, so the bytes do not change (stream_garble.cpp:
// rewrite_aliased, restated for a handle without that stream's state).  Returns whether anything may have been rewritten
// (*gates then points at s->rewritten); *latest: global id -> the circuit wire a gate Set it through last.
bool rewrite_aliased(gc_stream_batch *s, const gc_gate **gates, uint32_t ngates, uint32_t nwires, const uint32_t *in, uint32_t nin,
                     const uint32_t *out, uint32_t nout, std::unordered_map<uint32_t, uint32_t> *latest) {
    const uint32_t first_out = nwires - nout;
    latest->clear();
    std::unordered_map<uint32_t, uint32_t> out_ids, in_i;
    bool aliased = false;
    for (uint32_t j = 0; j < nout; j++) aliased |= !out_ids.emplace(out[j], j).second;  // twice in out[]
    for (uint32_t i = 0; i < nin && !aliased; i++) aliased = out_ids.count(in[i]) != 0;
    if (!aliased) return false;
    for (uint32_t i = 0; i < nin; i++) in_i.emplace(in[i], i);
    s->rewritten.assign(*gates, *gates + ngates);
    for (uint32_t g = 0; g < ngates; g++) {
        gc_gate &q = s->rewritten[g];
        auto redirect = [&](uint32_t w) {
            if (w >= nin && w < first_out) return w;
            const uint32_t id = w < nin ? in[w] : out[w - first_out];
            auto it = latest->find(id);
            if (it != latest->end()) return it->second;
            if (w >= first_out) {
                auto ii = in_i.find(id);
                if (ii != in_i.end()) return ii->second;
            }
            return w;
        };
        q.in0 = redirect(q.in0);
        if (q.op != GC_INV) q.in1 = redirect(q.in1);
        if (q.out >= first_out) (*latest)[out[q.out - first_out]] = q.out;
    }
    *gates = s->rewritten.data();
    return true;
}

// where a step's bytes go once their number is known: the caller's place, or a window of a gc_stream_batch_out.  Called
// when nothing can refuse the step any more and before anything of it is queued.
using Placer = std::function<int(size_t nbytes, void **d_out, size_t *stride)>;
// ... or the windows of a split handle: `plan` is called where a Placer is, and says in how many segments the bytes leave;
// segment j is bytes [*b0, *b1) of the step, session s's at *d_out + s * *stride; `launched` runs right behind its launch
struct SplitPlacer {
    std::function<int(size_t nbytes, uint32_t *nseg)> plan;
    std::function<void(uint32_t j, size_t *b0, size_t *b1, void **d_out, size_t *stride)> segment;
    std::function<int(uint32_t j)> launched;
};

// prefix: bytes in front of every session's step (they join the skeleton: the same for all sessions)
int garble_step(gc_stream_batch *s, const gc_gate *gates, uint32_t ngates, uint32_t nwires, const uint32_t *in, uint32_t nin,
                const uint32_t *out, uint32_t nout, void *d_out, size_t stride, size_t *written, const uint8_t *prefix = nullptr,
                size_t prefix_len = 0, const Placer *place = nullptr, const SplitPlacer *split = nullptr) {
    static const char *const what = "gc_stream_batch_garble";
    if (!s || !written || (ngates && !gates) || (nin && !in) || (nout && !out)) return GC_E_ARG;
    *written = 0;
    if (ngates == 0) return GC_OK;
    if (s->ctx->capturing) return GC_E_ARG;  // (the step's constants are a host copy)
    int rc = GC_OK;
    if (const char *why = step_refused(gates, ngates, nwires, nin, nout, &rc)) {
        std::snprintf(gc::tls_error, sizeof gc::tls_error, "%s: %s", what, why);
        return rc;
    }
    uint32_t mx = 0;
    for (uint32_t i = 0; i < nin; i++) mx = std::max(mx, in[i]);
    for (uint32_t i = 0; i < nout; i++) mx = std::max(mx, out[i]);
    if (mx >= gcs::stream_max_wires()) return refuse(what, "a global wire id >= GC_STREAM_MAX_WIRES");
    GC_HIP(hipSetDevice(s->ctx->device));
    // the bytes are those of the caller's gate list; the pass runs the list with in-place reads redirected
    s->skel.clear(), s->row_off.clear();
    size_t nbytes = step_skeleton(gates, ngates, nwires, in, nin, out, nout, &s->skel, &s->row_off);
    if (prefix_len) {
        s->skel.insert(s->skel.begin(), prefix, prefix + prefix_len);
        for (uint32_t &off : s->row_off) off += (uint32_t)prefix_len;
        nbytes += prefix_len;
    }
    *written = nbytes;
    if (nbytes >= 0x7fffffffu) return refuse(what, "a step of 2 GiB or more");
    if (!place && !split && (!d_out || stride % 4 != 0 || stride < nbytes))
        return refuse(what, "stride must be a multiple of 4 and >= the step's bytes");
    const gc_gate *run = gates;
    std::unordered_map<uint32_t, uint32_t> latest;
    rewrite_aliased(s, &run, ngates, nwires, in, nin, out, nout, &latest);
    SbCirc *ent = nullptr;
    rc = s->find_or_load(run, ngates, nwires, nin, nout, what, &ent);
    if (rc != GC_OK) return rc;
    // ---- nothing below refuses the step: the store may change now
    rc = s->ensure(mx);
    if (rc != GC_OK) return rc;
    const size_t rnd_need = (size_t)s->S * (1 + (size_t)nin) * sizeof(uint4);
    if (s->rnd_cap < rnd_need) {
        GC_HIP(hipStreamSynchronize(s->ctx->stream));
        if (s->d_rnd) (void)hipFree(s->d_rnd);
        s->d_rnd = nullptr, s->rnd_cap = 0;
        GC_HIP(hipMalloc((void **)&s->d_rnd, rnd_need + rnd_need / 2));
        s->rnd_cap = rnd_need + rnd_need / 2;
    }
    // equal ids in out[]: the output of the gate that Set the id last is stored (one no gate Sets: the last index)
    last_wins(out, nout, &s->out_marked);
    for (uint32_t j = 0; j < nout; j++) {
        auto it = latest.find(out[j]);
        if (it != latest.end()) s->out_marked[j] = it->second == nwires - nout + j ? out[j] : kNone;
    }
    uint32_t nseg = 0;
    if (place) rc = (*place)(nbytes, &d_out, &stride);
    if (split) rc = split->plan(nbytes, &nseg);
    if (rc != GC_OK) return rc;
    StepBlob b;
    SbStage *st = nullptr;
    gcsb::StepDev dev{};
    rc = send_step(*s, b, in, nin, s->out_marked.data(), nout, s->row_off, s->skel.data(), nbytes, &st, &dev);
    if (rc != GC_OK) return rc;
    hipStream_t q = s->ctx->stream;
    const uint32_t *d_in = (const uint32_t *)(st->dev + b.o_in), *d_outi = (const uint32_t *)(st->dev + b.o_out);
    gc_batch *bt = ent->batch;
    // 1. the step's inputs out of the store, in the d_rnd form of the keyed pass: [S][1 + nin] big-endian labels, R first
    launch_gather(s->d_store, s->store_layout(), 0, d_in, 0, nin, nullptr, 0, s->d_rnd + 1, 1 + (size_t)nin, s->S, q);
    gcsb::launch_rnd_form(s->d_rnd, s->d_R, s->S, 1 + nin, q);
    hipError_t e = hipGetLastError();
    // 2. one keyed batch pass of S instances
    if (e == hipSuccess) rc = gc_batch_garble_keyed(bt, s->d_keys, s->keylen, s->d_rnd);
    if (e == hipSuccess && rc == GC_OK) {
        // 3. the output L0s into the store through out[]; 4. every session's bytes
        gcsb::launch_rows(bt->d_W, bt->g.lw, ent->circ->d_out_slots, s->d_store, s->store_layout(), d_outi, nout, s->S, q);
        if (!split) gcsb::launch_serialise(dev, bt->d_T, bt->g.lt, (uint8_t *)d_out, stride, s->S, q);
        e = hipGetLastError();
        // a split step: the pass, the scatter and the constants above ran once; one launch per window, its seal right behind it
        for (uint32_t j = 0; j < nseg && e == hipSuccess && rc == GC_OK; j++) {
            size_t b0 = 0, b1 = 0;
            split->segment(j, &b0, &b1, &d_out, &stride);
            if (nseg == 1)  // (not cut: the whole-step kernel, as on an unsplit handle)
                gcsb::launch_serialise(dev, bt->d_T, bt->g.lt, (uint8_t *)d_out, stride, s->S, q);
            else
                gcsb::launch_serialise_range(dev, bt->d_T, bt->g.lt, (uint8_t *)d_out, stride, s->S, (uint32_t)b0, (uint32_t)b1, q);
            e = hipGetLastError();
            rc = split->launched(j);
        }
    }
    const int rce = step_sent(*s, st);
    GC_HIP(e);
    return rc != GC_OK ? rc : rce;
}

// One OpCircuit block as the peer sent it, parsed into a single-assignment gate list: gcw::walk_block (stream_wire.h — the
// gate loop and the refusals of stream_eval.cpp's evaluator) with a sink that keeps the gates and where the rows are.
// e->gates / io.inputs / out_ids: the device circuit and the global wires it reads and stores (kNone: a later gate of the
// block writes the same wire); skel = the block's bytes with its rows zeroed.
struct BatchSink {
    std::vector<gcw::ParsedGate> gates;
    std::vector<uint32_t> &row_off;
    uint32_t global_field(size_t, bool) { return 0; }
    void gate(uint32_t g, uint32_t in0, uint32_t in1, uint32_t op, bool writes_tmp) { gates[g] = gcw::ParsedGate{in0, in1, op, writes_tmp}; }
    void rows(size_t at, uint32_t n) {
        for (uint32_t r = 0; r < n; r++) row_off.push_back((uint32_t)(at + 16u * r));
    }
};
int parse_block(gc_stream_eval_batch *e, uint32_t ngates, uint32_t ntmp, uint32_t nwires, const uint8_t *buf, size_t len, size_t *used) {
    e->row_off.clear();
    BatchSink sink{std::vector<gcw::ParsedGate>(ngates), e->row_off};
    size_t pos = 0;
    const int rc = gcw::walk_block(buf, len, ngates, ntmp, nwires, e->stamps, e->io, sink, &pos);
    if (rc != GC_OK) return rc;
    const uint32_t nout = (uint32_t)e->io.writers.size();
    std::vector<uint32_t> id_of;
    gcw::ssa_gate_list(sink.gates, (uint32_t)e->io.inputs.size(), nout, [](const gcw::ParsedGate &g) { return g.writes_tmp; }, &id_of, &e->gates);
    std::vector<uint8_t> live;
    gcw::live_outputs(e->stamps, e->io, &live);
    e->out_ids.resize(nout);
    for (uint32_t k = 0; k < nout; k++) e->out_ids[k] = live[k] ? (uint32_t)e->io.writers[k] : kNone;
    e->skel.assign(buf, buf + pos);
    for (uint32_t off : e->row_off) std::memset(e->skel.data() + off, 0, 16);
    *used = pos;
    return GC_OK;
}

// the blocks of a step whose reference block has been accepted, in device memory: the caller's, or an upload of the handle's
using Supplier = std::function<int(size_t nbytes, const void **d_blocks, size_t *stride)>;

// supply: d_bad is the handle's running sum (not zeroed) and the blocks come from *supply
int eval_step(gc_stream_eval_batch *e, uint32_t ngates, uint32_t ntmp, uint32_t nwires, const uint8_t *ref, size_t len,
              const void *d_blocks, size_t stride, void *d_bad, size_t *consumed, const Supplier *supply = nullptr) {
    static const char *const what = "gc_stream_eval_batch_circuit";
    if (!e || !consumed || (!ref && len) || !d_bad) return GC_E_ARG;
    *consumed = 0;
    // the block is the peer's data: the same bounds as gc_stream_eval_circuit, before anything is sized by it
    if ((uint64_t)ntmp > 64ull * ngates + (1u << 20) || nwires > gcs::stream_max_wires()) return GC_E_ARG;
    if ((size_t)ngates > len / 5) return GC_E_ROWS;
    if (e->ctx->capturing) return GC_E_ARG;
    GC_HIP(hipSetDevice(e->ctx->device));
    hipStream_t q = e->ctx->stream;
    if (!supply) GC_HIP(hipMemsetAsync(d_bad, 0, (size_t)e->S * sizeof(uint32_t), q));
    if (ngates == 0) return GC_OK;
    size_t pos = 0;
    int rc = parse_block(e, ngates, ntmp, nwires, ref, len, &pos);
    if (rc != GC_OK) return rc;
    if (pos >= 0x7fffffffu) return refuse(what, "a block of 2 GiB or more");
    if (!supply && (!d_blocks || stride % 4 != 0 || stride < len)) return refuse(what, "stride must be a multiple of 4 and >= len");
    const uint32_t nin = (uint32_t)e->io.inputs.size(), nout = (uint32_t)e->out_ids.size();
    SbCirc *ent = nullptr;
    rc = e->find_or_load(e->gates.data(), ngates, nin + ngates, nin, nout, what, &ent);
    if (rc != GC_OK) return rc;
    uint32_t mx = 0;
    for (uint32_t id : e->io.inputs) mx = std::max(mx, id);
    for (uint32_t id : e->out_ids) mx = std::max(mx, id == kNone ? 0u : id);
    rc = e->ensure(mx);
    if (rc != GC_OK) return rc;
    if (supply) {
        rc = (*supply)(pos, &d_blocks, &stride);
        if (rc != GC_OK) return rc;
    }
    StepBlob b;
    SbStage *st = nullptr;
    gcsb::StepDev dev{};
    rc = send_step(*e, b, e->io.inputs.data(), nin, e->out_ids.data(), nout, e->row_off, e->skel.data(), pos, &st, &dev);
    if (rc != GC_OK) return rc;
    const uint32_t *d_in = (const uint32_t *)(st->dev + b.o_in), *d_outi = (const uint32_t *)(st->dev + b.o_out);
    gc_batch *bt = ent->batch;
    // 1. + 2. skeleton compare and the rows into the batch's table array; 3. the inputs out of the store
    gcsb::launch_ingest(dev, bt->d_T, bt->g.lt, (const uint8_t *)d_blocks, stride, e->S, (uint32_t *)d_bad, q);
    gcsb::launch_rows(e->d_store, e->store_layout(), d_in, bt->d_W, bt->g.lw, nullptr, nin, e->S, q);
    hipError_t err = hipGetLastError();
    // 4. one keyed batch pass; 5. the outputs into the store
    if (err == hipSuccess) rc = gc_batch_eval_keyed(bt, e->d_keys, e->keylen, bt);
    if (err == hipSuccess && rc == GC_OK) {
        gcsb::launch_rows(bt->d_W, bt->g.lw, ent->circ->d_out_slots, e->d_store, e->store_layout(), d_outi, nout, e->S, q);
        err = hipGetLastError();
    }
    const int rce = step_sent(*e, st);
    GC_HIP(err);
    if (rc == GC_OK && rce == GC_OK) *consumed = pos;
    return rc != GC_OK ? rc : rce;
}

int cache_stats(const SbCore *c, uint64_t *entries, uint64_t *bytes, uint64_t *loads, uint64_t *evictions) {
    if (!c) return GC_E_ARG;
    if (entries) *entries = c->cache.size();
    if (bytes) *bytes = c->cache_bytes;
    if (loads) *loads = c->n_loads;
    if (evictions) *evictions = c->n_evictions;
    return GC_OK;
}

// ids[] on the device for the length of one call (a host copy: the call waits for it)
int ids_to_device(SbCore &c, const uint32_t *ids, uint32_t n, DevBuf *d) {
    GC_HIP(d->alloc(4 * (size_t)n));
    GC_HIP(hipMemcpyAsync(d->p, ids, 4 * (size_t)n, hipMemcpyHostToDevice, c.ctx->stream));
    return GC_OK;
}

// one column of the store: wire w of every session (zero if the store never grew that far)
int read_column(SbCore &c, uint32_t w, std::vector<gc_label> *col) {
    col->assign(c.S, gc_label{0, 0});
    GC_HIP(hipSetDevice(c.ctx->device));
    if (w < c.rows)
        GC_HIP(hipMemcpyAsync(col->data(), c.d_store + (size_t)w * c.bstride, (size_t)c.S * sizeof(gc_label), hipMemcpyDeviceToHost,
                              c.ctx->stream));
    GC_HIP(hipStreamSynchronize(c.ctx->stream));
    return GC_OK;
}

// the ids of a select / decode / gather / set call: checked, the store grown to hold them (a wire never set reads as 0: its
// labels are 0 and R), and sent through the staging ring — `send` in their place, if given (set: all but the last of equal ids)
// nsend: `send` is a list of its own length (n == 0: no wire ids, a list of offsets — gc_stream_eval_batch_in_feed)
int io_ids(SbCore &c, const char *what, bool refuse_capture, const uint32_t *ids, uint32_t n, SbStage **st, const uint32_t **d_ids,
           const uint32_t *send = nullptr, uint32_t nsend = 0) {
    if (refuse_capture && c.ctx->capturing) return GC_E_ARG;
    uint32_t mx = 0;
    for (uint32_t i = 0; i < n; i++) mx = std::max(mx, ids[i]);
    if (mx >= gcs::stream_max_wires()) return refuse(what, "a wire id >= GC_STREAM_MAX_WIRES");
    GC_HIP(hipSetDevice(c.ctx->device));
    int rc = c.ensure(mx);
    if (rc != GC_OK) return rc;
    StepBlob b;
    gcsb::StepDev dev{};
    rc = send_step(c, b, send ? send : ids, nsend ? nsend : n, nullptr, 0, {}, nullptr, 0, st, &dev);
    if (rc == GC_OK) *d_ids = (const uint32_t *)((*st)->dev + b.o_in);
    return rc;
}

}  // namespace

extern "C" {

gc_stream_batch *gc_stream_batch_create(gc_ctx *ctx, uint32_t sessions, const void *d_keys, size_t keylen, const void *d_rnd,
                                        const uint32_t *inputs, uint32_t ninputs, int *status) try {
    int rc = GC_OK;
    std::unique_ptr<gc_stream_batch> s(new (std::nothrow) gc_stream_batch);
    if (!s) rc = GC_E_NOMEM;
    if (rc == GC_OK && (!d_rnd || (ninputs && !inputs))) rc = GC_E_ARG;
    if (rc == GC_OK) rc = s->init(ctx, sessions, d_keys, keylen);
    uint32_t mx = 0;
    for (uint32_t i = 0; rc == GC_OK && i < ninputs; i++) mx = std::max(mx, inputs[i]);
    if (rc == GC_OK && mx >= gcs::stream_max_wires()) rc = refuse("gc_stream_batch_create", "an input wire id >= GC_STREAM_MAX_WIRES");
    auto setup = [&]() -> int {
        GC_HIP(hipMalloc((void **)&s->d_R, (size_t)s->bstride * sizeof(uint4)));
        GC_HIP(hipMemsetAsync(s->d_R, 0, (size_t)s->bstride * sizeof(uint4), ctx->stream));
        int r = s->ensure(mx);
        if (r != GC_OK) return r;
        std::vector<uint32_t> ids;
        last_wins(inputs, ninputs, &ids);  // (NewStreaming Sets the inputs in order, stream_garble.go:62-72)
        DevBuf d;
        r = ids_to_device(*s, ids.data(), ninputs, &d);
        if (r != GC_OK) return r;
        gcsb::launch_init_store((const uint4 *)d_rnd, (const uint32_t *)d.p, ninputs, s->d_store, s->bstride, s->d_R, s->S, ctx->stream);
        GC_HIP(hipGetLastError());
        GC_HIP(hipStreamSynchronize(ctx->stream));
        return GC_OK;
    };
    if (rc == GC_OK) rc = setup();
    if (status) *status = rc;
    return rc == GC_OK ? s.release() : nullptr;
} catch (...) {
    const int rc__ = gc::on_exception();
    if (status) *status = rc__;
    return nullptr;
}

void gc_stream_batch_free(gc_stream_batch *s) { delete s; }

size_t gc_stream_batch_step_bytes(const gc_gate *gates, uint32_t ngates, uint32_t nwires, const uint32_t *in, uint32_t nin,
                                  const uint32_t *out, uint32_t nout) try {
    if ((ngates && !gates) || (nin && !in) || (nout && !out)) return 0;
    int rc = GC_OK;
    if (const char *why = step_refused(gates, ngates, nwires, nin, nout, &rc)) {
        std::snprintf(gc::tls_error, sizeof gc::tls_error, "gc_stream_batch_step_bytes: %s", why);
        return 0;
    }
    return step_skeleton(gates, ngates, nwires, in, nin, out, nout, nullptr, nullptr);
} catch (...) {
    (void)gc::on_exception();
    return 0;
}

int gc_stream_batch_garble(gc_stream_batch *s, const gc_gate *gates, uint32_t ngates, uint32_t nwires, const uint32_t *in,
                           uint32_t nin, const uint32_t *out, uint32_t nout, void *d_out, size_t stride, size_t *written) try {
    return garble_step(s, gates, ngates, nwires, in, nin, out, nout, d_out, stride, written);
} catch (...) {
    return gc::on_exception();
}

int gc_stream_batch_get_wire(gc_stream_batch *s, uint32_t w, gc_wire *out) try {
    if (!s || !out) return GC_E_ARG;
    std::vector<gc_label> l0, r(s->S);
    int rc = read_column(*s, w, &l0);
    if (rc != GC_OK) return rc;
    GC_HIP(hipMemcpy(r.data(), s->d_R, (size_t)s->S * sizeof(gc_label), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < s->S; i++) out[i] = gc_wire{l0[i], gc_label{l0[i].d0 ^ r[i].d0, l0[i].d1 ^ r[i].d1}};
    return GC_OK;
} catch (...) {
    return gc::on_exception();
}

int gc_stream_batch_gather_wires(gc_stream_batch *s, const uint32_t *ids, uint32_t n, void *d_wires_out) try {
    if (!s || (n && (!ids || !d_wires_out))) return GC_E_ARG;
    if (n == 0) return GC_OK;
    SbStage *st = nullptr;
    const uint32_t *d_ids = nullptr;
    int rc = io_ids(*s, "gc_stream_batch_gather_wires", false, ids, n, &st, &d_ids);  // (a wire never set reads as (0, R))
    if (rc != GC_OK) return rc;
    launch_gather(s->d_store, s->store_layout(), 0, d_ids, 0, n, s->d_R, 1, (uint4 *)d_wires_out,
                  2 * (size_t)n, s->S, s->ctx->stream);
    return ids_launched(*s, st);
} catch (...) {
    return gc::on_exception();
}

int gc_stream_batch_cache_stats(const gc_stream_batch *s, uint64_t *entries, uint64_t *bytes, uint64_t *loads, uint64_t *evictions) {
    return cache_stats(s, entries, bytes, loads, evictions);
}

gc_stream_eval_batch *gc_stream_eval_batch_create(gc_ctx *ctx, uint32_t sessions, const void *d_keys, size_t keylen, int *status) try {
    int rc = GC_OK;
    std::unique_ptr<gc_stream_eval_batch> e(new (std::nothrow) gc_stream_eval_batch);
    if (!e) rc = GC_E_NOMEM;
    if (rc == GC_OK) rc = e->init(ctx, sessions, d_keys, keylen);
    if (rc == GC_OK) rc = e->ensure(0);
    if (status) *status = rc;
    return rc == GC_OK ? e.release() : nullptr;
} catch (...) {
    const int rc__ = gc::on_exception();
    if (status) *status = rc__;
    return nullptr;
}

void gc_stream_eval_batch_free(gc_stream_eval_batch *e) { delete e; }

int gc_stream_eval_batch_set_wires(gc_stream_eval_batch *e, const uint32_t *ids, uint32_t n, const void *d_labels) try {
    if (!e || (n && (!ids || !d_labels))) return GC_E_ARG;
    if (n == 0) return GC_OK;
    std::vector<uint32_t> marked;
    last_wins(ids, n, &marked);
    SbStage *st = nullptr;
    const uint32_t *d_ids = nullptr;
    int rc = io_ids(*e, "gc_stream_eval_batch_set_wires", false, ids, n, &st, &d_ids, marked.data());
    if (rc != GC_OK) return rc;
    launch_scatter((const uint4 *)d_labels, n, n, d_ids, 0, e->d_store, e->store_layout(), 0, e->S,
                   e->ctx->stream);
    return ids_launched(*e, st);
} catch (...) {
    return gc::on_exception();
}

int gc_stream_eval_batch_get_wire(gc_stream_eval_batch *e, uint32_t w, gc_label *out) try {
    if (!e || !out) return GC_E_ARG;
    std::vector<gc_label> col;
    int rc = read_column(*e, w, &col);
    if (rc == GC_OK) std::memcpy(out, col.data(), (size_t)e->S * sizeof(gc_label));
    return rc;
} catch (...) {
    return gc::on_exception();
}

int gc_stream_eval_batch_cache_stats(const gc_stream_eval_batch *e, uint64_t *entries, uint64_t *bytes, uint64_t *loads,
                                     uint64_t *evictions) {
    return cache_stats(e, entries, bytes, loads, evictions);
}

int gc_stream_eval_batch_circuit(gc_stream_eval_batch *e, uint32_t ngates, uint32_t ntmp, uint32_t nwires, const uint8_t *ref_block,
                                 size_t len, const void *d_blocks, size_t stride, void *d_bad, size_t *consumed) try {
    return eval_step(e, ngates, ntmp, nwires, ref_block, len, d_blocks, stride, d_bad, consumed);
} catch (...) {
    return gc::on_exception();
}

}  // extern "C"

// ================================================================================================================================
// Inputs, results and the host-memory paths of the two handles: the garbler's own input labels and the
// decoded result on the device, windows of stream bytes in pinned host memory, and the evaluator's blocks from host memory.
// ================================================================================================================================

// One window: a device array [S][cap] the steps write into and a pinned host array of the same shape.  The ring state (which
// window fills, seals, is handed out) is gcsb::WindowRing; this handle adds the memory, the events and the copy stream.
struct gc_stream_batch_out {
    struct Win {
        uint8_t *dev = nullptr, *pin = nullptr;
        hipEvent_t sealed = nullptr, copied = nullptr;  // on the ctx stream / on the copy stream
    };
    gc_stream_batch *sb = nullptr;
    mutable std::mutex mu;  // the ring and the windows' pointers; never held across a wait for a copy
    gcsb::WindowRing ring;
    std::vector<Win> win;
    hipStream_t copy = nullptr;
    bool whole_rows = false;  // copy [S][cap] in one piece instead of the used columns (GC_STREAM_BATCH_OUT_WHOLE_ROWS)
    bool split = false;       // gc_stream_batch_out_create_split: a step is cut over the windows, none grows (fixed at creation)
    uint64_t split_steps = 0, segments = 0;  // steps that touched more than one window / serialiser launches

    static void drop(Win &w) {
        if (w.dev) (void)hipFree(w.dev);
        if (w.pin) (void)hipHostFree(w.pin);
        w.dev = w.pin = nullptr;
    }
    // both arrays or neither; the device array starts as zeros (a whole-row copy moves bytes no step wrote)
    int make(size_t cap, Win *w) const {
        const size_t bytes = (size_t)sb->S * cap;
        hipError_t e = hipMalloc((void **)&w->dev, bytes);
        if (e == hipSuccess) e = hipHostMalloc((void **)&w->pin, bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMemsetAsync(w->dev, 0, bytes, sb->ctx->stream);
        if (e != hipSuccess) {
            drop(*w);
            GC_HIP(e);
        }
        return GC_OK;
    }
    // the window's first n columns are complete in program order of the ctx stream: queue their way to the host
    int seal(uint32_t k, size_t n) {
        Win &w = win[k];
        const size_t cap = ring.cap[k];
        GC_HIP(hipEventRecord(w.sealed, sb->ctx->stream));
        GC_HIP(hipStreamWaitEvent(copy, w.sealed, 0));
        if (whole_rows || n == cap)
            GC_HIP(hipMemcpyAsync(w.pin, w.dev, (size_t)sb->S * cap, hipMemcpyDeviceToHost, copy));
        else
            GC_HIP(hipMemcpy2DAsync(w.pin, cap, w.dev, cap, n, sb->S, hipMemcpyDeviceToHost, copy));
        GC_HIP(hipEventRecord(w.copied, copy));
        return GC_OK;
    }
    ~gc_stream_batch_out() {
        if (sb) {
            (void)hipSetDevice(sb->ctx->device);
            if (copy) (void)hipStreamSynchronize(copy);
            (void)hipStreamSynchronize(sb->ctx->stream);
        }
        for (auto &w : win) {
            drop(w);
            if (w.sealed) (void)hipEventDestroy(w.sealed);
            if (w.copied) (void)hipEventDestroy(w.copied);
        }
        if (copy) (void)hipStreamDestroy(copy);
    }
};

// The intake of S byte streams.  What is held and where the next message starts is gcsb::Intake; this handle
// adds two device buffers [S][pitch] that read [the kept tail | the fed chunk], the pinned staging of pageable callers, the
// reference session's copy of the tail on the host, and the events between the handle's upload stream and the ctx stream.
struct gc_stream_eval_batch_in {
    struct Buf {
        uint8_t *dev = nullptr, *pin = nullptr;
        size_t pitch = 0, dev_cap = 0, pin_cap = 0;
        hipEvent_t uploaded = nullptr, consumed = nullptr;  // on the upload stream / on the ctx stream
        bool in_flight = false, in_use = false;             // `uploaded` / `consumed` has been recorded
    };
    gc_stream_eval_batch *e = nullptr;
    uint32_t ref = 0;
    gcsb::Intake st;
    Buf buf[2];
    uint32_t cur = 0;              // the buffer whose front holds the tail
    size_t tail_at = 0;            // ... at this column
    std::vector<uint8_t> ref_buf;  // the reference session's [tail | chunk] while a tail is held
    std::vector<uint32_t> msg_off;
    ~gc_stream_eval_batch_in() {
        if (e) {
            (void)hipSetDevice(e->ctx->device);
            if (e->up) (void)hipStreamSynchronize(e->up);
            (void)hipStreamSynchronize(e->ctx->stream);
        }
        for (auto &b : buf) {
            if (b.dev) (void)hipFree(b.dev);
            if (b.pin) (void)hipHostFree(b.pin);
            if (b.uploaded) (void)hipEventDestroy(b.uploaded);
            if (b.consumed) (void)hipEventDestroy(b.consumed);
        }
    }
};

namespace {

int select_dev(gc_stream_batch *s, const uint32_t *ids, uint32_t n, const void *d_bits, void *d_labels_out) {
    if (!s || (n && (!ids || !d_bits || !d_labels_out))) return GC_E_ARG;
    if (n == 0) return GC_OK;
    SbStage *st = nullptr;
    const uint32_t *d_ids = nullptr;
    int rc = io_ids(*s, "gc_stream_batch_select_labels_dev", true, ids, n, &st, &d_ids);
    if (rc != GC_OK) return rc;
    gcsb::launch_select(s->d_store, s->bstride, d_ids, n, s->d_R, (const uint8_t *)d_bits, (uint4 *)d_labels_out, s->S, s->ctx->stream);
    return ids_launched(*s, st);
}

int decode_dev(gc_stream_batch *s, const uint32_t *ids, uint32_t n, const void *d_labels, void *d_bits_out, void *d_bad) {
    if (!s || !d_bad || (n && (!ids || !d_labels || !d_bits_out))) return GC_E_ARG;
    if (s->ctx->capturing) return GC_E_ARG;
    GC_HIP(hipSetDevice(s->ctx->device));
    GC_HIP(hipMemsetAsync(d_bad, 0, (size_t)s->S * sizeof(uint32_t), s->ctx->stream));
    if (n == 0) return GC_OK;
    SbStage *st = nullptr;
    const uint32_t *d_ids = nullptr;
    int rc = io_ids(*s, "gc_stream_batch_decode_dev", true, ids, n, &st, &d_ids);
    if (rc != GC_OK) return rc;
    gcsb::launch_decode_labels(s->d_store, s->bstride, d_ids, n, s->d_R, (const uint4 *)d_labels, (uint8_t *)d_bits_out,
                               (uint32_t *)d_bad, s->S, s->ctx->stream);
    return ids_launched(*s, st);
}

// what a split handle answers to a step it cannot take now (busy: counted) or ever (too large: named); GC_OK: it fits
int split_answer(gc_stream_batch_out *h, const gcsb::WindowRing::Split &p, size_t n) {
    if (p.too_large) {
        std::snprintf(gc::tls_error, sizeof gc::tls_error,
                      "gc_stream_batch_out_garble: a step of %zu bytes per session can never be given room in %u windows of %zu bytes "
                      "(at most %zu: one window less than the ring)",
                      n, h->ring.count(), h->ring.cap[0], (size_t)(h->ring.count() - 1) * h->ring.cap[0]);
        return GC_E_ARG;
    }
    if (p.is_busy) {
        h->ring.note_busy();
        return GC_E_BUSY;
    }
    return GC_OK;
}

// the split form of out_garble, under the handle's lock; size: the step's bytes if its shape is not refused, else 0
int out_garble_split(gc_stream_batch_out *h, const uint8_t *prefix, size_t prefix_len, const gc_gate *gates, uint32_t ngates,
                     uint32_t nwires, const uint32_t *in, uint32_t nin, const uint32_t *out, uint32_t nout, size_t *written, size_t size) {
    gc_stream_batch *s = h->sb;
    if (size) {
        const int rc = split_answer(h, h->ring.plan_split(size), size);
        if (rc != GC_OK) return rc;
    }
    GC_HIP(hipSetDevice(s->ctx->device));
    gcsb::WindowRing::Split p;
    size_t n = 0;
    uint32_t sealed = 0;  // windows of the step whose seal has been queued
    const size_t cap = h->ring.cap[0];
    SplitPlacer sp;
    sp.plan = [&](size_t nbytes, uint32_t *nseg) -> int {
        const gcsb::WindowRing::Split q = h->ring.plan_split(nbytes);
        const int rc = split_answer(h, q, nbytes);
        if (rc != GC_OK) return rc;
        h->ring.commit_split(q, nbytes);
        h->segments += q.nwin, h->split_steps += q.nwin > 1;
        p = q, n = nbytes, *nseg = q.nwin;
        return GC_OK;
    };
    sp.segment = [&](uint32_t j, size_t *b0, size_t *b1, void **d_out, size_t *stride) {
        *b0 = p.begin(j, n, cap), *b1 = p.begin(j + 1, n, cap);
        *d_out = h->win[(p.win + j) % h->ring.count()].dev + (j ? 0 : p.at);
        *stride = cap;
    };
    sp.launched = [&](uint32_t j) -> int {
        if (j >= p.nsealed) return GC_OK;
        sealed = j + 1;
        return h->seal((p.win + j) % h->ring.count(), cap);
    };
    const int rc = garble_step(s, gates, ngates, nwires, in, nin, out, nout, nullptr, 0, written, prefix, prefix_len, nullptr, &sp);
    // (the ring has the windows as sealed whatever became of the step's launches: their events must exist)
    int rcs = GC_OK;
    for (uint32_t j = sealed; j < p.nsealed; j++) {
        const int r = h->seal((p.win + j) % h->ring.count(), cap);
        if (rcs == GC_OK) rcs = r;
    }
    return rc != GC_OK ? rc : rcs;
}

int out_garble(gc_stream_batch_out *h, const uint8_t *prefix, size_t prefix_len, const gc_gate *gates, uint32_t ngates,
               uint32_t nwires, const uint32_t *in, uint32_t nin, const uint32_t *out, uint32_t nout, size_t *written) {
    if (!h || !written || prefix_len > 64 || (prefix_len && !prefix) || (ngates && !gates) || (nin && !in) || (nout && !out))
        return GC_E_ARG;
    *written = 0;
    gc_stream_batch *s = h->sb;
    // a full ring is known from the step's size alone: answer before the step touches anything (a step that is refused by
    // its shape is left to garble_step, which says why).  The size is worked out before the lock is taken, so that a caller
    // who repeats a busy call does not keep the lock from the thread that would release a window.
    int shape = GC_OK;
    size_t size = 0;
    if (ngates && !s->ctx->capturing && !step_refused(gates, ngates, nwires, nin, nout, &shape))
        size = step_skeleton(gates, ngates, nwires, in, nin, out, nout, nullptr, nullptr) + prefix_len;
    std::lock_guard<std::mutex> lock(h->mu);
    if (h->split) return out_garble_split(h, prefix, prefix_len, gates, ngates, nwires, in, nin, out, nout, written, size);
    if (size && h->ring.plan_step(size).is_busy) {
        h->ring.note_busy();
        return GC_E_BUSY;
    }
    GC_HIP(hipSetDevice(s->ctx->device));
    uint32_t seal_after = gcsb::WindowRing::kNoWindow;
    size_t seal_len = 0;
    const Placer place = [&](size_t n, void **d_out, size_t *stride) -> int {
        const gcsb::WindowRing::Step p = h->ring.plan_step(n);
        if (p.is_busy) {
            h->ring.note_busy();
            return GC_E_BUSY;
        }
        gc_stream_batch_out::Win bigger;
        if (p.grow_to) {  // (the window is empty and free: nothing on the device or on the link uses its arrays)
            const int rc = h->make(p.grow_to, &bigger);
            if (rc != GC_OK) return rc;
        }
        if (p.seal_before != gcsb::WindowRing::kNoWindow) {
            const int rc = h->seal(p.seal_before, p.seal_len);
            if (rc != GC_OK) {
                gc_stream_batch_out::drop(bigger);
                return rc;
            }
        }
        if (p.grow_to) {
            gc_stream_batch_out::drop(h->win[p.win]);
            h->win[p.win].dev = bigger.dev, h->win[p.win].pin = bigger.pin;
        }
        h->ring.commit(p, n);
        if (p.seal_after) seal_after = p.win, seal_len = p.at + n;
        *d_out = h->win[p.win].dev + p.at;
        *stride = h->ring.cap[p.win];
        return GC_OK;
    };
    const int rc = garble_step(s, gates, ngates, nwires, in, nin, out, nout, nullptr, 0, written, prefix, prefix_len, &place);
    // (the ring has the window as sealed whatever became of the step's launches: its events must exist)
    const int rcs = seal_after != gcsb::WindowRing::kNoWindow ? h->seal(seal_after, seal_len) : GC_OK;
    return rc != GC_OK ? rc : rcs;
}

// the handle's upload stream, running sum and events, made by the first call that needs them
int eval_host_setup(gc_stream_eval_batch *e) {
    GC_HIP(hipSetDevice(e->ctx->device));
    if (!e->up) GC_HIP(hipStreamCreateWithFlags(&e->up, hipStreamNonBlocking));
    for (auto &b : e->blk) {
        if (!b.uploaded) GC_HIP(hipEventCreateWithFlags(&b.uploaded, hipEventDisableTiming));
        if (!b.consumed) GC_HIP(hipEventCreateWithFlags(&b.consumed, hipEventDisableTiming));
    }
    if (!e->d_badsum) {
        GC_HIP(hipMalloc((void **)&e->d_badsum, (size_t)e->S * sizeof(uint32_t)));
        GC_HIP(hipMemsetAsync(e->d_badsum, 0, (size_t)e->S * sizeof(uint32_t), e->ctx->stream));
    }
    return GC_OK;
}

int eval_host(gc_stream_eval_batch *e, uint32_t ngates, uint32_t ntmp, uint32_t nwires, const uint8_t *blocks, size_t stride,
              size_t len, uint32_t ref_session, size_t *consumed) {
    if (!e || !consumed || (!blocks && len) || ref_session >= e->S || (e->S > 1 && stride < len)) return GC_E_ARG;
    *consumed = 0;
    if (e->ctx->capturing) return GC_E_ARG;
    int rc = eval_host_setup(e);
    if (rc != GC_OK) return rc;
    gc_stream_eval_batch::BlockBuf *used = nullptr;
    const Supplier supply = [&](size_t nbytes, const void **d_blocks, size_t *pitch_out) -> int {
        gc_stream_eval_batch::BlockBuf &b = e->blk[e->nblk++ % gc_stream_eval_batch::kBlockBufs];
        const size_t pitch = up16(nbytes), need = (size_t)e->S * pitch;
        const bool pinned = gc_host_is_pinned(blocks) != 0;
        if (b.dev_cap < need) {  // (freed only when the block before has been ingested)
            if (b.in_flight) GC_HIP(hipEventSynchronize(b.uploaded));
            if (b.in_use) GC_HIP(hipEventSynchronize(b.consumed));
            if (b.dev) (void)hipFree(b.dev);
            b.dev = nullptr, b.dev_cap = 0;
            GC_HIP(hipMalloc((void **)&b.dev, need + need / 2));
            b.dev_cap = need + need / 2;
        } else if (b.in_use) {
            GC_HIP(hipStreamWaitEvent(e->up, b.consumed, 0));
        }
        if (pinned) {  // DMA straight from the caller's memory, row by row at the caller's stride
            // (one session: its stride is not looked at, and a source pitch below the width would be refused)
            GC_HIP(hipMemcpy2DAsync(b.dev, pitch, blocks, e->S > 1 ? stride : nbytes, nbytes, e->S, hipMemcpyHostToDevice, e->up));
        } else {
            if (b.in_flight) GC_HIP(hipEventSynchronize(b.uploaded));  // (the staging's previous block has left)
            if (b.pin_cap < need) {
                if (b.pin) (void)hipHostFree(b.pin);
                b.pin = nullptr, b.pin_cap = 0;
                GC_HIP(hipHostMalloc((void **)&b.pin, need + need / 2, hipHostMallocDefault));
                b.pin_cap = need + need / 2;
            }
            for (uint32_t s = 0; s < e->S; s++) std::memcpy(b.pin + (size_t)s * pitch, blocks + (size_t)s * stride, nbytes);
            GC_HIP(hipMemcpyAsync(b.dev, b.pin, need, hipMemcpyHostToDevice, e->up));
        }
        GC_HIP(hipEventRecord(b.uploaded, e->up));
        b.in_flight = true;
        GC_HIP(hipStreamWaitEvent(e->ctx->stream, b.uploaded, 0));
        used = &b;
        *d_blocks = b.dev, *pitch_out = pitch;
        return GC_OK;
    };
    rc = eval_step(e, ngates, ntmp, nwires, blocks ? blocks + (size_t)ref_session * stride : nullptr, len, nullptr, 0, e->d_badsum,
                   consumed, &supply);
    if (used) {  // what reads the buffer is queued (or was not: then the event completes at once)
        const hipError_t err = hipEventRecord(used->consumed, e->ctx->stream);
        used->in_use = err == hipSuccess;
        if (rc == GC_OK) GC_HIP(err);
    }
    return rc;
}

int return_dev(gc_stream_eval_batch *e, const uint32_t *ids, uint32_t n, void *d_labels_out) {
    if (!e || (n && (!ids || !d_labels_out))) return GC_E_ARG;
    if (n == 0) return GC_OK;
    SbStage *st = nullptr;
    const uint32_t *d_ids = nullptr;
    int rc = io_ids(*e, "gc_stream_eval_batch_return_labels_dev", true, ids, n, &st, &d_ids);  // (a wire never set reads as 0)
    if (rc != GC_OK) return rc;
    gcsb::launch_return_labels(e->d_store, e->bstride, d_ids, n, (uint4 *)d_labels_out, e->S, e->ctx->stream);
    return ids_launched(*e, st);
}

// the buffer of a feed: [keep bytes from the buffer before | the chunk], on the handle's upload stream
int in_upload(gc_stream_eval_batch_in *h, const gcsb::Intake::Feed &f, const uint8_t *chunk, size_t stride,
              gc_stream_eval_batch_in::Buf **out) {
    gc_stream_eval_batch *e = h->e;
    gc_stream_eval_batch_in::Buf &prev = h->buf[h->cur], &b = h->buf[h->cur ^ 1u];
    const size_t pitch = up16(f.width), need = (size_t)e->S * pitch;
    if (b.dev_cap < need) {  // (freed only when what read it has run: the copy of its tail into `prev`, its ingesters)
        if (b.in_flight) GC_HIP(hipStreamSynchronize(e->up));
        if (b.in_use) GC_HIP(hipEventSynchronize(b.consumed));
        uint8_t *nw = nullptr;
        const size_t cap = std::max<size_t>(need + need / 2, (size_t)1 << 16);
        GC_HIP(hipMalloc((void **)&nw, cap));
        if (b.dev) (void)hipFree(b.dev);
        b.dev = nw, b.dev_cap = cap, b.in_use = false;
    } else if (b.in_use) {
        GC_HIP(hipStreamWaitEvent(e->up, b.consumed, 0));
    }
    const bool pinned = gc_host_is_pinned(chunk) != 0;
    if (!pinned) {
        const size_t pneed = (size_t)e->S * f.n;
        if (b.in_flight) GC_HIP(hipEventSynchronize(b.uploaded));  // (the staging's previous chunk has left)
        if (b.pin_cap < pneed) {
            uint8_t *nw = nullptr;
            const size_t cap = std::max<size_t>(pneed + pneed / 2, (size_t)1 << 16);
            GC_HIP(hipHostMalloc((void **)&nw, cap, hipHostMallocDefault));
            if (b.pin) (void)hipHostFree(b.pin);
            b.pin = nw, b.pin_cap = cap;
        }
    }
    // ---- nothing below allocates
    b.pitch = pitch;
    if (f.keep)  // the tail moves to the front: the open message is contiguous wherever it is evaluated
        GC_HIP(hipMemcpy2DAsync(b.dev, pitch, prev.dev + h->tail_at, prev.pitch, f.keep, e->S, hipMemcpyDeviceToDevice, e->up));
    if (pinned) {  // (one session: its stride is not looked at, and a source pitch below the width would be refused)
        GC_HIP(hipMemcpy2DAsync(b.dev + f.keep, pitch, chunk, e->S > 1 ? stride : f.n, f.n, e->S, hipMemcpyHostToDevice, e->up));
    } else {
        for (uint32_t s = 0; s < e->S; s++) std::memcpy(b.pin + (size_t)s * f.n, chunk + (size_t)s * stride, f.n);
        GC_HIP(hipMemcpy2DAsync(b.dev + f.keep, pitch, b.pin, f.n, f.n, e->S, hipMemcpyHostToDevice, e->up));
    }
    GC_HIP(hipEventRecord(b.uploaded, e->up));
    b.in_flight = true;
    GC_HIP(hipStreamWaitEvent(e->ctx->stream, b.uploaded, 0));
    *out = &b;
    return GC_OK;
}

int in_feed(gc_stream_eval_batch_in *h, const uint8_t *chunk, size_t stride, size_t len, size_t *taken, uint32_t *next_op) {
    if (!h || !taken || !next_op || (len && !chunk)) return GC_E_ARG;
    *taken = 0, *next_op = gcsb::Intake::kOpCircuit;
    gc_stream_eval_batch *e = h->e;
    if (e->S > 1 && stride < len) return GC_E_ARG;
    if (e->ctx->capturing) return GC_E_ARG;
    if (len == 0) return GC_OK;
    if (len >= 0x7fffffffu || h->st.held + len >= 0x7fffffffu) return refuse("gc_stream_eval_batch_in_feed", "a chunk of 2 GiB or more");
    GC_HIP(hipSetDevice(e->ctx->device));
    gcsb::Intake::Feed f = h->st.plan_feed(len);
    gc_stream_eval_batch_in::Buf *b = nullptr;
    int rc = in_upload(h, f, chunk, stride, &b);
    if (rc != GC_OK) return rc;  // (nothing has changed: the tail is where it was)
    // the reference session's bytes, contiguous: the caller's own while nothing is held
    const uint8_t *ref = chunk + (size_t)h->ref * stride;
    if (f.keep) {
        h->ref_buf.resize(f.width);
        std::memcpy(h->ref_buf.data() + f.keep, ref, len);
        ref = h->ref_buf.data();
    }
    h->msg_off.clear();
    int hip_rc = GC_OK;
    for (;;) {
        gcsb::Intake::Header hd;
        gcsb::Intake::Found x = h->st.frame(ref + f.at, gcsb::Intake::avail(f), &hd);
        if (x.kind == gcsb::Intake::kMessage) {
            const size_t at = f.at + gcsb::Intake::kHeader;
            const Supplier supply = [&](size_t, const void **d_blocks, size_t *pitch_out) -> int {
                *d_blocks = b->dev + at, *pitch_out = b->pitch;
                return GC_OK;
            };
            size_t used = 0;
            rc = eval_step(e, hd.ngates, hd.ntmp, hd.nwires, ref + at, f.width - at, nullptr, 0, e->d_badsum, &used, &supply);
            if (rc == GC_OK) {
                h->msg_off.push_back((uint32_t)f.at);
                x.len = gcsb::Intake::kHeader + used;
            } else if (rc == GC_E_ROWS) {  // the bytes end inside the block: wait for more
                x.kind = gcsb::Intake::kMore;
            } else {
                x.kind = gcsb::Intake::kRefused, x.rc = rc;
                if (rc == GC_E_HIP || rc == GC_E_NOMEM) hip_rc = rc;
            }
        }
        if (!h->st.apply(f, x)) break;
    }
    // the headers of the evaluated messages against the reference session's, in one launch; then the buffer is the ingesters'
    if (!h->msg_off.empty()) {
        SbStage *stg = nullptr;
        const uint32_t *d_off = nullptr;
        const int rcf = io_ids(*e, "gc_stream_eval_batch_in_feed", false, nullptr, 0, &stg, &d_off, h->msg_off.data(), (uint32_t)h->msg_off.size());
        if (rcf == GC_OK) {
            gcsb::launch_frames(b->dev, b->pitch, d_off, (uint32_t)h->msg_off.size(), e->S, h->ref, e->d_badsum, e->ctx->stream);
            const int rcl = ids_launched(*e, stg);
            if (rcl != GC_OK && hip_rc == GC_OK) hip_rc = rcl;
        } else if (hip_rc == GC_OK) {
            hip_rc = rcf;
        }
    }
    const hipError_t err = hipEventRecord(b->consumed, e->ctx->stream);
    b->in_use = err == hipSuccess;
    // the tail: in this buffer from f.at on, and the reference session's on the host
    if (f.carry) {
        if (ref == h->ref_buf.data()) {
            std::memmove(h->ref_buf.data(), h->ref_buf.data() + f.at, f.carry);
        } else {
            h->ref_buf.resize(f.carry);
            std::memcpy(h->ref_buf.data(), ref + f.at, f.carry);
        }
    }
    h->cur ^= 1u, h->tail_at = f.at;  // (not before: a parser that throws leaves the tail in the buffer before)
    h->st.commit(f, true);
    *taken = f.taken, *next_op = f.next_op;
    if (hip_rc != GC_OK) return hip_rc;
    GC_HIP(err);
    return f.rc;
}

}  // namespace

extern "C" {

int gc_stream_batch_select_labels_dev(gc_stream_batch *s, const uint32_t *ids, uint32_t n, const void *d_bits, void *d_labels_out) try {
    return select_dev(s, ids, n, d_bits, d_labels_out);
} catch (...) {
    return gc::on_exception();
}

int gc_stream_batch_decode_dev(gc_stream_batch *s, const uint32_t *ids, uint32_t n, const void *d_labels, void *d_bits_out,
                               void *d_bad) try {
    return decode_dev(s, ids, n, d_labels, d_bits_out, d_bad);
} catch (...) {
    return gc::on_exception();
}

int gc_stream_batch_select_labels(gc_stream_batch *s, const uint32_t *ids, uint32_t n, const uint8_t *bits, gc_label *labels_out) try {
    if (!s || (n && (!ids || !bits || !labels_out))) return GC_E_ARG;
    if (n == 0) return GC_OK;
    if (s->ctx->capturing) return GC_E_ARG;
    std::lock_guard<std::mutex> lock(s->ctx->mu);  // (a host form: §17)
    GC_HIP(hipSetDevice(s->ctx->device));
    const size_t cells = (size_t)s->S * n;
    Staged io[] = {{bits, nullptr, cells}, {nullptr, labels_out, cells * sizeof(gc_label)}};
    int rc = stage_in(io, std::size(io), s->ctx->stream);
    if (rc == GC_OK) rc = select_dev(s, ids, n, io[0].d.p, io[1].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), s->ctx->stream);
    return rc;
} catch (...) {
    return gc::on_exception();
}

int gc_stream_batch_decode(gc_stream_batch *s, const uint32_t *ids, uint32_t n, const gc_label *labels, uint8_t *bits_out,
                           uint32_t *bad_out) try {
    if (!s || !bad_out || (n && (!ids || !labels || !bits_out))) return GC_E_ARG;
    if (s->ctx->capturing) return GC_E_ARG;
    std::lock_guard<std::mutex> lock(s->ctx->mu);  // (a host form: §17)
    GC_HIP(hipSetDevice(s->ctx->device));
    const size_t cells = (size_t)s->S * n;
    Staged io[] = {{labels, nullptr, cells * sizeof(gc_label)}, {nullptr, bits_out, cells}, {nullptr, bad_out, (size_t)s->S * sizeof(uint32_t)}};
    int rc = stage_in(io, std::size(io), s->ctx->stream);
    if (rc == GC_OK) rc = decode_dev(s, ids, n, io[0].d.p, io[1].d.p, io[2].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), s->ctx->stream);
    return rc;
} catch (...) {
    return gc::on_exception();
}

static gc_stream_batch_out *out_create(gc_stream_batch *s, size_t window_bytes, uint32_t nwindows, bool split, int *status) try {
    int rc = GC_OK;
    std::unique_ptr<gc_stream_batch_out> h(new (std::nothrow) gc_stream_batch_out);
    if (!h) rc = GC_E_NOMEM;
    if (h) h->split = split;
    if (rc == GC_OK && (!s || window_bytes == 0 || window_bytes > ((size_t)1 << 40) || nwindows > 4096)) rc = GC_E_ARG;
    if (rc == GC_OK && !h->ring.init(window_bytes, nwindows)) rc = GC_E_ARG;
    auto setup = [&]() -> int {
        h->sb = s;
        const char *e = std::getenv("GC_STREAM_BATCH_OUT_WHOLE_ROWS");
        h->whole_rows = e && *e && *e != '0';
        GC_HIP(hipSetDevice(s->ctx->device));
        GC_HIP(hipStreamCreateWithFlags(&h->copy, hipStreamNonBlocking));
        h->win.resize(nwindows);
        for (uint32_t k = 0; k < nwindows; k++) {
            GC_HIP(hipEventCreateWithFlags(&h->win[k].sealed, hipEventDisableTiming));
            GC_HIP(hipEventCreateWithFlags(&h->win[k].copied, hipEventDisableTiming));
            const int r = h->make(h->ring.cap[k], &h->win[k]);
            if (r != GC_OK) return r;
        }
        return GC_OK;
    };
    if (rc == GC_OK) rc = setup();
    if (status) *status = rc;
    return rc == GC_OK ? h.release() : nullptr;
} catch (...) {
    const int rc__ = gc::on_exception();
    if (status) *status = rc__;
    return nullptr;
}

gc_stream_batch_out *gc_stream_batch_out_create(gc_stream_batch *s, size_t window_bytes, uint32_t nwindows, int *status) {
    return out_create(s, window_bytes, nwindows, false, status);
}

gc_stream_batch_out *gc_stream_batch_out_create_split(gc_stream_batch *s, size_t window_bytes, uint32_t nwindows, int *status) {
    return out_create(s, window_bytes, nwindows, true, status);
}

int gc_stream_batch_out_split_stats(const gc_stream_batch_out *h, uint64_t *split_steps, uint64_t *segments) try {
    if (!h) return GC_E_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    if (split_steps) *split_steps = h->split_steps;
    if (segments) *segments = h->segments;
    return GC_OK;
} catch (...) {
    return gc::on_exception();
}

int gc_stream_batch_set_fallback(gc_stream_batch *s, int on) {
    if (!s) return GC_E_ARG;
    s->fallback = on != 0;
    return GC_OK;
}

int gc_stream_eval_batch_set_fallback(gc_stream_eval_batch *e, int on) {
    if (!e) return GC_E_ARG;
    e->fallback = on != 0;
    return GC_OK;
}

void gc_stream_batch_out_free(gc_stream_batch_out *h) { delete h; }

int gc_stream_batch_out_garble(gc_stream_batch_out *h, const uint8_t *prefix, size_t prefix_len, const gc_gate *gates, uint32_t ngates,
                               uint32_t nwires, const uint32_t *in, uint32_t nin, const uint32_t *out, uint32_t nout,
                               size_t *written) try {
    return out_garble(h, prefix, prefix_len, gates, ngates, nwires, in, nin, out, nout, written);
} catch (...) {
    return gc::on_exception();
}

int gc_stream_batch_out_flush(gc_stream_batch_out *h) try {
    if (!h) return GC_E_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    size_t n = 0;
    const uint32_t w = h->ring.plan_flush(&n);
    if (w == gcsb::WindowRing::kNoWindow) return GC_OK;
    GC_HIP(hipSetDevice(h->sb->ctx->device));
    const int rc = h->seal(w, n);
    if (rc == GC_OK) h->ring.commit_flush();
    return rc;
} catch (...) {
    return gc::on_exception();
}

int gc_stream_batch_out_next(gc_stream_batch_out *h, const uint8_t **base, size_t *stride, size_t *len) try {
    if (!h || !base || !stride || !len) return GC_E_ARG;
    *base = nullptr, *stride = 0, *len = 0;
    hipEvent_t copied = nullptr;
    {
        std::lock_guard<std::mutex> lock(h->mu);
        size_t n = 0;
        const uint32_t w = h->ring.next(&n);
        if (w == gcsb::WindowRing::kNoWindow) return GC_OK;
        *base = h->win[w].pin, *stride = h->ring.cap[w], *len = n;
        copied = h->win[w].copied;
    }
    GC_HIP(hipSetDevice(h->sb->ctx->device));
    GC_HIP(hipEventSynchronize(copied));
    return GC_OK;
} catch (...) {
    return gc::on_exception();
}

int gc_stream_batch_out_release(gc_stream_batch_out *h) try {
    if (!h) return GC_E_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    return h->ring.release() == gcsb::WindowRing::kNoWindow ? GC_E_ARG : GC_OK;
} catch (...) {
    return gc::on_exception();
}

int gc_stream_batch_out_stats(const gc_stream_batch_out *h, uint64_t *sealed, uint64_t *bytes_per_session, uint64_t *grown,
                              uint64_t *busy) try {
    if (!h) return GC_E_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    if (sealed) *sealed = h->ring.sealed;
    if (bytes_per_session) *bytes_per_session = h->ring.bytes_per_session;
    if (grown) *grown = h->ring.grown;
    if (busy) *busy = h->ring.busy;
    return GC_OK;
} catch (...) {
    return gc::on_exception();
}

int gc_stream_eval_batch_circuit_host(gc_stream_eval_batch *e, uint32_t ngates, uint32_t ntmp, uint32_t nwires, const uint8_t *blocks,
                                      size_t stride, size_t len, uint32_t ref_session, size_t *consumed) try {
    return eval_host(e, ngates, ntmp, nwires, blocks, stride, len, ref_session, consumed);
} catch (...) {
    return gc::on_exception();
}

int gc_stream_eval_batch_uploads_wait(gc_stream_eval_batch *e) try {
    if (!e) return GC_E_ARG;
    GC_HIP(hipSetDevice(e->ctx->device));
    if (e->up) GC_HIP(hipStreamSynchronize(e->up));
    return GC_OK;
} catch (...) {
    return gc::on_exception();
}

int gc_stream_eval_batch_bad(gc_stream_eval_batch *e, uint32_t *bad_out) try {
    if (!e || !bad_out) return GC_E_ARG;
    GC_HIP(hipSetDevice(e->ctx->device));
    if (e->up) GC_HIP(hipStreamSynchronize(e->up));
    if (e->d_badsum)
        GC_HIP(hipMemcpyAsync(bad_out, e->d_badsum, (size_t)e->S * sizeof(uint32_t), hipMemcpyDeviceToHost, e->ctx->stream));
    else
        std::memset(bad_out, 0, (size_t)e->S * sizeof(uint32_t));
    GC_HIP(hipStreamSynchronize(e->ctx->stream));
    return GC_OK;
} catch (...) {
    return gc::on_exception();
}

int gc_stream_eval_batch_return_labels_dev(gc_stream_eval_batch *e, const uint32_t *ids, uint32_t n, void *d_labels_out) try {
    return return_dev(e, ids, n, d_labels_out);
} catch (...) {
    return gc::on_exception();
}

int gc_stream_eval_batch_return_labels(gc_stream_eval_batch *e, const uint32_t *ids, uint32_t n, gc_label *labels_out) try {
    if (!e || (n && (!ids || !labels_out))) return GC_E_ARG;
    if (n == 0) return GC_OK;
    if (e->ctx->capturing) return GC_E_ARG;
    std::lock_guard<std::mutex> lock(e->ctx->mu);  // (a host form: §17)
    GC_HIP(hipSetDevice(e->ctx->device));
    Staged io[] = {{nullptr, labels_out, (size_t)e->S * n * sizeof(gc_label)}};
    int rc = stage_in(io, std::size(io), e->ctx->stream);
    if (rc == GC_OK) rc = return_dev(e, ids, n, io[0].d.p);
    if (rc == GC_OK) rc = stage_out(io, std::size(io), e->ctx->stream);
    return rc;
} catch (...) {
    return gc::on_exception();
}

gc_stream_eval_batch_in *gc_stream_eval_batch_in_create(gc_stream_eval_batch *e, uint32_t ref_session, size_t max_message_bytes,
                                                        int *status) try {
    int rc = GC_OK;
    std::unique_ptr<gc_stream_eval_batch_in> h(new (std::nothrow) gc_stream_eval_batch_in);
    if (!h) rc = GC_E_NOMEM;
    if (rc == GC_OK && (!e || ref_session >= e->S || max_message_bytes >= 0x7fffffffu || !h->st.init(max_message_bytes))) rc = GC_E_ARG;
    auto setup = [&]() -> int {
        const int r = eval_host_setup(e);
        if (r != GC_OK) return r;
        for (auto &b : h->buf) {
            GC_HIP(hipEventCreateWithFlags(&b.uploaded, hipEventDisableTiming));
            GC_HIP(hipEventCreateWithFlags(&b.consumed, hipEventDisableTiming));
        }
        h->e = e, h->ref = ref_session;
        return GC_OK;
    };
    if (rc == GC_OK) rc = setup();
    if (status) *status = rc;
    return rc == GC_OK ? h.release() : nullptr;
} catch (...) {
    const int rc__ = gc::on_exception();
    if (status) *status = rc__;
    return nullptr;
}

void gc_stream_eval_batch_in_free(gc_stream_eval_batch_in *h) { delete h; }

int gc_stream_eval_batch_in_feed(gc_stream_eval_batch_in *h, const uint8_t *chunk, size_t stride, size_t len, size_t *taken,
                                 uint32_t *next_op) try {
    return in_feed(h, chunk, stride, len, taken, next_op);
} catch (...) {
    return gc::on_exception();
}

int gc_stream_eval_batch_in_stats(const gc_stream_eval_batch_in *h, uint64_t *steps, uint64_t *bytes_per_session, uint64_t *uploads,
                                  uint64_t *carried_bytes) {
    if (!h) return GC_E_ARG;
    if (steps) *steps = h->st.steps;
    if (bytes_per_session) *bytes_per_session = h->st.bytes_per_session;
    if (uploads) *uploads = h->st.uploads;
    if (carried_bytes) *carried_bytes = h->st.carried_bytes;
    return GC_OK;
}

}  // extern "C"
