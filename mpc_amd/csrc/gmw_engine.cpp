// gmw_engine.cpp — the GMW party engine (gcengine.h: gc_gmw_*): one party of the n-party GMW online phase over a batch of
// instances of one circuit (gmw/network.go:563-624, andBatchFlush :660-757), and the local folds of tripleBatch
// (gmw/triples.go:287-466).  Host side: plan upload, pass state machine, launches; gmw_kernels.hip is the device side.
//
// A pass is set_inputs (1 launch), set_triples (none), R + 1 steps (1 launch each; R = AND levels), get_outputs (a copy):
// R + 2 launches.  The handle owns the slot store [nslots][ceil(batch/64)] u64 and two message buffers (this party's d, e
// of the level being opened and of the level being closed, alternately), so the caller's msg_out may be reused at once.
#include <algorithm>
#include <new>

#include "engine.h"
#include "gmw.h"

struct gc_gmw {
    gc_ctx *ctx = nullptr;
    gc::GmwPlan plan;
    uint32_t nparties = 0, party = 0, batch = 0, bw = 0;
    uint64_t *d_slots = nullptr;
    gc::GmwGate *d_gates = nullptr;
    uint32_t *d_idx = nullptr;   // sub offsets, AND slot lists, output slots (one allocation)
    uint32_t *d_sub = nullptr, *d_out_slots = nullptr;
    uint64_t *d_own[2] = {nullptr, nullptr};  // [2][max_level_words][batch]
    uint64_t *d_out = nullptr;                // [ceil(noutputs/64)][batch]
    uint64_t *d_trip = nullptr;               // host-form triples: a, b, c [TW][batch] each (on first use)
    uint64_t *d_msg = nullptr;                // host-form step: peers then msg_out (on first use)
    size_t msg_cap = 0;
    const uint64_t *ta = nullptr, *tb = nullptr, *tc = nullptr;
    bool have_inputs = false, have_triples = false, done = false;
    uint32_t round = 0;
    uint32_t launches = 0, last_launches = 0;
};

namespace {

void gmw_release(gc_gmw *g) {
    if (!g) return;
    if (g->ctx) (void)hipSetDevice(g->ctx->device);
    for (void *p : {(void *)g->d_slots, (void *)g->d_gates, (void *)g->d_idx, (void *)g->d_own[0], (void *)g->d_own[1],
                    (void *)g->d_out, (void *)g->d_trip, (void *)g->d_msg})
        if (p) (void)hipFree(p);
    delete g;
}

template <class T>
hipError_t upload(T **d, const std::vector<T> &v, hipStream_t s) {
    const size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
    hipError_t e = hipMalloc((void **)d, bytes);
    if (e == hipSuccess && !v.empty()) e = hipMemcpyAsync(*d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s);
    return e;
}

size_t msg_words(const gc_gmw *g, uint32_t w) { return (size_t)2 * w * g->batch; }

int gmw_create(gc_gmw *g, const gc_gate *gates, uint32_t ngates, uint32_t nwires, uint32_t ninputs, uint32_t noutputs) {
    int rc = gc::build_gmw_plan(gates, ngates, nwires, ninputs, noutputs, &g->plan);
    if (rc != GC_OK) return rc;
    const gc::GmwPlan &p = g->plan;
    hipStream_t s = g->ctx->stream;
    GC_HIP(hipSetDevice(g->ctx->device));
    GC_HIP(hipMalloc((void **)&g->d_slots, std::max<size_t>((size_t)p.nslots * g->bw * 8, 16)));
    GC_HIP(upload(&g->d_gates, p.gates, s));
    std::vector<uint32_t> idx(p.sub);
    idx.insert(idx.end(), p.idx.begin(), p.idx.end());
    idx.insert(idx.end(), p.out_slots.begin(), p.out_slots.end());
    GC_HIP(upload(&g->d_idx, idx, s));
    g->d_sub = g->d_idx;
    g->d_out_slots = g->d_idx + p.sub.size() + p.idx.size();
    const size_t own = std::max<size_t>(msg_words(g, p.info.max_level_words) * 8, 16);
    GC_HIP(hipMalloc((void **)&g->d_own[0], own));
    GC_HIP(hipMalloc((void **)&g->d_own[1], own));
    GC_HIP(hipMalloc((void **)&g->d_out, std::max<size_t>((size_t)((noutputs + 63) / 64) * g->batch * 8, 16)));
    GC_HIP(hipStreamSynchronize(s));  // the host vectors of the uploads are the plan's own; keep nothing pending
    return GC_OK;
}

}  // namespace

extern "C" {

gc_gmw *gc_gmw_create(gc_ctx *ctx, const gc_gate *gates, uint32_t ngates, uint32_t nwires, uint32_t ninputs, uint32_t noutputs,
                      uint32_t nparties, uint32_t party, uint32_t batch, int *status) try {
    int rc = GC_OK;
    gc_gmw *g = nullptr;
    if (!ctx || nparties < 2 || party >= nparties || batch == 0) rc = GC_E_ARG;
    if (rc == GC_OK) {
        g = new (std::nothrow) gc_gmw;
        if (!g) rc = GC_E_NOMEM;
    }
    if (rc == GC_OK) {
        g->ctx = ctx;
        g->nparties = nparties;
        g->party = party;
        g->batch = batch;
        g->bw = (batch + 63) / 64;
        rc = gmw_create(g, gates, ngates, nwires, ninputs, noutputs);
        if (rc != GC_OK) {
            gmw_release(g);
            g = nullptr;
        }
    }
    if (status) *status = rc;
    return g;
} catch (...) {
    const int rc__ = gc::on_exception();
    if (status) *status = rc__;
    return nullptr;
}

void gc_gmw_free(gc_gmw *g) {
    if (g && g->ctx) (void)hipStreamSynchronize(g->ctx->stream);
    gmw_release(g);
}

int gc_gmw_get_info(const gc_gmw *g, gc_gmw_info *out) {
    if (!g || !out) return GC_E_ARG;
    *out = g->plan.info;
    return GC_OK;
}

uint32_t gc_gmw_last_launches(const gc_gmw *g) { return g ? g->last_launches : 0; }

int gc_gmw_set_inputs_dev(gc_gmw *g, const void *d_inputs) {
    if (!g || (!d_inputs && g->plan.info.ninputs)) return GC_E_ARG;
    if (g->ctx->capturing) return GC_E_ARG;  // the pass state advances on the host: nothing to replay
    GC_HIP(hipSetDevice(g->ctx->device));
    g->have_inputs = g->have_triples = g->done = false;
    g->round = 0;
    g->launches = 0;
    if (g->plan.info.ninputs) {
        GC_HIP(gc::gmw_launch_inputs(g->ctx->stream, g->d_slots, (const uint64_t *)d_inputs, g->plan.info.ninputs, g->batch, g->bw));
        g->launches++;
    }
    g->have_inputs = true;
    return GC_OK;
}

int gc_gmw_set_inputs(gc_gmw *g, const uint64_t *inputs) {
    if (!g || (!inputs && g->plan.info.ninputs)) return GC_E_ARG;
    const size_t bytes = (size_t)((g->plan.info.ninputs + 63) / 64) * g->batch * 8;
    if (!bytes) return gc_gmw_set_inputs_dev(g, nullptr);
    GC_HIP(hipSetDevice(g->ctx->device));
    // staged through the host-form message buffer, sized on demand
    if (g->msg_cap < bytes) {
        if (g->d_msg) GC_HIP(hipFree(g->d_msg));
        g->d_msg = nullptr;
        g->msg_cap = 0;
        GC_HIP(hipMalloc((void **)&g->d_msg, bytes));
        g->msg_cap = bytes;
    }
    GC_HIP(hipMemcpyAsync(g->d_msg, inputs, bytes, hipMemcpyHostToDevice, g->ctx->stream));
    int rc = gc_gmw_set_inputs_dev(g, g->d_msg);
    if (rc != GC_OK) return rc;
    GC_HIP(hipStreamSynchronize(g->ctx->stream));
    return GC_OK;
}

int gc_gmw_set_triples_dev(gc_gmw *g, const void *d_a, const void *d_b, const void *d_c) {
    if (!g || !g->have_inputs || g->round || (g->plan.info.triple_words && (!d_a || !d_b || !d_c))) return GC_E_ARG;
    g->ta = (const uint64_t *)d_a;
    g->tb = (const uint64_t *)d_b;
    g->tc = (const uint64_t *)d_c;
    g->have_triples = true;
    return GC_OK;
}

int gc_gmw_set_triples(gc_gmw *g, const uint64_t *a, const uint64_t *b, const uint64_t *c) {
    if (!g || !g->have_inputs || g->round) return GC_E_ARG;
    const size_t words = (size_t)g->plan.info.triple_words * g->batch;
    if (!words) return gc_gmw_set_triples_dev(g, nullptr, nullptr, nullptr);
    if (!a || !b || !c) return GC_E_ARG;
    GC_HIP(hipSetDevice(g->ctx->device));
    if (!g->d_trip) GC_HIP(hipMalloc((void **)&g->d_trip, 3 * words * 8));
    hipStream_t s = g->ctx->stream;
    GC_HIP(hipMemcpyAsync(g->d_trip, a, words * 8, hipMemcpyHostToDevice, s));
    GC_HIP(hipMemcpyAsync(g->d_trip + words, b, words * 8, hipMemcpyHostToDevice, s));
    GC_HIP(hipMemcpyAsync(g->d_trip + 2 * words, c, words * 8, hipMemcpyHostToDevice, s));
    GC_HIP(hipStreamSynchronize(s));
    return gc_gmw_set_triples_dev(g, g->d_trip, g->d_trip + words, g->d_trip + 2 * words);
}

int gc_gmw_step_dev(gc_gmw *g, const void *d_peer_msgs, uint32_t npeers, void *d_msg_out, uint32_t *level, size_t *words) {
    if (!g || !level || !words) return GC_E_ARG;
    if (!g->have_inputs || g->done || npeers != g->nparties - 1) return GC_E_ARG;
    if (!g->have_triples && g->plan.info.triple_words) return GC_E_ARG;
    if (g->ctx->capturing) return GC_E_ARG;
    const gc::GmwPlan &p = g->plan;
    const gc::GmwRound &R = p.rounds[g->round];
    const gc::GmwRound *prev = g->round ? &p.rounds[g->round - 1] : nullptr;
    if (prev && prev->and_n && npeers && !d_peer_msgs) return GC_E_ARG;
    if (R.and_n && !d_msg_out) return GC_E_ARG;
    GC_HIP(hipSetDevice(g->ctx->device));
    gc::GmwStepArgs a{};
    a.slots = g->d_slots;
    a.gates = g->d_gates + R.gate_first;
    a.sub = g->d_sub + R.sub_first;
    a.nsub = R.nsub;
    const uint32_t idx0 = (uint32_t)p.sub.size();  // the AND slot lists follow the sub-round offsets in d_idx
    if (prev && prev->and_n) {
        a.close_out = g->d_idx + idx0 + prev->and_out;
        a.close_n = prev->and_n;
        a.close_w = prev->and_w;
        a.close_W = prev->and_W;
        a.own_prev = g->d_own[(g->round - 1) & 1];
        a.peers = (const uint64_t *)d_peer_msgs;
        a.npeers = npeers;
    }
    if (R.and_n) {
        a.and_in = g->d_idx + idx0 + R.and_in;
        a.and_n = R.and_n;
        a.and_w = R.and_w;
        a.and_W = R.and_W;
        a.own_next = g->d_own[g->round & 1];
        a.msg_out = (uint64_t *)d_msg_out;
    }
    a.ta = g->ta;
    a.tb = g->tb;
    a.tc = g->tc;
    const bool last = g->round + 1 == p.rounds.size();
    if (last) {
        a.out_slots = g->d_out_slots;
        a.nout = p.info.noutputs;
        a.out = g->d_out;
    }
    a.batch = g->batch;
    a.bw = g->bw;
    a.party0 = g->party == 0;
    GC_HIP(gc::gmw_launch_step(g->ctx->stream, a));
    g->launches++;
    *level = R.level;
    *words = R.and_w;
    g->round++;
    if (last) {
        g->done = true;
        g->last_launches = g->launches;
    }
    return GC_OK;
}

int gc_gmw_step(gc_gmw *g, const uint64_t *peer_msgs, uint32_t npeers, uint64_t *msg_out, uint32_t *level, size_t *words) {
    if (!g || !level || !words) return GC_E_ARG;
    if (!g->have_inputs || g->done || npeers != g->nparties - 1) return GC_E_ARG;
    const gc::GmwPlan &p = g->plan;
    const gc::GmwRound &R = p.rounds[g->round];
    const gc::GmwRound *prev = g->round ? &p.rounds[g->round - 1] : nullptr;
    const size_t in_words = prev && prev->and_n ? npeers * msg_words(g, prev->and_w) : 0;
    const size_t out_words = msg_words(g, R.and_w);
    if ((in_words && !peer_msgs) || (out_words && !msg_out)) return GC_E_ARG;
    GC_HIP(hipSetDevice(g->ctx->device));
    const size_t bytes = std::max<size_t>((in_words + out_words) * 8, 16);
    if (g->msg_cap < bytes) {
        if (g->d_msg) GC_HIP(hipFree(g->d_msg));
        g->d_msg = nullptr;
        g->msg_cap = 0;
        GC_HIP(hipMalloc((void **)&g->d_msg, bytes));
        g->msg_cap = bytes;
    }
    hipStream_t s = g->ctx->stream;
    if (in_words) GC_HIP(hipMemcpyAsync(g->d_msg, peer_msgs, in_words * 8, hipMemcpyHostToDevice, s));
    int rc = gc_gmw_step_dev(g, in_words ? g->d_msg : nullptr, npeers, g->d_msg + in_words, level, words);
    if (rc != GC_OK) return rc;
    if (out_words) GC_HIP(hipMemcpyAsync(msg_out, g->d_msg + in_words, out_words * 8, hipMemcpyDeviceToHost, s));
    GC_HIP(hipStreamSynchronize(s));
    return GC_OK;
}

int gc_gmw_get_outputs_dev(gc_gmw *g, void *d_out) {
    if (!g || !g->done) return GC_E_ARG;
    const size_t bytes = (size_t)((g->plan.info.noutputs + 63) / 64) * g->batch * 8;
    if (!bytes) return GC_OK;
    if (!d_out) return GC_E_ARG;
    GC_HIP(hipSetDevice(g->ctx->device));
    GC_HIP(hipMemcpyAsync(d_out, g->d_out, bytes, hipMemcpyDeviceToDevice, g->ctx->stream));
    return GC_OK;
}

int gc_gmw_get_outputs(gc_gmw *g, uint64_t *out) {
    if (!g || !g->done) return GC_E_ARG;
    const size_t bytes = (size_t)((g->plan.info.noutputs + 63) / 64) * g->batch * 8;
    if (!bytes) return GC_OK;
    if (!out) return GC_E_ARG;
    GC_HIP(hipSetDevice(g->ctx->device));
    GC_HIP(hipMemcpyAsync(out, g->d_out, bytes, hipMemcpyDeviceToHost, g->ctx->stream));
    GC_HIP(hipStreamSynchronize(g->ctx->stream));
    return GC_OK;
}

// ---- Beaver triple folds (tripleBatch's local loops) ----

static int gmw_fold(gc_ctx *ctx, int kind, uint32_t delta_bit, const void *x, const void *y, const void *z, void *c, size_t words) {
    if (!ctx) return GC_E_ARG;
    if (!words) return GC_OK;
    if (!x || !c || (kind == 0 && !y) || (kind == 2 && (!y || !z))) return GC_E_ARG;
    GC_HIP(hipSetDevice(ctx->device));
    GC_HIP(gc::gmw_launch_fold(ctx->stream, kind, delta_bit, (const uint64_t *)x, (const uint64_t *)y, (const uint64_t *)z,
                               (uint64_t *)c, words));
    return GC_OK;
}

int gc_gmw_triples_local_dev(gc_ctx *ctx, const void *d_a, const void *d_b, void *d_c, size_t words) {
    return gmw_fold(ctx, 0, 0, d_a, d_b, nullptr, d_c, words);
}

int gc_gmw_triples_sender_u_dev(gc_ctx *ctx, uint32_t delta_bit, const void *d_a, void *d_u, size_t words) {
    return gmw_fold(ctx, 1, delta_bit, d_a, nullptr, nullptr, d_u, words);
}

int gc_gmw_triples_sender_fold_dev(gc_ctx *ctx, const void *d_s, const void *d_u, const void *d_v, void *d_c, size_t words) {
    return gmw_fold(ctx, 2, 0, d_s, d_u, d_v, d_c, words);
}

int gc_gmw_triples_receiver_fold_dev(gc_ctx *ctx, const void *d_r, void *d_c, size_t words) {
    return gmw_fold(ctx, 3, 0, d_r, nullptr, nullptr, d_c, words);
}

}  // extern "C"
