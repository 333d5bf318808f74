// stream_eval.cpp — C ABI of the streaming evaluator (circuit.StreamEval): circuit/stream_evaluator.go:29-96
// (the wire store) and :226-432 (one OpCircuit block: parse, evaluate, Set the global outputs).  Blocks are grouped, laned and
// launched like the garbler's steps (stream_garble.cpp's head, stream_group.cpp); a block seen before is recognised by its byte
// skeleton (stream_skel.h).
#include "stream_eval_internal.h"

using namespace gcs;

namespace {

// a slot for a new group of blocks: nothing comes back from an evaluator group, so a launched group's slot is free as
// soon as its kernels have run; at most eight groups of the ctx stream in flight, then the oldest is waited for (deep
// blocks on their lanes are bounded by kDeepInFlight and not counted: waiting for a 2 ms multiplier would idle the ctx stream)
Slot *eval_slot(StreamCore &c, uint32_t *index, bool big) {
    auto done_with = [&](Slot &sl) {
        if (sl.deep_id) {
            if (sl.error != GC_OK) (void)hipStreamSynchronize(c.deep.lanes[(size_t)sl.lane]);
            c.deep.retire(sl.lane, sl.deep_id);
        }
        sl.reset();
    };
    uint32_t on_ctx = 0;
    bool any_free = false;
    for (auto &sl : c.slots) any_free = any_free || (sl->kind == Slot::kFree && (sl->arena_cap >= ((size_t)2 << 20)) == big);
    if (!any_free) {  // (an event query is a microsecond or two: only when a slot is wanted)
        for (uint32_t i = 0; i < c.slots.size(); i++) {
            Slot &sl = *c.slots[i];
            if (sl.kind == Slot::kGroup && sl.launched && (sl.error != GC_OK || hipEventQuery(sl.done) == hipSuccess)) done_with(sl);
            any_free = any_free || sl.kind == Slot::kFree;
        }
        (void)hipGetLastError();  // hipErrorNotReady of the queries
    }
    for (auto &sl : c.slots)
        if (sl->kind == Slot::kGroup && sl->launched && !sl->deep_id) on_ctx++;
    if (on_ctx >= 8 && !any_free) {
        // the OLDEST launched group (the first one in slot order may be the newest: waiting for that one drains
        // everything queued, and the GPU then idles until the next group is ready — 136 us between the groups of the mixed
        // program)
        Slot *oldest = nullptr;
        for (auto &sl : c.slots)
            if (sl->kind == Slot::kGroup && sl->launched && !sl->deep_id && (!oldest || sl->launch_no < oldest->launch_no)) oldest = sl.get();
        if (oldest) {
            (void)hipEventSynchronize(oldest->done);
            done_with(*oldest);
        }
    }
    return slot_new(c.ctx, c.slots, index, big);
}

// (the core's hook: the chunks of the peer's stream that the jobs of a launched group gather their rows from)
void eval_chunks_launched(StreamCore &c, Slot &g, uint32_t slot) { evdev_launched(static_cast<gc_stream_eval *>(&c), g, slot); }

}  // namespace

extern "C" {

gc_stream_eval *gc_stream_eval_create(gc_ctx *ctx, const uint8_t *key, size_t keylen, int *status) try {
    int rc = GC_OK;
    AesKey k;
    gc_stream_eval *e = nullptr;
    if (!ctx) rc = GC_E_ARG;
    else if (!key || !aes_expand_key(key, keylen, &k)) rc = GC_E_KEYSIZE;
    else if (!(e = new (std::nothrow) gc_stream_eval)) rc = GC_E_NOMEM;
    if (e) {
        e->ctx = ctx;
        e->eval = true;
        e->chunks_launched = eval_chunks_launched;
        e->key.assign(key, key + keylen);
        e->rounds = k.rounds;
        e->cache_budget = cache_budget_from_env();
        e->deep.read_env();
        e->use_skels = std::getenv("GC_STREAM_NO_SKELETON") == nullptr;
        hipError_t er = hipSetDevice(ctx->device);
        if (er == hipSuccess) er = hipMalloc((void **)&e->d_rk, sizeof k.w);
        if (er == hipSuccess) er = hipMemcpy(e->d_rk, k.w, sizeof k.w, hipMemcpyHostToDevice);
        if (er != hipSuccess) {
            set_error("gc_stream_eval_create", er);
            rc = GC_E_HIP;
            gc_stream_eval_free(e);
            e = nullptr;
        }
    }
    if (status) *status = rc;
    return e;
} catch (...) {
    const int rc__ = gc::on_exception();
    if (status) *status = rc__;
    return nullptr;
}

void gc_stream_eval_free(gc_stream_eval *e) {
    if (!e) return;
    e->prof.print("evaluator", e->n_blocks_total);
    if (e->ctx) {
        (void)hipSetDevice(e->ctx->device);
        (void)hipStreamSynchronize(e->ctx->stream);
    }
    e->deep.release();
    evdev_free(e);
    if (e->held) gc_circ_release_batch(e->held_circ, e->held);
    for (auto &kv : e->cache) gc_circ_free(kv.second.circ);
    for (auto &sl : e->slots) sl->release();
    if (e->d_rk) (void)hipFree(e->d_rk);
    if (e->d_io) (void)hipFree(e->d_io);
    if (e->up_stream) {
        (void)hipStreamSynchronize(e->up_stream);
        (void)hipStreamDestroy(e->up_stream);
    }
    for (int i = 0; i < (int)gc_stream_eval::kEvalRing; i++) {
        if (e->up_ev[i]) (void)hipEventDestroy(e->up_ev[i]);
        gc::ctx_buf_put(e->ctx, true, e->slab_pin[i], e->slab_cap[i] * sizeof(gc_label));
        if (e->slab_ev[i]) (void)hipEventDestroy(e->slab_ev[i]);
        gc::ctx_buf_put(e->ctx, true, e->io_pin[i], e->io_pin_cap[i] * sizeof(uint32_t));
        if (e->io_dev[i]) (void)hipFree(e->io_dev[i]);
    }
    e->store.release();
    delete e;
}

int gc_stream_eval_set_wire(gc_stream_eval *e, uint32_t w, const gc_label *l) try {
    if (!e || !l) return GC_E_ARG;
    int rc = close_group(*e);  // a queued block reads the wire's OLD label (the reference runs in program order)
    if (rc != GC_OK) return rc;
    if (e->deep.n_inflight) e->deep.drain();  // ... also a deep block on its lane
    e->store.set(w, *l);
    return GC_OK;
} catch (...) {
    return gc::on_exception();
}

int gc_stream_eval_stats(const gc_stream_eval *e, uint64_t *parsed, uint64_t *matched) {
    if (!e) return GC_E_ARG;
    if (parsed) *parsed = e->n_parsed;
    if (matched) *matched = e->n_matched;
    return GC_OK;
}

int gc_stream_eval_dev_stats(const gc_stream_eval *e, uint64_t *blocks, uint64_t *fallbacks) {
    if (!e) return GC_E_ARG;
    evdev_stats(e, blocks, fallbacks);
    return GC_OK;
}

int gc_stream_eval_fuse_stats(const gc_stream_eval *e, uint64_t *fused_units, uint64_t *fused_blocks, uint64_t *plans_built,
                              uint64_t *unfit) {
    return fuse_stats(e, fused_units, fused_blocks, plans_built, unfit);
}

int gc_stream_eval_wait_stats(const gc_stream_eval *e, uint64_t *waiting_units) { return wait_stats(e, waiting_units); }

int gc_stream_eval_deep_stats(const gc_stream_eval *e, uint64_t *deep_blocks, uint32_t *lanes) { return deep_stats(e, deep_blocks, lanes); }

int gc_stream_eval_get_wire(gc_stream_eval *e, uint32_t w, gc_label *l) try {
    if (!e || !l) return GC_E_ARG;
    int rc = close_group(*e);  // a queued block may be the one that writes the wire
    if (rc != GC_OK) return rc;
    if (e->deep.n_inflight) e->deep.drain();  // ... or a deep block on its lane
    rc = e->store.get(e->ctx, w, l);
    const int rcc = gc_ctx_coop_check(e->ctx);  // (the stream was waited for: a cooperative pass that lost a workgroup is noted here)
    return rc != GC_OK ? rc : rcc;
} catch (...) {
    return gc::on_exception();
}

}  // extern "C"

namespace gcs {

uint32_t stream_max_wires() {
    static const uint32_t v = [] {
        const char *e = std::getenv("GC_STREAM_MAX_WIRES");
        const unsigned long long n = e ? std::strtoull(e, nullptr, 0) : 0;
        return n ? (uint32_t)std::min<unsigned long long>(n, 0xffffffffull) : (1u << 28);
    }();
    return v;
}

// the global id fields gf_off (byte offset | 1 << 31 for the 4-byte form) of the block at buf
static void read_global_ids(const uint8_t *buf, const std::vector<uint32_t> &gf_off, std::vector<uint32_t> *ids) {
    ids->resize(gf_off.size());
    for (size_t f = 0; f < gf_off.size(); f++) {
        const uint8_t *q = buf + (gf_off[f] & 0x7fffffffu);
        (*ids)[f] = (gf_off[f] >> 31) ? ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3]
                                      : ((uint32_t)q[0] << 8) | q[1];
    }
}

// repeat pattern of a block's global ids: per field, the index of the first field naming the same wire (stamps in last_w
// under a generation of their own).  false: an id >= nwires, or a pattern other than expect[] (if given)
static bool canon_of(gc_stream_eval *e, const uint32_t *ids, uint32_t nf, uint32_t nwires, const uint32_t *expect,
                     std::vector<uint32_t> *canon) {
    gcw::WireStamps &st = e->stamps;
    const uint64_t gen = st.next_gen(), stamp = gen << 32;
    if (canon) canon->resize(nf);
    for (uint32_t f = 0; f < nf; f++) {
        const uint32_t id = ids[f];
        if (id >= nwires) return false;
        st.touch_w(id);
        uint32_t first = f;
        if ((st.last_w[id] >> 32) == gen) first = (uint32_t)st.last_w[id];
        else st.last_w[id] = stamp | f;
        if (expect && expect[f] != first) return false;
        if (canon) (*canon)[f] = first;
    }
    return true;
}

bool eval_adopt_ids(gc_stream_eval *e, const EvalSkel &sk, const uint32_t *ids, uint32_t nwires) {
    if (!canon_of(e, ids, (uint32_t)sk.gf_off.size(), nwires, sk.gf_canon.data(), nullptr)) return false;
    const uint32_t nin = sk.nin, nout = sk.nout;
    e->io_host.resize((size_t)nin + nout + 1);
    for (uint32_t k = 0; k < nin; k++) e->io_host[k] = ids[sk.in_gf[k]];
    e->wr_ids.resize(nout);
    for (uint32_t k = 0; k < nout; k++) {
        e->wr_ids[k] = ids[sk.out_gf[k]];
        e->io_host[nin + k] = sk.out_live[k] ? e->wr_ids[k] : 0xffffffffu;
    }
    return true;
}

// the row buffer of the block being taken in: a small block (candidate for a step group) parses its rows into plain host
// scratch — they are copied into the group's pinned upload region when the block is queued —, a big block uses the next entry
// of the pinned ring
int eval_rows_buffer(gc_stream_eval *e, uint32_t ngates, bool *small_block_out, uint32_t *sb_out, gc_label **slab_out) {
    const bool small_block = ngates <= kSmallGates;
    const uint32_t sb = e->slab_turn % gc_stream_eval::kEvalRing;
    if (small_block) {
        if (e->rows_scratch.size() < (size_t)ngates * 3 + 1) e->rows_scratch.resize((size_t)ngates * 3 + 1);
        GC_HIP(hipSetDevice(e->ctx->device));
    } else {
        e->slab_turn++;
        GC_HIP(hipSetDevice(e->ctx->device));
        if (!e->slab_ev[sb]) GC_HIP(hipEventCreateWithFlags(&e->slab_ev[sb], hipEventDisableTiming));
        else GC_HIP(hipEventSynchronize(e->slab_ev[sb]));  // the pass of the block kEvalRing calls ago (long done)
        const size_t want = (size_t)ngates * 3 + 1;
        if (e->slab_cap[sb] < want) {  // (from the ctx's lists: a stream's evaluator finds the buffers of the one before it)
            uint8_t *p = (uint8_t *)e->slab_pin[sb];
            size_t cap = e->slab_cap[sb] * sizeof(gc_label);
            const hipError_t eg = grow_pin(e->ctx, &p, &cap, want * sizeof(gc_label));
            e->slab_pin[sb] = (gc_label *)p;
            e->slab_cap[sb] = cap / sizeof(gc_label);
            GC_HIP(eg);
        }
    }
    gc_label *slab = small_block ? e->rows_scratch.data() : e->slab_pin[sb];
    *small_block_out = small_block, *sb_out = sb, *slab_out = slab;
    return GC_OK;
}

// a big block (or a small one without a one-workgroup plan: rare): its own launch sequence, behind everything queued
static int eval_big_block(gc_stream_eval *e, const BlockIn &in, StreamTrace &tr, size_t *consumed) {
    CircEntry *ent = in.ent;
    const uint32_t nin = in.nin, nout = in.nout, sb = in.sb;
    const size_t nrows = in.nrows, pos = in.pos;
    const bool small_block = in.small_block;
    gc_label *slab = in.slab;
    const EvalSkel *rows_from = in.rows_from;
    const uint8_t *buf = in.buf;
    std::vector<uint32_t> &wr_ids = e->wr_ids;
    gc_ctx *ctx = e->ctx;
    {
        int rcq = close_group(*e);
        if (rcq != GC_OK) return rcq;
        if (e->deep.n_inflight) {  // a pass on the ctx stream: behind every deep block in flight (DeepLanes)
            e->deep.poll();
            std::lock_guard<std::mutex> lk(ctx->mu);
            GC_HIP(e->deep.wait_all(ctx->stream));
        }
        {  // ... and later deep blocks must see what it reads and writes
            e->win.ensure(e->store.host.size());
            e->win.mark_pass(WireSet{e->io_host.data(), nin, wr_ids.data(), nout});
        }
    }
    gc_circ *circ = ent->circ;
    uint32_t *d_io = nullptr;
    const gc::StoreXchg *d_xchg = nullptr;
    gc_batch *b = nullptr;
    if (rows_from) {  // (a matched small block without a one-workgroup plan: rare — its rows into the scratch after all)
        rows_from->copy_rows(buf, slab);
        rows_from = nullptr;
    }
    const gc_label *slab_arg = slab;
    if (!small_block) {
        // the batch (its table buffer) first: not the one of the block before (held), so its pass may still be running
        // while this block's rows are copied in
        int rcb = gc_pass_batch(circ, &b);
        if (rcb != GC_OK) return rcb;
        slab_arg = nullptr;
    }
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        hipError_t er = hipSetDevice(ctx->device);
        int rcs = er == hipSuccess ? e->store.flush(ctx) : GC_E_HIP;
        const size_t nio = e->io_host.size();
        const size_t x_off = (nio + 1) & ~(size_t)1, nio_alloc = x_off + sizeof(gc::StoreXchg) / 4;
        if (rcs != GC_OK) {
        } else if (small_block) {  // (without an LDS plan: rare; the pass is waited for below)
            er = grow(&e->d_io, &e->io_cap, nio);
            if (er == hipSuccess) er = hipMemcpyAsync(e->d_io, e->io_host.data(), nio * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
            d_io = e->d_io;
        } else {
            // this ring entry's pinned staging and device copy (free: slab_ev[sb] was waited for above); rows and wire maps
            // go up on the upload stream, behind the last pass that read this table buffer, and the ctx stream waits for them
            if (e->io_pin_cap[sb] < nio_alloc) {
                uint8_t *p = (uint8_t *)e->io_pin[sb];
                size_t cap = e->io_pin_cap[sb] * sizeof(uint32_t);
                er = grow_pin(ctx, &p, &cap, nio_alloc * sizeof(uint32_t));
                e->io_pin[sb] = (uint32_t *)p;
                e->io_pin_cap[sb] = cap / sizeof(uint32_t);
            }
            if (er == hipSuccess) er = grow(&e->io_dev[sb], &e->io_dev_cap[sb], nio_alloc);
            if (er == hipSuccess && !e->up_stream) er = hipStreamCreateWithFlags(&e->up_stream, hipStreamNonBlocking);
            if (er == hipSuccess && !e->up_ev[sb]) er = hipEventCreateWithFlags(&e->up_ev[sb], hipEventDisableTiming);
            for (uint32_t i = 0; i < gc_stream_eval::kEvalRing && er == hipSuccess; i++)
                if (e->ring_batch[i] == b && i != sb && e->slab_ev[i]) er = hipStreamWaitEvent(e->up_stream, e->slab_ev[i], 0);
            if (er == hipSuccess && nrows)
                er = hipMemcpyAsync(b->d_T, slab, nrows * sizeof(gc_label), hipMemcpyHostToDevice, e->up_stream);
            if (er == hipSuccess) {
                std::memcpy(e->io_pin[sb], e->io_host.data(), nio * sizeof(uint32_t));
                // ... and the pass's label exchange record behind them (a cooperative pass gathers and scatters itself)
                const gc::StoreXchg x = gc_pass_xchg(circ, e->store.d, e->io_dev[sb], e->io_dev[sb] + nin);
                std::memcpy(e->io_pin[sb] + x_off, &x, sizeof x);
                d_xchg = (const gc::StoreXchg *)(e->io_dev[sb] + x_off);
                er = hipMemcpyAsync(e->io_dev[sb], e->io_pin[sb], nio_alloc * sizeof(uint32_t), hipMemcpyHostToDevice, e->up_stream);
            }
            if (er == hipSuccess) er = hipEventRecord(e->up_ev[sb], e->up_stream);
            if (er == hipSuccess) er = hipStreamWaitEvent(ctx->stream, e->up_ev[sb], 0);
            d_io = e->io_dev[sb];
        }
        if (rcs != GC_OK || er != hipSuccess) {
            if (er != hipSuccess) set_error("gc_stream_eval_circuit", er);
            if (b) {
                // a copy into the batch's buffers may be in flight: nothing else may use it before that has run
                (void)hipStreamSynchronize(e->up_stream);
                gc_circ_release_batch(circ, b);
            }
            return rcs != GC_OK ? rcs : er == hipErrorOutOfMemory ? GC_E_NOMEM : GC_E_HIP;
        }
    }
    int rc = gc_pass_dev(circ, true, e->key.data(), e->key.size(), nullptr, e->store.d, d_io, d_io + nin, slab_arg, nrows, &b, d_xchg);

    // the pinned slab (and this entry's buffers) may be overwritten once what was enqueued from it has run: also when the
    // pass failed half-way (the uploads are in flight)
    if (!small_block) {
        (void)hipEventRecord(e->slab_ev[sb], ctx->stream);
        for (auto &rb : e->ring_batch)
            if (rb == b) rb = nullptr;
        e->ring_batch[sb] = b;  // (null when the pass failed: gc_pass_dev has put the batch back)
    } else {
        (void)hipStreamSynchronize(ctx->stream);  // rows in plain host scratch (a small block without an LDS plan: rare)
    }
    if (rc != GC_OK) {
        if (!small_block) (void)hipStreamSynchronize(e->up_stream);
        return rc;
    }
    if (small_block) {
        gc_circ_release_batch(circ, b);
    } else {
        if (e->held) gc_circ_release_batch(e->held_circ, e->held);
        e->held = b;
        e->held_circ = circ;
    }
    for (uint32_t k = 0; k < nout; k++) e->store.on_dev[e->wr_ids[k]] = 1;
    tr.lap("eval: enqueue");
    *consumed = pos;
    return GC_OK;
}

// a small block joins a group of independent blocks — evaluated side by side in one launch sequence —, a deep one takes a lane
// (place_step)
static int eval_queue_block(gc_stream_eval *e, const BlockIn &in, const WireSet &ws, bool is_deep, int follow_lane, StreamTrace &tr,
                            size_t *consumed) {
    CircEntry *ent = in.ent;
    const uint32_t nin = in.nin, nout = in.nout, sb = in.sb;
    const size_t nrows = in.nrows;
    const bool small_block = in.small_block;
    gc_ctx *ctx = e->ctx;
    if (!e->store.dirty.empty()) {
        int rcs = flush_store(*e);
        if (rcs != GC_OK) return rcs;
    }
    // what the block takes of a group: its wire array and its rows — in the upload region and, for a chain, in the arena again
    const size_t wbytes = up256((size_t)ent->job.w_tile * 16);
    const PlaceArgs pa{2 * wbytes + 2 * nrows * 16, &Slot::up_used, small_block, small_block, (size_t)kOpenGroupsMax * 16, eval_slot};
    Placement p;
    int rcp = place_step(*e, ent, ws, in.ngates, is_deep, follow_lane, pa, &p);
    if (rcp != GC_OK) return rcp;
    Slot &g = *e->slots[p.slot];
    // the rows of a block of many gates were parsed into the pinned ring: they go up from there (launch_group); the rows of
    // a block the DEVICE matched are in device memory already: the launch sequence gathers them into the job's table array
    const bool ext_rows = is_deep && !small_block;
    const bool dev_rows = in.d_block != nullptr && !ext_rows;
    const size_t io_bytes = up16(((size_t)nin + nout) * sizeof(uint32_t)), row_bytes = ext_rows || dev_rows ? 0 : up16(nrows * sizeof(gc_label));
    hipError_t er = g.reserve_up(up16(g.up_used) - g.up_used + io_bytes + row_bytes + 16);
    if (er != hipSuccess) {
        set_error("gc_stream_eval_circuit (pinned)", er);
        if (is_deep) g.reset();
        return GC_E_NOMEM;
    }
    JobRec j;
    j.ent = ent;
    j.nin = nin, j.nout = nout;
    g.up_used = up16(g.up_used);
    j.off_io = g.up_used;
    if (nin + nout) std::memcpy(g.h_up + g.up_used, e->io_host.data(), ((size_t)nin + nout) * sizeof(uint32_t));
    g.up_used += io_bytes;
    j.off_rows = g.up_used;
    if (!ext_rows && !dev_rows && nrows) {
        if (in.rows_from) in.rows_from->copy_rows(in.buf, (gc_label *)(g.h_up + g.up_used));
        else std::memcpy(g.h_up + g.up_used, in.slab, nrows * sizeof(gc_label));
    }
    g.up_used += row_bytes;
    j.off_w = g.arena_used;
    g.arena_used += wbytes;
    if (dev_rows) {
        j.d_block = in.d_block, j.d_row_off = in.d_row_off, j.chunk = in.chunk;
        j.off_t = g.arena_used;
        g.arena_used += up256(nrows * sizeof(gc_label));
        g.chunk_refs.push_back(in.chunk);
        evdev_ref(e, in.chunk);
    }
    if (ext_rows) {
        // the rows go up NOW, on the upload stream, from the pinned ring entry into the slot's arena: the entry is free
        // again as soon as that copy has run (on the lane it would wait for the deep blocks queued there, and the parser
        // for the entry)
        j.rows_in_arena = true;
        j.off_t = g.arena_used;
        g.arena_used += up256(nrows * sizeof(gc_label));
        std::lock_guard<std::mutex> lk(ctx->mu);
        er = grow_dev(ctx, &g.d_arena, &g.arena_cap, g.arena_used);
        if (er == hipSuccess && !e->up_stream) er = hipStreamCreateWithFlags(&e->up_stream, hipStreamNonBlocking);
        if (er == hipSuccess && !e->up_ev[sb]) er = hipEventCreateWithFlags(&e->up_ev[sb], hipEventDisableTiming);
        if (er == hipSuccess && nrows)
            er = hipMemcpyAsync(g.d_arena + j.off_t, in.slab, nrows * sizeof(gc_label), hipMemcpyHostToDevice, e->up_stream);
        if (er == hipSuccess) er = hipEventRecord(e->up_ev[sb], e->up_stream);
        (void)hipEventRecord(e->slab_ev[sb], e->up_stream);
        e->ring_batch[sb] = nullptr;
        if (er != hipSuccess) {
            set_error("gc_stream_eval_circuit (rows)", er);
            (void)hipStreamSynchronize(e->up_stream);
            g.reset();
            return er == hipErrorOutOfMemory ? GC_E_NOMEM : GC_E_HIP;
        }
        g.rows_ev = e->up_ev[sb];
    }
    g.lds = std::max(g.lds, ent->lds);
    g.has_or = g.has_or || ent->has_or;
    j.nrows = (uint32_t)nrows;
    queue_step(*e, g, p, j, ws, e->io_host.data() + nin);
    if (is_deep) {
        int rcl = launch_deep(*e, g, p, ws);
        if (rcl != GC_OK) return rcl;
    }
    for (uint32_t k = 0; k < nout; k++) e->store.on_dev[ws.wr[k]] = 1;
    e->prof.lap(StageProf::kMark);
    tr.lap(is_deep ? "eval: launched on a lane" : "eval: queued in group");
    *consumed = in.pos;
    return GC_OK;
}

// The block joins a group / takes a lane / runs as a pass of its own (see the head of stream_garble.cpp)
int eval_schedule(gc_stream_eval *e, const BlockIn &in, size_t *consumed) {
    StreamTrace tr;
    in.ent->last_use = ++e->tick;
    const WireSet ws{e->io_host.data(), in.nin, e->wr_ids.data(), in.nout};
    int follow_lane = -1;  // a short block that depends on a deep block in flight follows it onto its lane
    const bool is_deep = step_is_deep(*e, in.ent, ws, true, in.small_block, &follow_lane);
    e->n_blocks_total++;
    e->prof.lap(StageProf::kOther);
    if (is_deep || (in.small_block && entry_is_small(in.ent))) return eval_queue_block(e, in, ws, is_deep, follow_lane, tr, consumed);
    return eval_big_block(e, in, tr, consumed);
}

namespace {

// the sizes of a block's header, and the store grown to the block's numWires
int check_block_header(gc_stream_eval *e, uint32_t ngates, uint32_t ntmp, uint32_t nwires, size_t len) {
    // The block comes from the peer: bound it before anything is sized by it.  A gate is at least 5 bytes (op + two
    // 16-bit ids), so a header that announces more gates than the bytes can hold is a truncated stream; global wire
    // ids must stay below the numWires of the block's own header (the reference indexes its store with them,
    // stream_evaluator.go:29-96: an id beyond it panics there) and tmp ids below numTmpWires.
    // The header's two sizes are the peer's as well, and both size arrays (the reference's InitCircuit allocates numWires and
    // numTmpWires labels on the spot, stream_evaluator.go:52-59): a block of n gates names at most 3 n wires, so a numTmpWires
    // far beyond that is not a compiler's; the global store is bounded by GC_STREAM_MAX_WIRES (default 2^28 wires = 4 GiB of
    // labels on each side of the bus).  (Before the length test: such a block is refused however many of its bytes are here.)
    if ((uint64_t)ntmp > 64ull * ngates + (1u << 20) || nwires > stream_max_wires()) return GC_E_ARG;
    if ((size_t)ngates > len / 5) return GC_E_ROWS;
    e->store.ensure(nwires);  // InitCircuit(numWires, numTmpWires)
    return GC_OK;
}

// ---- a block seen before, up to its rows and global ids?  Fills b (circuit, sizes, where the rows are), e->io_host, e->wr_ids.
bool match_known_skeleton(gc_stream_eval *e, uint32_t ntmp, uint32_t nwires, size_t len, BlockIn *b) {
    if (!e->use_skels) return false;
    auto it = e->skels.find(((uint64_t)b->ngates << 32) | ntmp);
    if (it == e->skels.end()) return false;
    for (size_t si = 0; si < it->second.size(); si++) {
        const EvalSkel &sk = *it->second[si];
        if (sk.nbytes > len) continue;
        if (!e->pool.match(sk, b->buf, b->small_block ? nullptr : b->slab)) continue;
        // the skeleton's bookkeeping for a block that equals it byte-wise: the ids at their known offsets, in the skeleton's
        // repeat pattern?
        read_global_ids(b->buf, sk.gf_off, &e->gf_ids);
        if (!eval_adopt_ids(e, sk, e->gf_ids.data(), nwires)) continue;
        b->ent = sk.ent, b->nin = sk.nin, b->nout = sk.nout;
        b->nrows = sk.nrows, b->pos = sk.nbytes;
        // (a small block's rows are copied ONCE, into the upload region of the group it joins — eval_queue_block)
        if (b->small_block) b->rows_from = &sk;
        // most recently matched first: the variants of a circuit (which operands have 16-bit ids, which repeat) are
        // tried in that order and the least recently matched one goes when there are too many
        if (si) std::rotate(it->second.begin(), it->second.begin() + (long)si, it->second.begin() + (long)si + 1);
        return true;
    }
    return false;
}

// What gcw::walk_block (stream_wire.h) tells the evaluator about a block it has not seen: the gates as the cache keys them,
// their hash, the rows into the slab, and the block's skeleton recorded on the way (e->rec: compare runs, global id fields).
// (The hooks are forced inline: a first-seen block is parsed on the host's critical path.)
struct EvalSink {
    const uint8_t *buf;
    EvalSkel &rec;
    std::vector<CircKey> &gates;
    gc_label *slab;
    CircuitHash ph;
    size_t nrows = 0, run_start = 0;
    static __forceinline__ uint64_t load_be64(const uint8_t *p) {
        uint64_t v;
        std::memcpy(&v, p, 8);
        return __builtin_bswap64(v);
    }
    __forceinline__ void cut(size_t at, uint32_t skip, uint32_t rows) {  // the compare run ends at `at`: a global id or rows follow
        rec.chunks.push_back(EvalSkel::Chunk{(uint32_t)(at - run_start), (uint16_t)skip, (uint16_t)rows});
        run_start = at + skip + 16u * (size_t)rows;
    }
    __forceinline__ uint32_t global_field(size_t o, bool is_short) {  // the id field at o names a global wire: its field number
        cut(o, is_short ? 2u : 4u, 0);
        rec.gf_off.push_back((uint32_t)o | (is_short ? 0u : 0x80000000u));
        return (uint32_t)rec.gf_off.size() - 1;
    }
    __forceinline__ void gate(uint32_t g, uint32_t in0, uint32_t in1, uint32_t op, bool writes_tmp) {
        gates[g] = CircKey{in0, in1, writes_tmp ? 1u : 0u, op};
        ph.mix(g, gates[g]);
    }
    __forceinline__ void rows(size_t at, uint32_t n) {
        cut(at, 0, n);
        for (uint32_t r = 0; r < n; r++, at += 16) slab[nrows++] = gc_label{load_be64(buf + at), load_be64(buf + at + 8)};
    }
};

// Parse the gate stream (stream_evaluator.go:272-345): e->keys = the block AS PARSED — {in0, in1, writes-a-tmp, op} per gate,
// operands named by the gate that wrote them (bit 31: the k-th distinct input) — which fixes the device circuit completely
// and is what the cache is keyed on (*hash); its wire ids are only worked out when the cache does not know the block
// (load_or_find_circuit).  e->io: the inputs and the global writers; the rows into b->slab.  The refusals are walk_block's.
int parse_new_block(gc_stream_eval *e, uint32_t ntmp, uint32_t nwires, size_t len, BlockIn *b, uint64_t *hash) {
    e->keys.resize(b->ngates);  // (no per-call allocation: a block has ~10^5 gates)
    e->rec.chunks.clear(), e->rec.gf_off.clear();
    EvalSink sink{b->buf, e->rec, e->keys, b->slab, CircuitHash(b->ngates, 0, 0, 0)};
    const int rc = gcw::walk_block(b->buf, len, b->ngates, ntmp, nwires, e->stamps, e->io, sink, &b->pos);
    if (rc != GC_OK) return rc;
    sink.cut(b->pos, 0, 0);
    b->nrows = sink.nrows, b->nin = (uint32_t)e->io.inputs.size(), b->nout = (uint32_t)e->io.writers.size();
    *hash = ((sink.ph.done() ^ b->nin) * CircuitHash::kPrime ^ b->nout) * CircuitHash::kPrime;
    return GC_OK;
}

// the device circuit of the parsed block (e->keys), cached by content
int load_or_find_circuit(gc_stream_eval *e, BlockIn *b, uint64_t h) {
    const uint32_t ngates = b->ngates, nin = b->nin, nout = b->nout, cw = nin + ngates;
    std::vector<CircKey> &gates = e->keys;
    CircEntry *ent = cache_find_keys(e->cache, h, gates, cw, nin, nout);
    if (!ent) {
        if (e->cache_gates + ngates + 1 > e->cache_budget && !e->cache.empty()) {
            // The cache is bounded (the blocks are the peer's data: a stream of ever new circuits must not grow host and
            // device memory without limit; the reference evaluator holds one block).  Least recently used circuits go,
            // with the byte skeletons that point at them; nothing may refer to them any more: launch what is queued and
            // drain the stream first (rare: once per budget's worth of NEW circuits).
            int rcq = close_group(*e);
            if (rcq != GC_OK) return rcq;
            GC_HIP(hipStreamSynchronize(e->ctx->stream));
            e->deep.drain();
            for (auto &sl : e->slots)
                if (sl->kind == Slot::kGroup && sl->launched) sl->reset();
            if (e->held) gc_circ_release_batch(e->held_circ, e->held);  // (back into its circuit's pool before that may go)
            e->held = nullptr;
            for (auto &rb : e->ring_batch) rb = nullptr;
            cache_make_room(e->cache, &e->cache_gates, e->cache_budget, (size_t)ngates + 1, [&](gc_circ *gone) {
                for (auto &kv : e->skels) {
                    auto &v = kv.second;
                    for (size_t i = v.size(); i-- > 0;)
                        if (v[i]->ent && v[i]->ent->circ == gone) {
                            evdev_drop(e, v[i].get());
                            e->skel_bytes -= std::min(e->skel_bytes, v[i]->held());
                            v.erase(v.begin() + (long)i);
                        }
                }
            });
        }
        // wire ids of the device circuit: inputs, then the tmp-writing gates, then the global-writing gates
        int st = GC_OK;
        gcw::ssa_gate_list(gates, nin, nout, [](const CircKey &k) { return k.out != 0; }, &e->id_of, &e->gates);
        gc_circ *nc = gc_circ_load(e->ctx, e->gates.data(), ngates, cw, nin, nout, &st);
        if (!nc) return st;
        ent = cache_put_keys(e->cache, h, nc, gates, cw, nin, nout);
        e->cache_gates += ent->cost;
        ent->eval_form = true;  // (chain fusion: `gates` holds the block as parsed; its ctx-wide identity)
        ent->uid = fuse_register(e->ctx, true, h, ent->gates, cw, nin, nout);
    }
    b->ent = ent;
    return GC_OK;
}

// Input labels are gathered from, output labels scattered into, the device-resident store: nothing waits for the
// GPU, so the parsing of the next block overlaps the evaluation of this one.  Only the LAST gate of the block that
// writes a global wire stores it (streaming.Set in gate order, :346-432: the last write wins).  (Reads the stamps of the
// block's walk: before anything takes a new generation.)
void bind_parsed_wires(gc_stream_eval *e, const BlockIn &b) {
    const uint32_t nin = b.nin, nout = b.nout;
    e->io_host.resize((size_t)nin + nout + 1);
    for (uint32_t i = 0; i < nin; i++) e->io_host[i] = e->io.inputs[i];
    e->wr_ids.resize(nout);
    gcw::live_outputs(e->stamps, e->io, &e->rec.out_live);
    for (uint32_t k = 0; k < nout; k++) {
        const uint32_t idx = e->wr_ids[k] = (uint32_t)e->io.writers[k];
        e->io_host[nin + k] = e->rec.out_live[k] ? idx : 0xffffffffu;
    }
}

// keep the skeleton: the next block of this circuit is matched byte-wise instead of parsed
void record_skeleton(gc_stream_eval *e, uint32_t ntmp, uint32_t nwires, size_t len, const BlockIn &b) {
    constexpr size_t kSkelCap = (size_t)1 << 30;  // beyond 1 GiB of reference blocks every new circuit is parsed each time
    if (!e->use_skels || len >= 0x7fffffffu || e->skel_bytes + 2 * b.pos > kSkelCap) return;
    auto &v = e->skels[((uint64_t)b.ngates << 32) | ntmp];
    // one circuit serialises differently with the widths of the ids it is bound to (per gate: 16-bit ids if all of the
    // gate's are <= 0xffff) and with operands that repeat: an adder of a mixed program shows up in a dozen forms
    if (v.size() >= kSkelVariants) {
        evdev_drop(e, v.back().get());
        e->skel_bytes -= std::min(e->skel_bytes, v.back()->held());
        v.pop_back();
    }
    std::unique_ptr<EvalSkel> sk(new EvalSkel);
    sk->nbytes = b.pos, sk->key = ((uint64_t)b.ngates << 32) | ntmp;
    sk->nrows = (uint32_t)b.nrows, sk->nin = b.nin, sk->nout = b.nout, sk->ent = b.ent;
    sk->bytes.assign(b.buf, b.buf + b.pos);
    sk->build(e->rec.chunks);
    sk->gf_off = e->rec.gf_off;
    sk->in_gf = e->io.in_field, sk->out_gf = e->io.out_field, sk->out_live = e->rec.out_live;
    read_global_ids(b.buf, sk->gf_off, &e->gf_ids);
    if (canon_of(e, e->gf_ids.data(), (uint32_t)sk->gf_off.size(), nwires, nullptr, &sk->gf_canon)) {
        sk->shape_hash();
        e->skel_bytes += sk->held();
        evdev_add(e, sk.get());
        v.insert(v.begin(), std::move(sk));
    }
}

}  // namespace

// One OpCircuit block (gc_stream_eval_circuit; block after block in gc_stream_eval_blocks): bounded, then recognised by its
// byte skeleton or parsed, its circuit found or loaded and its skeleton kept, then scheduled.
int eval_block(gc_stream_eval *e, uint32_t ngates, uint32_t ntmp, uint32_t nwires, const uint8_t *buf, size_t len,
               size_t *consumed) {
    *consumed = 0;
    int rc = check_block_header(e, ngates, ntmp, nwires, len);
    if (rc != GC_OK || ngates == 0) return rc;
    StreamTrace tr;
    BlockIn b{};
    b.ngates = ngates, b.buf = buf;
    rc = eval_rows_buffer(e, ngates, &b.small_block, &b.sb, &b.slab);
    if (rc != GC_OK) return rc;
    tr.lap("eval: row buffer free");
    if (match_known_skeleton(e, ntmp, nwires, len, &b)) {
        e->n_matched++;
        tr.lap("eval: skeleton match");
    } else {
        uint64_t h = 0;
        rc = parse_new_block(e, ntmp, nwires, len, &b, &h);
        if (rc != GC_OK) return rc;
        tr.lap("eval: parse");
        rc = load_or_find_circuit(e, &b, h);
        if (rc != GC_OK) return rc;
        tr.lap("eval: hash + cache");
        bind_parsed_wires(e, b);
        e->n_parsed++;
        record_skeleton(e, ntmp, nwires, len, b);
    }
    return eval_schedule(e, b, consumed);
}

}  // namespace gcs

extern "C" {

int gc_stream_eval_circuit(gc_stream_eval *e, uint32_t ngates, uint32_t ntmp, uint32_t nwires, const uint8_t *buf,
                           size_t len, size_t *consumed) try {
    if (!e || (!buf && len) || !consumed) return GC_E_ARG;
    return eval_block(e, ngates, ntmp, nwires, buf, len, consumed);
} catch (...) {
    return gc::on_exception();
}

int gc_stream_eval_blocks(gc_stream_eval *e, const uint8_t *buf, size_t len, size_t *consumed, uint32_t *nblocks,
                          int *more) try {
    if (!e || (!buf && len) || !consumed) return GC_E_ARG;
    *consumed = 0;
    if (nblocks) *nblocks = 0;
    if (more) *more = 0;
    auto be32 = [](const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; };
    size_t pos = 0;
    uint32_t n = 0;
    int rc = GC_OK;
    bool cut = false;
    // a read buffer of many blocks: the device recognises them (stream_eval_dev.cpp) — what it leaves (a cut-off last block,
    // a block nobody has seen yet that is not all here, another operation) goes through the loop below
    // (the device's turn again behind every block the host had to take: it only stops where it cannot place a block)
    auto device_turn = [&]() {
        size_t used = 0;
        uint32_t nb = 0;
        rc = evdev_blocks(e, buf + pos, len - pos, &used, &nb);
        pos += used, n += nb;
    };
    device_turn();
    while (rc == GC_OK && len - pos >= 20 && be32(buf + pos) == 1 /* OpCircuit, stream_evaluator.go:22-26 */) {
        const uint32_t ngates = be32(buf + pos + 8), ntmp = be32(buf + pos + 12), nwires = be32(buf + pos + 16);
        const uint8_t *body = buf + pos + 20;
        const size_t avail = len - pos - 20;
        // The last block of a buffer is, as a rule, cut off.  Finding that out by parsing it gate by gate until the bytes run
        // out costs more than evaluating a whole block: when every known layout of this (gates, tmp wires) key is longer
        // than what is here and what is here equals the head of one of them, the block is a known one that is not complete.
        // (A NEW layout that is complete in fewer bytes and shares that head is taken for incomplete as well: the caller
        // comes back with more bytes — in a well-formed stream something always follows a block — and it is parsed then.)
        if ((uint64_t)ntmp > 64ull * ngates + (1u << 20) || nwires > stream_max_wires()) {
            rc = GC_E_ARG;  // (eval_block's own test, in front of the look at what is here of the block)
            break;
        }
        auto it = e->use_skels ? e->skels.find(((uint64_t)ngates << 32) | ntmp) : e->skels.end();
        if (it != e->skels.end()) {
            bool fits = false, head = false;
            for (const auto &sk : it->second) fits = fits || sk->nbytes <= avail;
            if (!fits)
                for (const auto &sk : it->second) head = head || skel_simd::same(body, sk->bytes.data(), sk->mask.data(), avail);
            if (head) {
                cut = true;
                break;
            }
        }
        size_t used = 0;
        rc = eval_block(e, ngates, ntmp, nwires, body, avail, &used);
        if (rc != GC_OK) break;
        pos += 20 + used;
        n++;
        device_turn();
    }
    // a block that ends beyond the buffer is not an error of this call: the caller brings more bytes, or knows that none come
    if (rc == GC_E_ROWS) {
        cut = true;
        rc = GC_OK;
    }
    if (rc == GC_OK && pos < len && (len - pos < 4 || (len - pos < 20 && be32(buf + pos) == 1))) cut = true;  // a header cut in two
    if (more && cut) *more = 1;
    *consumed = pos;
    if (nblocks) *nblocks = n;
    return rc;
} catch (...) {
    return gc::on_exception();
}

}  // extern "C"
