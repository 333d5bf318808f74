/*
 * gcengine.h — C ABI of the MI355X garbled-circuit engine (libgcengine.so).
 *
 * This is the drop-in boundary for the hot path of markkurossi/mpc.  The reference is pure
 * Go and has no FFI layer; each entry point below names the exported Go function whose BODY
 * it replaces (the cgo stub a maintainer adds is shown in INTEGRATION.md and go/).
 * Plain C: pointers + sizes only, no callbacks, every function re-entrant.  All pointers
 * are caller-owned and only used for the duration of the call unless stated otherwise.
 *
 * Memory layouts are Go's in-memory structs, so Go slices cross cgo without copies:
 *   gc_label == ot.Label   {D0,D1 uint64}            ot/label.go:28-31
 *   gc_wire  == ot.Wire    {L0,L1 Label}             ot/label.go:18-21
 *   gc_gate  == circuit.Gate (20 bytes)              circuit/circuit.go:260-266
 */
#ifndef GCENGINE_H
#define GCENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gc_label { uint64_t d0, d1; } gc_label;
typedef struct gc_wire { gc_label l0, l1; } gc_wire;
typedef struct gc_gate {
    uint32_t in0, in1, out;
    uint8_t op; /* circuit.Operation: XOR=0 XNOR=1 AND=2 OR=3 INV=4 (circuit.go:25-34) */
    uint8_t pad_[3];
    uint32_t level;
} gc_gate;

enum {
    GC_XOR = 0, GC_XNOR = 1, GC_AND = 2, GC_OR = 3, GC_INV = 4
};

/* status codes; the Go shim maps them to the reference's error values */
enum {
    GC_OK = 0,
    GC_E_KEYSIZE = -1, /* aes.NewCipher: "crypto/aes: invalid key size" (garble.go:260, eval.go:20) */
    GC_E_RAND = -2,    /* random stream shorter than R + inputs (io.Reader error, garble.go:253,272) */
    GC_E_GATE = -3,    /* "invalid gate type" / "invalid operation" (garble.go:326, eval.go:43) */
    GC_E_ROWS = -4,    /* "corrupted circuit": table shorter than the gates need (eval.go:54-56,86-89) */
    GC_E_ARG = -5,     /* NULL / size mismatch */
    GC_E_HIP = -6,     /* HIP runtime failure (no device, launch error); see gc_last_error() */
    GC_E_NOMEM = -7,   /* device or host allocation failed */
    GC_E_WIRE = -8,    /* gate reads a wire that no input/gate has written, or wire id >= nwires */
    GC_E_POINT = -9,   /* ot.ErrPointNotOnCurve: "ot: point not on curve" (co_helpers.go:17, :179-188) */
    GC_E_BUSY = -10    /* gc_stream_batch_out_garble: every output window is sealed or handed out; nothing has happened */
};

const char *gc_strerror(int status);
/* thread-local detail of the last GC_E_HIP / GC_E_NOMEM on this thread ("" if none) */
const char *gc_last_error(void);
/* ABI version of this header (checked by the bindings).  2: + gc_dev_* (device memory for hosts without a HIP
 * allocator), gc_rot_* (ot/rot.go), gc_stream_garble_flush / gc_stream_stats / gc_stream_intern / gc_stream_garble_begin_h and up
 * to 4 096 circuits in flight per stream (step groups); every v1 entry point is unchanged. */
#define GC_ABI_VERSION 2
int gc_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Circuit plan — host-only "compile" of a gate list (no GPU needed).
 * Replaces nothing in the reference; it is the levelised re-encoding the device needs
 * (reference analogue: Circuit.AssignLevels, circuit/circuit.go:206-254, TargetYao).
 * Gates are renamed to single-assignment slots, bucketed by dependency level, and given the
 * tweak / table-row prefix sums of the reference's serial loop (garble.go:357-359,419-420,
 * 451-452 and :199-211) so that level-parallel execution is bit-identical to it.
 * ------------------------------------------------------------------------------------------ */
typedef struct gc_plan gc_plan;

typedef struct gc_plan_info {
    uint32_t ngates, nwires, ninputs, noutputs;
    uint32_t nlevels;   /* == Stats[NumLevels] of AssignLevels(TargetYao) */
    uint32_t max_width; /* == Stats[MaxWidth] */
    uint32_t slab_rows; /* table labels per instance: AND 2, OR 3, INV 1 */
    uint32_t n_xor, n_xnor, n_and, n_or, n_inv;
    uint32_t nslots;    /* device wire slots = ninputs + ngates */
    uint32_t n_steps;   /* dependency levels = launches per pass of schedule 0 */
    uint32_t n_hash_phases; /* fused schedule: steps that hash (non-free depth of the circuit) */
    uint32_t n_fused_steps; /* fused schedule: hash phases + XOR sub-levels */
    uint32_t n_lds_slots;   /* fused schedule: peak number of live wire labels (0xffffffff: > 65534) */
    /* flattened fused schedule: every NEEDED XOR output is one XOR over a list of earlier labels */
    uint32_t n_flat_slots;  /* peak live labels + the zero slot (0xffffffff: not available) */
    uint32_t n_flat_outs;   /* XOR outputs that are materialised (of n_xor + n_xnor gates) */
    uint32_t n_flat_terms;  /* labels read by them in total */
    uint32_t n_flat_steps;  /* hash phases + XOR rounds = workgroup barriers per pass */
    uint32_t n_flat_units;  /* staging units */
} gc_plan_info;

gc_plan *gc_plan_create(const gc_gate *gates, uint32_t ngates, uint32_t nwires, uint32_t ninputs,
                        uint32_t noutputs, int *status);
/* The plan a CHAIN of streamed circuits runs on when the streaming engine fuses them into one job (round 5, chain fusion:
 * gc_stream_fuse_stats below; mpc_amd/csrc/stream_fuse.cpp).  Step k has gates[k][0 .. ngates[k]) in its own wire ids —
 * inputs [0, nin[k]), outputs the last nout[k] wires — and wiring[k][i] says where its input i comes from: 0xffffffff = the
 * stream's wire store, else (m << 24 | j) = output j of the earlier step m (wiring[0] may be NULL: all from the store).  The
 * merged circuit reads the store inputs in step order, its outputs are every step's outputs in step order, the hash tweak
 * starts over at every step (circuit/stream_garble.go:174) and the table rows count through.  Host only; the introspection
 * calls below apply (gc_plan_describe: gate k of step s is gate first_gate_of_step[s] + k of the merged list). */
gc_plan *gc_plan_create_chain(const gc_gate *const *gates, const uint32_t *ngates, const uint32_t *nwires, const uint32_t *nin,
                              const uint32_t *nout, const uint32_t *const *wiring, uint32_t nsteps, int *status);
void gc_plan_free(gc_plan *);
int gc_plan_get_info(const gc_plan *, gc_plan_info *out);
/* introspection used by the parity tests (arrays sized by the caller):
 *  level_of_gate[ngates]  reference gate.Level for every gate (original order)
 *  tweak_of_gate[ngates]  value of `id` when the serial loop reaches the gate
 *  row_of_gate[ngates+1]  first slab row of the gate (== Garbled.Gates[i] offset into the slab)
 *  slot_of_gate[ngates]   device wire slot written by the gate
 * any pointer may be NULL */
/* Host-side self-check of the flattened fused schedule (no GPU involved): evaluates the circuit on plaintext bits by
 * walking the exact unit program, LDS slot assignment, part joins and global stores the fused kernels execute, with
 * their parallel semantics.  in_bits[ninputs], out_bits[noutputs] (one byte per bit).  GC_E_WIRE: a slot was read
 * before it was written; GC_E_ARG: no flattened schedule / malformed items. */
int gc_plan_simulate(const gc_plan *, const uint8_t *in_bits, uint8_t *out_bits);
int gc_plan_describe(const gc_plan *, uint32_t *level_of_gate, uint32_t *tweak_of_gate,
                     uint32_t *row_of_gate, uint32_t *slot_of_gate);
/* 64-bit fingerprint of the device program of the plan (level steps, hash-phase schedule, flattened unit program and LDS
 * slots): equal fingerprints = the same work launched for this circuit.  bench.py ties PMC counters to it (round 6). */
int gc_plan_fingerprint(const gc_plan *, uint64_t *fp);
/* The two figures of the flattened schedule that fix a batch's tile and LDS image beside n_flat_slots (host only, for tests
 * that predict them): unit_stride16 = uint4 per LDS stage buffer (the largest unit), max_parts = the largest number of
 * lanes one XOR list is spread over (1, 2 or 4).  Either pointer may be NULL.  GC_E_ARG: no flattened schedule. */
int gc_plan_flat_geometry(const gc_plan *, uint32_t *unit_stride16, uint32_t *max_parts);

/* ------------------------------------------------------------------------------------------
 * Device context + circuit
 * ------------------------------------------------------------------------------------------ */
typedef struct gc_ctx gc_ctx;   /* one HIP device + one stream; create one per goroutine/thread for concurrency */
typedef struct gc_circ gc_circ; /* a plan uploaded to a device; immutable, shareable between threads */

int gc_device_count(void);
gc_ctx *gc_ctx_create(int device, int *status);
void gc_ctx_destroy(gc_ctx *);
int gc_ctx_sync(gc_ctx *);
/* ONE instance of a wide circuit (a big streamed step) runs as one launch of 32 workgroups that meet at a barrier between
 * levels; their wait is bounded, and a pass that lost a workgroup is done again on the device, on the same stream, before
 * anything that follows it (so no call fails and no result differs: (*Streaming).Garble of the reference never fails
 * spuriously, circuit/stream_garble.go:161-192) — it costs time, and the ctx keeps to one launch per level from then on.
 * state: 0 not used yet, 1 in use, -1 off (GC_NO_COOP, the self-test failed, or after a timeout); timeouts: passes that were
 * done again.  Either pointer may be NULL.  (GC_COOP_FORCE_TIMEOUT=n makes the n-th pass of every ctx lose a workgroup.) */
int gc_ctx_coop_stats(gc_ctx *, int *state, uint64_t *timeouts);
/* which device the ctx really sits on: its PCI bus id as text ("0000:75:00.0", hipDeviceGetPCIBusId) — a multi-GPU launcher
 * that hands every rank its own HIP_VISIBLE_DEVICES shows each process ONE device, number 0; the bus id tells the ranks'
 * devices apart (bench.py --gpus N records it per rank in its config4 block).  len >= 16. */
int gc_ctx_pci_bus_id(gc_ctx *, char *buf, size_t len);
/* the ctx's HIP stream as an opaque pointer (hipStream_t) for callers that enqueue their own work */
void *gc_ctx_stream(gc_ctx *);

/* Pipeline graphs (hipGraph): record a sequence of DEVICE-RESIDENT calls on this ctx (gc_batch_garble,
 * _select_inputs, _eval, _decode, _egress_tables, gc_cot_*_dev, ...; same pointers every time) once, then replay it
 * with a single launch — removes the host launch latency between the five-odd kernels of a step.
 * Between begin and end nothing executes; host-buffer calls (gc_garble, gc_eval, read_*, ...), changes of key,
 * schedule or batch geometry, and gc_iknp_*_dev (their column streams advance with every call: the position cannot be
 * baked into a graph; they return GC_E_ARG) are not allowed inside a capture; gc_batch_last_ms is not updated by replays. */
typedef struct gc_graph gc_graph;
int gc_ctx_capture_begin(gc_ctx *);
int gc_ctx_capture_end(gc_ctx *, gc_graph **out);
int gc_graph_launch(gc_graph *);
void gc_graph_free(gc_graph *);

gc_circ *gc_circ_load(gc_ctx *, const gc_gate *gates, uint32_t ngates, uint32_t nwires,
                      uint32_t ninputs, uint32_t noutputs, int *status);
void gc_circ_free(gc_circ *);
const gc_plan *gc_circ_plan(const gc_circ *);
/* execution schedule used by gc_garble / gc_eval on this circuit (see gc_batch_set_schedule):
 * 0 = one launch per dependency level, 1 = fused single launch (default), 2 = fused, single-phase kernel.
 * Bit-identical results. */
int gc_circ_set_schedule(gc_circ *, int schedule);

/* ------------------------------------------------------------------------------------------
 * Host-buffer API — bodies of the reference's per-call entry points, plus a batch dimension
 * (instance-major: instance i's data follows instance i-1's).
 * ------------------------------------------------------------------------------------------ */

/* Replaces (c *Circuit) Garble(rand io.Reader, key []byte) (*Garbled, error)   circuit/garble.go:248
 *  key/keylen  16, 24 or 32 bytes
 *  rnd         per instance the bytes the io.Reader would deliver, in consumption order:
 *              R (16 B; S bit is forced on, garble.go:258) then one L0 per input wire
 *              (garble.go:271-278): stride 16*(1+ninputs); rndlen >= batch*stride or GC_E_RAND
 *  r_out       [batch]                    Garbled.R
 *  wires_out   [batch][nwires] or NULL    Garbled.Wires (both labels, original wire ids)
 *  io_out      [batch][ninputs+noutputs] or NULL: Wires[0:ninputs] then Wires[nwires-noutputs:]
 *              — the only ranges the reference's callers read (garbler.go:87,132,153)
 *  slab_out    [batch][slab_rows]         the dense table slab, gate order (Garbled.Gates[i] =
 *              slab[row_of_gate[i] : row_of_gate[i+1]])                                     */
int gc_garble(gc_circ *, const uint8_t *key, size_t keylen, const uint8_t *rnd, size_t rndlen,
              uint32_t batch, gc_label *r_out, gc_wire *wires_out, gc_wire *io_out, gc_label *slab_out);

/* Replaces (c *Circuit) Eval(key []byte, wires []ot.Label, garbled [][]ot.Label) error   circuit/eval.go:17
 *  wires_inout [batch][nwires] or NULL: inputs pre-filled at [0,ninputs); all wires written in place
 *  inputs      [batch][ninputs]  used when wires_inout is NULL
 *  slab        [batch][slab_rows], slab_rows_given must equal the plan's slab_rows (else GC_E_ROWS)
 *  out_labels  [batch][noutputs] or NULL: wires[nwires-noutputs:]                              */
int gc_eval(gc_circ *, const uint8_t *key, size_t keylen, uint32_t batch, gc_label *wires_inout,
            const gc_label *inputs, const gc_label *slab, size_t slab_rows_given, gc_label *out_labels);

/* The same two calls speaking the wire format of the 2-party driver (SURVEY §8f row 1 on the host-buffer API):
 * gc_garble_wire = Circuit.Garble + the table send loop of circuit.Garbler (circuit/garbler.go:53-82) — wire_out
 * receives, per instance and `stride` bytes apart (multiple of 4, >= gc_tables_wire_bytes()),
 *   BE32(#gates) | per gate BE32(#rows) rows x BE(D0)||BE(D1)
 * i.e. exactly what the SendUint32 / SendLabel loop would put on the connection: the shim hands it to conn in one
 * piece.  gc_eval_wire = the receive loop of circuit.Evaluator (circuit/evaluator.go:40-66) + Circuit.Eval; *bad
 * counts headers that do not match the circuit ("wrong number of gates", evaluator.go:44-47; row counts that Eval
 * rejects, eval.go:54-56,86-89): non-zero returns GC_E_ROWS and nothing is evaluated. */
int gc_garble_wire(gc_circ *, const uint8_t *key, size_t keylen, const uint8_t *rnd, size_t rndlen, uint32_t batch,
                   gc_label *r_out, gc_wire *io_out, uint8_t *wire_out, size_t stride);
int gc_eval_wire(gc_circ *, const uint8_t *key, size_t keylen, uint32_t batch, const gc_label *inputs,
                 const uint8_t *wire_in, size_t stride, gc_label *out_labels, uint32_t *bad);

/* Pinned host memory for the two calls above (additive; the reference pools its scratch on the Go heap,
 * garble.go:195-225 — the shim backs that pool with gc_host_alloc instead).  When slab_out / wires_out / io_out /
 * slab / wires_inout point into pinned memory the calls DMA straight from / into the caller's pages (~57 GB/s instead
 * of 37 / 46 GB/s through the runtime's bounce buffers) and overlap the DMA of one chunk of instances with the
 * layout transpose of the next.  Pageable pointers keep working unchanged.
 *  gc_host_alloc      hipHostMalloc (portable: usable with every device); NULL on failure
 *  gc_host_register   pins an existing range (page-aligned ranges register fastest); undo with gc_host_unregister
 *                     before the memory is freed */
void *gc_host_alloc(size_t bytes);
void gc_host_free(void *);
int gc_host_register(void *p, size_t bytes);
int gc_host_unregister(void *p);
int gc_host_is_pinned(const void *p);

/* Device memory for the device-resident API below (additive; the reference has no device).  A Go host owns no HIP
 * allocator, so the library hands out, fills and reads back the buffers that gc_batch_* (d_rnd, d_bits, d_bits_out,
 * d_mismatch, ...), the *_dev OT calls and gc_comm_allgather take: with these five calls the whole device-resident
 * pipeline is reachable through this header alone (go/circuit/batch_hip.go; tests/cpp/test_device_pipeline.cpp).
 * All of them run on the ctx's device and order themselves on the ctx stream:
 *  gc_dev_alloc     hipMalloc; NULL + *status (GC_E_NOMEM / GC_E_HIP) on failure; contents undefined
 *  gc_dev_free      waits for the ctx stream (kernels may still use the buffer), then frees; NULL is a no-op
 *  gc_dev_upload    host -> device behind everything queued on the ctx stream; returns when `src` may be reused
 *                   (cgo must not leave Go memory referenced after the call)
 *  gc_dev_download  device -> host after everything queued on the ctx stream; returns with the bytes in `dst`
 *  gc_dev_memset    stream-ordered fill, asynchronous
 *  gc_dev_copy      device -> device on the ctx stream, asynchronous (e.g. slot j of an accumulator)
 * d + offset arithmetic on the returned pointers is the caller's (they are plain device addresses). */
void *gc_dev_alloc(gc_ctx *, size_t bytes, int *status);
void gc_dev_free(gc_ctx *, void *d);
int gc_dev_upload(gc_ctx *, void *d_dst, const void *src, size_t bytes);
int gc_dev_download(gc_ctx *, void *dst, const void *d_src, size_t bytes);
int gc_dev_memset(gc_ctx *, void *d, int byte_value, size_t bytes);
int gc_dev_copy(gc_ctx *, void *d_dst, const void *d_src, size_t bytes);

/* Garble ONE instance whose R and input-wire L0 labels are given instead of drawn from a random
 * stream (what Streaming.Garble needs: the inputs of an SSA-step circuit are wires garbled earlier).
 *  r        the stream's R (S bit already set)        inputs   [ninputs] L0 labels
 *  slab_out [slab_rows]                               out_l0   [noutputs] L0 of the output wires */
int gc_garble_labels(gc_circ *, const uint8_t *key, size_t keylen, const gc_label *r, const gc_label *inputs,
                     gc_label *slab_out, gc_label *out_l0);

/* ------------------------------------------------------------------------------------------
 * Streaming garbler (config 5) — circuit/stream_garble.go
 * ------------------------------------------------------------------------------------------ */
typedef struct gc_stream gc_stream;
/* Replaces NewStreaming(cfg, key, inputs, conn)   circuit/stream_garble.go:41-75
 *  rnd = the bytes cfg.GetRandom() would deliver: R (16 B) then one L0 per entry of inputs[] */
gc_stream *gc_stream_create(gc_ctx *, const uint8_t *key, size_t keylen, const uint8_t *rnd, size_t rndlen,
                            const uint32_t *inputs, uint32_t ninputs, int *status);
void gc_stream_free(gc_stream *);
/* Replaces (*Streaming).GetInput(w)   stream_garble.go:117-119 */
int gc_stream_get_wire(gc_stream *, uint32_t w, gc_wire *out);
/* Replaces (*Streaming).Garble(c, in, out)   stream_garble.go:161-192: garbles the circuit (tweak restarts
 * at 0, :174) and appends the serialised gates — op|flags, 16/32-bit wire indexes, table rows, exactly as
 * :391-446 writes them into conn.WriteBuf — to buf.  *written = bytes needed; GC_E_ARG if cap is smaller.
 * in[] / out[] may overlap (output wires that are input wires are resolved through in[] and never set, as in
 * :131-157), and may name the same GLOBAL wire (in-place update): a gate that reads such an input after the gate that
 * set the output sees the new label, as the reference's per-gate stream.wire() look-up does.  Deliberate differences,
 * none reachable from compiled programs: a gate that writes an input-mapped wire is rejected (GC_E_ARG); a gate that
 * reads an output-range wire before any gate of the circuit wrote it is rejected (GC_E_WIRE; the reference would read
 * the global store's current label); a global wire that was never set reads as (L0, L1) = (0, R) — the reference's
 * zero-initialised store gives (0, 0); the engine never stores L1 (always L0 ^ R). */
int gc_stream_garble(gc_stream *, const gc_gate *gates, uint32_t ngates, uint32_t nwires, const uint32_t *in,
                     uint32_t nin, const uint32_t *out, uint32_t nout, uint8_t *buf, size_t cap, size_t *written);

/* The same call in two halves (additive): _begin QUEUES one circuit — input labels gathered from the stream's wire store
 * (which lives in HBM), garbling, output labels scattered back, serialisation — and returns without waiting for the GPU;
 * _finish hands out the bytes of the OLDEST circuit in flight.  Calling begin(k + 1 ... k + d) before finish(k) overlaps
 * the host's share of a step (content hash, plan look-up, launches) with the GPU's share of the steps before, and gives
 * the engine STEP-LEVEL PARALLELISM: queued circuits of at most 32 768 gates (8 192 if their levels are wide) that share no global wire through in[] /
 * out[] (no read-after-write, write-after-write, write-after-read) are garbled side by side by ONE launch sequence —
 * one workgroup per circuit — the way independent SSA instructions of a compiled program (compiler/ssa/streamer.go:
 * 412-524 garbles one circuit per instruction) allow; a circuit that depends on a queued one starts the next group, and
 * larger circuits keep a launch sequence of their own.  The bytes still leave in program order, so a driver writes them
 * to the connection exactly as before.  At most 4 096 circuits in flight (a further _begin returns GC_E_ARG);
 * gc_stream_garble is _begin + _finish and needs nothing in flight; gc_stream_get_wire launches what is queued and
 * waits for it.  _finish launches the group of the oldest circuit if it is still open; gc_stream_garble_flush does the
 * same without waiting (a driver that wants the GPU to start before it has queued a whole window).  If cap is too small
 * _finish returns GC_E_ARG with *written = the size needed; that circuit has been garbled (its outputs are set) and its
 * bytes are dropped. */
int gc_stream_garble_begin(gc_stream *, const gc_gate *gates, uint32_t ngates, uint32_t nwires, const uint32_t *in,
                           uint32_t nin, const uint32_t *out, uint32_t nout);
int gc_stream_garble_finish(gc_stream *, uint8_t *buf, size_t cap, size_t *written);
/* The same without the copy (additive): *bytes points into the engine's pinned staging and stays valid until the next
 * gc_stream_garble_finish / _finish_view / gc_stream_free on this stream — for a caller that moves the bytes on itself
 * (the Go shim copies them into conn.WriteBuf, stream_garble.go:177-185: one copy instead of two; on a program of 13 000-gate
 * multipliers the copy out of the staging was most of the host's time per step). */
int gc_stream_garble_finish_view(gc_stream *, const uint8_t **bytes, size_t *len);
/* gc_stream_garble_finish with the copy DEFERRED (additive, round 5): *written is known when the call returns, the bytes are in
 * buf[0 .. *written) once gc_stream_garble_copies_wait (or gc_stream_free) has returned — a few threads of the stream do the
 * copying (GC_STREAM_COPY_THREADS, default 3) while the caller's thread queues the next circuits.  For a host that fills a
 * large write buffer of its own: on the Ed25519-shaped program the stream is 22 bytes per gate, so at 8e8 gates/s the copy
 * out of the staging alone is 17 GB/s — more than the one core that also queues 26 000 circuits can move.  buf must stay
 * valid and untouched until the wait; the three kinds of finish may be mixed (every one hands out the OLDEST circuit). */
int gc_stream_garble_finish_async(gc_stream *, uint8_t *buf, size_t cap, size_t *written);
int gc_stream_garble_copies_wait(gc_stream *);
int gc_stream_garble_flush(gc_stream *);
/* A driver garbles the same few circuits over and over (the streamer keeps one compiled circuit per SSA instruction
 * shape: 23 for Ed25519 sign.mpcl, benchmarks.md:698), and gc_stream_garble_begin has to recognise the gate list by
 * content on every call (a hash and a gate-by-gate comparison: most of the host's share of a small step).
 * gc_stream_intern does that ONCE and returns a handle for the stream's lifetime (the Go shim keeps a
 * map[*Circuit]handle; interned circuits are exempt from cache eviction); gc_stream_garble_begin_h is
 * gc_stream_garble_begin for an interned circuit: in[] / out[] have the circuit's ninputs / noutputs entries. */
int gc_stream_intern(gc_stream *, const gc_gate *gates, uint32_t ngates, uint32_t nwires, uint32_t ninputs,
                     uint32_t noutputs, uint32_t *handle);
int gc_stream_garble_begin_h(gc_stream *, uint32_t handle, const uint32_t *in, const uint32_t *out);
/* gives an interned circuit back to the bounded cache (a host that drops a compiled circuit; the Go shim's
 * (*Streaming).Forget(c) does it — an explicit call: the shim's handle map keeps the *Circuit alive, so no finalizer could):
 * the handle is invalid afterwards (GC_E_ARG) and its number may be handed out again */
int gc_stream_release(gc_stream *, uint32_t handle);
/* launch sequences so far: groups of small circuits, circuits that ran in them, circuits with a sequence of their own
 * (any pointer may be NULL) */
int gc_stream_stats(const gc_stream *, uint64_t *groups, uint64_t *grouped_steps, uint64_t *big_steps);
/* Deep lanes (additive).  A step whose one-workgroup pass is long — hundreds of dependent hash phases: a 128- / 256-bit
 * multiplier, a 256- / 512-bit adder, 0.5 - 2 ms on one CU — runs on one of a few extra HIP streams of the ctx, beside the
 * groups of small steps, and is ordered against them by events only where two steps share a wire; the bytes still leave in
 * program order (circuit/stream_garble.go:161-192 is one serial loop: nothing on the wire or in the wire store may differ
 * from it).  deep_steps: steps that ran that way so far (they are also counted as groups of one by gc_stream_stats);
 * lanes: streams in use (0: none — GC_STREAM_DEEP_LANES=0, or no stream of the runtime runs beside the ctx stream: such
 * steps then keep the launch sequence of the big steps).  GC_STREAM_DEEP_LANES (default 3) and GC_STREAM_DEEP_STEPS
 * (barriers per pass from which a step counts as deep, default 300) are read when a ctx / a stream first needs them.
 * Either pointer may be NULL. */
int gc_stream_deep_stats(const gc_stream *, uint64_t *deep_steps, uint32_t *lanes);
/* Chain fusion (round 5; mpc_amd/csrc/stream_fuse.cpp): a queued step whose dependencies among the steps still queued all sit
 * in ONE launch unit is appended to that unit, and the chain — mul -> add -> add -> ... -> carry — runs as one planned job
 * whose gates are scheduled across the step boundaries (a ten-link chain of 64-bit adders: 63 + 9 dependent hash phases
 * instead of 10 x 63).  The hash tweak still starts over at every circuit (circuit/stream_garble.go:174) and the bytes still
 * leave step by step in program order (:385-449): nothing on the wire or in the wire store differs.  fused_units: launch
 * units of more than one step so far; fused_steps: the steps in them; plans_built: merged plans this stream had to build
 * (they are cached per ctx); unfit: units whose merged plan fits no workgroup (their steps ran one launch after the other).
 * GC_STREAM_NO_FUSE in the environment switches the fusion off.  Any pointer may be NULL. */
int gc_stream_fuse_stats(const gc_stream *, uint64_t *fused_units, uint64_t *fused_steps, uint64_t *plans_built, uint64_t *unfit);
/* Units that WAIT inside a launch — an experiment, off unless GC_STREAM_DEPS=1 is in the environment when the stream is
 * created (EXPERIMENTS.md, round 5: on the programs measured it costs more chain fusion than it saves launches).  A queued step
 * that conflicts with steps of an open group — and cannot be fused into one unit with them: it conflicts with several units,
 * or is too large for a chain — then still joins that group: its workgroup waits, on the device, for the done-flags of exactly
 * the units it conflicts with (mpc_amd/csrc/kernels.h: d_sync) instead of the whole step waiting for the whole group in a
 * later launch.  Program order per wire is what the reference's serial loop gives (stream_garble.go:131-157): a reader runs
 * behind the writer it names, a writer behind the earlier readers and writers of its wire.  waiting_units: such units so far
 * (0 when the experiment is off). */
int gc_stream_wait_stats(const gc_stream *, uint64_t *waiting_units);

/* Streaming evaluator: the store of circuit.StreamEval (stream_evaluator.go:29-96) and the
 * per-gate loop of StreamEvaluator for ONE OpCircuit block (stream_evaluator.go:270-432).  The host driver keeps
 * reading the framing (OpCircuit header: step, numGates, numTmpWires, numWires) and hands the gate bytes over;
 * the gates are parsed back into a circuit, levelised and evaluated with the same kernels as Circuit.Eval.  The wire
 * store lives in HBM: gc_stream_eval_circuit returns once the block is parsed and its kernels are enqueued (the parsing of
 * the next block overlaps them) — or, for blocks of at most 32 768 gates, QUEUED: consecutive small blocks that share no
 * global wire are evaluated side by side by one launch sequence, as on the garbler's side; gc_stream_eval_get_wire
 * launches what is queued and waits for it.  The per-stream circuit cache is bounded (GC_STREAM_CACHE_GATES gates,
 * default 8 Mi; least recently used circuits and their byte skeletons go first): the blocks are the peer's data. */
typedef struct gc_stream_eval gc_stream_eval;
gc_stream_eval *gc_stream_eval_create(gc_ctx *, const uint8_t *key, size_t keylen, int *status);
void gc_stream_eval_free(gc_stream_eval *);
int gc_stream_eval_set_wire(gc_stream_eval *, uint32_t w, const gc_label *l); /* input labels (OT results etc.) */
int gc_stream_eval_get_wire(gc_stream_eval *, uint32_t w, gc_label *l);       /* OpReturn / OpResult reads */
/* *consumed = bytes of buf used by the ngates gates; GC_E_GATE "invalid operation", GC_E_ROWS truncated stream (also:
 * more gates announced than len / 5 bytes can hold), GC_E_ARG a tmp wire read before this block wrote it (tmp wires are
 * private to their OpCircuit block), a tmp id >= ntmp or a global wire id >= nwires, and header sizes no compiler
 * produces: ntmp > 64 ngates + 2^20, nwires > GC_STREAM_MAX_WIRES (default 2^28) — both size arrays.  The block is the peer's data:
 * nothing is sized by it before these checks, and allocation failures come back as GC_E_NOMEM. */
int gc_stream_eval_circuit(gc_stream_eval *, uint32_t ngates, uint32_t ntmp, uint32_t nwires, const uint8_t *buf,
                           size_t len, size_t *consumed);
/* The framing loop of StreamEvaluator around that (stream_evaluator.go:226-270) for as many WHOLE OpCircuit blocks as buf holds
 * (additive).  buf starts at an operation word: 4 bytes big-endian, OpCircuit = 1, then step, numGates, numTmpWires, numWires
 * (compiler/ssa/streamer.go:679-693), then the gates.  Block after block is evaluated as gc_stream_eval_circuit would; the call
 * stops in front of the first operation that is not OpCircuit (OpReturn: the caller reads the result wires) and in front of
 * a block that ends beyond len — then *more = 1: bring more bytes and call again from *consumed, or, if none can come, the
 * stream is truncated (what gc_stream_eval_circuit reports as GC_E_ROWS).  *consumed = bytes used, *nblocks = blocks
 * evaluated (both also when an error is returned: the blocks before the bad one are done); nblocks / more may be NULL.
 * A Go host hands over conn.ReadBuf[ReadStart:ReadEnd] (p2p/protocol.go:29-35, 1 MiB) instead of collecting one block gate
 * by gate; buf is only read during the call.  (A thread comparing the blocks ahead with their byte skeletons while this one
 * queues the ones before was built and measured: +7 % with the whole stream in one call, -25 % in 1 MiB pieces — the rows
 * then reach the queueing thread from another core's cache — and removed.) */
int gc_stream_eval_blocks(gc_stream_eval *, const uint8_t *buf, size_t len, size_t *consumed, uint32_t *nblocks, int *more);
/* Blocks handed to gc_stream_eval_circuit so far: parsed[0] gate by gate, parsed[1] recognised as a block seen before up
 * to its table rows and the global wires it is bound to (same op / flag bytes and tmp ids at the same offsets, global ids
 * repeating in the same pattern): those are not decoded again.  Either pointer may be NULL.  (GC_STREAM_NO_SKELETON in the
 * environment at gc_stream_eval_create time switches the recognition off: every block is decoded.) */
int gc_stream_eval_stats(const gc_stream_eval *, uint64_t *parsed, uint64_t *matched);
/* the evaluator's counterpart of gc_stream_deep_stats */
int gc_stream_eval_deep_stats(const gc_stream_eval *, uint64_t *deep_blocks, uint32_t *lanes);
/* Device-side match (round 5; mpc_amd/csrc/stream_eval_dev.cpp): gc_stream_eval_blocks sends a read buffer of 64 KiB or more
 * to the GPU as it is — one DMA, straight from the caller's memory when that is pinned (gc_host_alloc / gc_host_register), else
 * through pinned staging — where one workgroup recognises the blocks by their byte skeletons and reads their global wire ids;
 * the table rows are gathered from the device copy by the launch that needs them.  The host reads 20 bytes of header and the
 * ids of a block instead of every byte twice.  blocks: blocks scheduled on a device verdict so far; fallbacks: blocks the device
 * was asked about that the host's matcher / parser took after all (other bytes or another repeat pattern of the ids than any
 * skeleton of the shape has, an id beyond numWires) — counted apart from `blocks`, never among them; blocks the device is not
 * asked about (new, or cut off by the buffer's end) count in neither.  GC_STREAM_NO_DEVICE_MATCH: off.  Pointers may be NULL. */
int gc_stream_eval_dev_stats(const gc_stream_eval *, uint64_t *blocks, uint64_t *fallbacks);
/* the evaluator's counterpart of gc_stream_fuse_stats (its blocks chain exactly as the garbler's steps do) */
int gc_stream_eval_fuse_stats(const gc_stream_eval *, uint64_t *fused_units, uint64_t *fused_blocks, uint64_t *plans_built,
                              uint64_t *unfit);
/* ... and of gc_stream_wait_stats */
int gc_stream_eval_wait_stats(const gc_stream_eval *, uint64_t *waiting_units);

/* ------------------------------------------------------------------------------------------
 * Device-resident batch API — what a Go host pipelining many instances (GarbleBatch/EvalBatch,
 * additive to the reference API) calls; also what bench.py times.  All d_* arguments are
 * DEVICE pointers; calls enqueue on the ctx stream and return without waiting.
 * Device layouts are wire-major / instance-minor so that a wavefront reads 64 consecutive
 * instances of one wire as one 1 KiB coalesced access:
 *   wire labels  uint4 [nslots][bstride]     tables  uint4 [slab_rows][bstride]
 * where bstride = batch rounded up to 64.
 * ------------------------------------------------------------------------------------------ */
typedef struct gc_batch gc_batch;

gc_batch *gc_batch_create(gc_circ *, uint32_t batch, int *status);
void gc_batch_free(gc_batch *);
uint32_t gc_batch_stride(const gc_batch *);
/* geometry the fused schedules chose for this batch: instances per workgroup tile (1 for schedule 0), and
 * whether the live wire labels fit in LDS (otherwise the fused kernel keeps them in HBM) */
uint32_t gc_batch_tile_instances(const gc_batch *);
int gc_batch_wires_in_lds(const gc_batch *);
/* schedule: 0 = one launch per dependency level (the reference's AssignLevels order), labels laid
 *               out [wire][instance];
 *           1 = fused (default): ONE launch per pass, every workgroup owns a tile of instances and
 *               walks all levels with workgroup barriers; labels laid out [tile][wire][instance].  When the
 *               live labels fit in LDS the tile's two halves run one stage apart (one half's XOR chain
 *               hides behind the other half's hashing);
 *           2 = as 1 (same layout) but with the single-phase kernel: every instance of the tile in lock
 *               step (what tiles of one instance use anyway; kept selectable for comparison and tests).
 * Results are bit-identical.  Changing the schedule re-allocates the batch's device arrays. */
int gc_batch_set_schedule(gc_batch *, int schedule);
/* fused schedule only: also write EVERY wire label to the global wire array (needed by
 * gc_batch_read_wires / gc_batch_read_labels; gc_garble / gc_eval switch it on when the caller asks
 * for Garbled.Wires / the full wires slice).  Off by default: only input and output wires are kept. */
int gc_batch_set_store_all(gc_batch *, int on);
/* use a captured hipGraph for the per-level launches (default on) */
int gc_batch_set_graph(gc_batch *, int on);

/* garble all instances: d_rnd = [batch][1+ninputs][16] bytes (same stream as gc_garble) */
int gc_batch_garble(gc_batch *, const uint8_t *key, size_t keylen, const void *d_rnd);
/* evaluator inputs: active label of input wire w of instance i = L0 ^ bit*R, picked on the
 * device from the garbler's state (stands in for "send own labels + OT", garbler.go:85-132);
 * d_bits = u8 [batch][ninputs] */
int gc_batch_select_inputs(gc_batch *evaluator, const gc_batch *garbler, const void *d_bits);
/* evaluator inputs from explicit labels, d_labels = gc_label [batch][ninputs] */
int gc_batch_set_inputs(gc_batch *evaluator, const void *d_labels);
/* evaluate with the tables of `tables` (device layout [slab_rows][bstride]); may be the
 * garbler's batch itself */
int gc_batch_eval(gc_batch *evaluator, const uint8_t *key, size_t keylen, const gc_batch *tables);
/* The same two passes with ONE AES KEY PER INSTANCE: circuit.Garbler draws a fresh key on every call and sends it to the
 * peer (circuit/garbler.go:47-53, 64), so a batch that gathers S concurrent sessions holds S keys.
 * d_keys = u8 [batch][keylen], one AES key per instance (garbler.go:47-53); keylen 16, 24 or 32 for all.  Device-resident
 * like their one-key twins: enqueued on the ctx stream, nothing is waited for; the round keys are expanded ON THE DEVICE
 * as part of the pass, so a captured graph replays with whatever keys the buffer holds at replay time.  Instance i's
 * bytes are those of gc_batch_garble / gc_batch_eval with key i.
 * Scope (gc_batch_keyed_supported: 1 / 0; gc_batch_keyed_path: which kernels): schedule 1, and either the wires in LDS
 * (gc_batch_wires_in_lds) on the flattened kernels with the tile's key table fitting into LDS behind the wire slots (path 1),
 * or the wires in HBM — no LDS plan, one that does not fit, one still pending — on the level-walking keyed kernels (path
 * 2), which leave every wire (gc_batch_read_wires).  A batch whose wires are in LDS but whose key table does not fit is
 * refused unless gc_batch_set_keyed_path(b, 2) sends it to path 2.  Not built: schedules 0 and 2, the cooperative and
 * level-launch one-instance forms, the streaming jobs, the host-buffer calls gc_garble / gc_eval.
 * GC_E_KEYSIZE for any other keylen, GC_E_ARG for a NULL pointer, GC_E_ARG with a gc_last_error() text for a batch
 * outside the scope. */
int gc_batch_garble_keyed(gc_batch *, const void *d_keys, size_t keylen, const void *d_rnd);
int gc_batch_eval_keyed(gc_batch *evaluator, const void *d_keys, size_t keylen, const gc_batch *tables);
int gc_batch_keyed_supported(const gc_batch *);
/* which kernels the keyed calls run on this batch now: 0 none (they return GC_E_ARG), 1 flattened with the wires in LDS,
 * 2 level-walking with the wires in HBM */
int gc_batch_keyed_path(const gc_batch *);
/* 0 (default): the rule above.  2: path 2 for every schedule-1 batch, also one whose wires are in LDS under the one-key
 * kernels (its arrays hold every wire slot whatever the kernel) — the way to serve a batch whose key table does not fit,
 * at the HBM-wire kernels' cost.  Other values, schedule 0 / 2: GC_E_ARG.  Graphs captured before stay valid for what
 * they captured. */
int gc_batch_set_keyed_path(gc_batch *, int path);
/* Path 2 has two forms with the same bytes, one launch each (gc_batch_last_launches 1), nothing reaching the host: the plain
 * form walks a level in passes of the whole workgroup; the split form gives the hashed and the free gates of a level wider than
 * 1 024 column lanes to different waves.  form 0 (default): the rule — the split form when the plan has such levels in that
 * pass's lane count at the batch's tile width and they average three passes of 1 024 lanes or more (below that the split
 * form measured no faster: DESIGN.md §15), the plain form otherwise.  1: always plain.  2: always split (a narrow circuit
 * then runs the split kernels' single-pass branch throughout).  Other values: GC_E_ARG.  Holds for any path-2 pass of the
 * batch, forced or natural.  Graphs captured before stay valid for what they captured. */
int gc_batch_set_keyed_hbm_form(gc_batch *, int form);
/* what the keyed calls would run now: 0 when gc_batch_keyed_path is not 2, else 1 (plain) or 2 (split); under the rule the
 * answer is the garbler's (an evaluation splits only where its own, smaller lane count has a wide level) */
int gc_batch_keyed_hbm_form(const gc_batch *);
/* developer aid: hash waves of every split level of the garbler's / the evaluator's pass, 1 .. 15, still capped by the lanes
 * the level has; 0 = the rule.  Values above 15: GC_E_ARG */
int gc_batch_debug_keyed_hbm_hash_waves(gc_batch *, uint32_t garble_h, uint32_t eval_h);
/* BitFromLabel (circuit/helpers.go:18-28) for every output wire: d_bits_out = u8 [batch][noutputs];
 * *d_mismatch (u32, device) counts labels that match neither L0 nor L1 */
int gc_batch_decode(const gc_batch *garbler, const gc_batch *evaluator, void *d_bits_out, void *d_mismatch);

/* read-backs (synchronous; host pointers) */
int gc_batch_read_r(gc_batch *, gc_label *r_out);                     /* [batch] */
int gc_batch_read_slab(gc_batch *, gc_label *slab_out);               /* [batch][slab_rows] (reference order) */
int gc_batch_read_wires(gc_batch *, gc_wire *wires_out);              /* garbler: [batch][nwires]; needs store_all */
int gc_batch_read_labels(gc_batch *, gc_label *labels_out);           /* evaluator: [batch][nwires]; needs store_all */
int gc_batch_read_outputs(gc_batch *, gc_label *out);                 /* [batch][noutputs] active/L0 labels */
int gc_batch_write_slab(gc_batch *, const gc_label *slab);            /* host [batch][slab_rows] -> device layout */
/* raw device pointers (for RCCL gathers / the caller's own kernels) */
void *gc_batch_dev_wires(gc_batch *);
void *gc_batch_dev_slab(gc_batch *);
void *gc_batch_dev_r(gc_batch *);
/* output-wire labels gathered into a dense device buffer gc_label [noutputs][bstride] */
int gc_batch_gather_outputs(gc_batch *, void *d_out);
/* Device-side hand-over of input labels through an OT (garbler.go:102-132): the garbler's {L0, L1} pairs of input
 * wires [first, first+count) as gc_wire [batch][count] (what COT.Send consumes), and the evaluator's delivered
 * labels gc_label [batch][count] back into its wire array.  Asynchronous on the ctx stream. */
int gc_batch_gather_input_wires(gc_batch *garbler, uint32_t first, uint32_t count, void *d_wires_out);
int gc_batch_set_input_range(gc_batch *evaluator, uint32_t first, uint32_t count, const void *d_labels);

/* Table egress / ingest in the wire format of the 2-party driver, on the device:
 * replaces the per-gate SendUint32(len) + SendLabel loop of circuit.Garbler (circuit/garbler.go:69-82) and the
 * receive loop of circuit.Evaluator (circuit/evaluator.go:40-66).  Per instance:
 *   BE32(#gates) | per gate: BE32(#rows) rows x BE(D0)||BE(D1)        = gc_tables_wire_bytes() bytes
 * so the host hands the buffer to conn.Write / fills it from the conn in one piece.
 * d_out / d_in: device byte buffers, `stride` bytes between instances (multiple of 4, >= the size).
 * ingest: *d_bad (u32, device) counts headers that do not match the circuit ("wrong number of gates",
 * evaluator.go:44-47; row counts that Eval would reject, eval.go:54-56,86-89). */
size_t gc_tables_wire_bytes(const gc_circ *);
int gc_batch_egress_tables(gc_batch *, void *d_out, size_t stride);
int gc_batch_ingest_tables(gc_batch *, const void *d_in, size_t stride, void *d_bad);
/* sha2pc's encoding of the same tables (sha2pc/encoding.go:363-411 encodeGarbledTables / decodeGarbledTables): the
 * rows of all gates back to back in gate order, BE(D0)||BE(D1) each, no headers: 16 * slab_rows bytes per instance
 * (= garbledTableByteLen, sha2pc/params.go); stride = bytes between instances, a multiple of 16. */
int gc_batch_egress_tables_dense(gc_batch *, void *d_out, size_t stride);
int gc_batch_ingest_tables_dense(gc_batch *, const void *d_in, size_t stride);

/* timing of the most recent garble / eval on this batch, measured with HIP events recorded on
 * the ctx stream around the gate kernels (the one fused launch, or the level launches; the few-microsecond
 * label initialisation kernel of a garble is outside) (ms); negative if none */
float gc_batch_last_ms(gc_batch *);
/* gate-kernel launches issued by the most recent garble / eval (1 for the fused schedules) */
uint32_t gc_batch_last_launches(gc_batch *);
/* developer aid: s_memtime breakdown of the fused kernels.  enable != 0 switches the instrumented
 * build of the kernel on for subsequent passes; out16 (may be NULL) receives, averaged over
 * workgroups, 8 cycle counters of wave 0 {prologue, hash phase, barrier after hash, staging commit,
 * XOR run, chunk-end barrier, -, -} followed by the same 8 for wave 3, from the most recent
 * instrumented pass. */
int gc_batch_debug_profile(gc_batch *, int enable, uint64_t *out8);
/* developer aid (synchronous): the round-key words the keyed passes hash with, as the device expands them from d_keys:
 * words_out = u32 [batch][4 * (rounds + 1)], big-endian words of the AES key schedule with the last round key XORed with
 * round key 0; host_words_out (may be NULL) receives the same from the host's schedule.  Any batch. */
int gc_batch_debug_keyed_schedule(gc_batch *, const void *d_keys, size_t keylen, uint32_t *words_out,
                                  uint32_t *host_words_out);

/* ------------------------------------------------------------------------------------------
 * Streaming for S sessions of ONE program per call (additive) — a host that gathers S concurrent
 * two-party sessions running the same streamed program (compiler/ssa/streamer.go -> circuit.Streaming.Garble).  Every
 * session runs the same SSA step on the same circuit with the same in[] / out[]; they differ in key, R and labels.  A step
 * is ONE keyed batch pass over S instances (gc_batch_garble_keyed / gc_batch_eval_keyed) between a gather from and a scatter
 * into a device-resident wire store [wire id][bstride] (bstride = sessions rounded up to 64; garbler: R per session plus
 * L0, evaluator: the active label), which grows on demand with the largest id of in[] / out[].  Session s's results are byte
 * for byte those of gc_stream_* / gc_stream_eval_* for that session alone, with its own key and random stream.  All d_*
 * arguments are DEVICE pointers.  Steps of a handle are serial on the ctx stream; only the sessions are parallel.
 * ------------------------------------------------------------------------------------------ */
typedef struct gc_stream_batch gc_stream_batch;
typedef struct gc_stream_eval_batch gc_stream_eval_batch;
/* NewStreaming (stream_garble.go:41-75) for `sessions` (1 .. 65 535) sessions:
 *  d_keys  u8 [sessions][keylen], keylen 16, 24 or 32 for all (GC_E_KEYSIZE otherwise); copied
 *  d_rnd   u8 [sessions][1 + ninputs][16]: per session what gc_stream_create's rnd holds — R (its S bit is forced on), then one
 *          L0 per entry of inputs[]; read before the call returns
 * A wire never set reads as (L0, L1) = (0, R), as in gc_stream.  GC_E_ARG for a wire id >= GC_STREAM_MAX_WIRES (here and
 * in every call below), GC_E_NOMEM when the store cannot grow. */
gc_stream_batch *gc_stream_batch_create(gc_ctx *, uint32_t sessions, const void *d_keys, size_t keylen, const void *d_rnd,
                                        const uint32_t *inputs, uint32_t ninputs, int *status);
void gc_stream_batch_free(gc_stream_batch *);
/* host only, no GPU: the bytes (*Streaming).Garble(c, in, out) writes for this step (stream_garble.go:385-449) — the same for
 * every session; 0 for a step that gc_stream_batch_garble refuses by its shape (see there; gc_last_error() says why) */
size_t gc_stream_batch_step_bytes(const gc_gate *gates, uint32_t ngates, uint32_t nwires, const uint32_t *in, uint32_t nin,
                                  const uint32_t *out, uint32_t nout);
/* (*Streaming).Garble(c, in, out) for all sessions (stream_garble.go:161-192; the tweak restarts at 0 per circuit): enqueued
 * on the ctx stream — gather of in[] from the store, the keyed pass, scatter through out[], serialiser — and not waited for.
 * *written = the step's bytes (= gc_stream_batch_step_bytes), known when the call returns; session s's bytes land at
 * (u8 *)d_out + s * stride exactly as :391-446 writes them; stride: any multiple of 4 >= *written; d_out: any byte alignment
 * (a caller appends step after step at a running offset).  in[] and out[] may name the same GLOBAL wire (in-place update):
 * a gate that reads such an input after the gate that set the output sees the new label, as in gc_stream_garble.  The
 * circuit + batch are recognised by gate-list content and cached per handle, bounded in device bytes
 * (GC_STREAM_BATCH_CACHE_BYTES, default 1 GiB; least recently used first).  ngates == 0 writes nothing and is GC_OK.  Not inside a pipeline capture (GC_E_ARG).
 * Refused with GC_E_ARG and a gc_last_error() text, the store unchanged: a step whose circuit is outside
 * gc_batch_keyed_supported at this number of sessions (wires in LDS and the key table does not fit); a circuit whose output
 * range overlaps its input range (nwires - nout < nin); a gate that writes an input-mapped wire.  GC_E_GATE / GC_E_WIRE for
 * an invalid op / a wire id >= nwires. */
int gc_stream_batch_garble(gc_stream_batch *, const gc_gate *gates, uint32_t ngates, uint32_t nwires, const uint32_t *in,
                           uint32_t nin, const uint32_t *out, uint32_t nout, void *d_out, size_t stride, size_t *written);
/* (*Streaming).GetInput(w) of every session: out[sessions]; waits for the ctx stream */
int gc_stream_batch_get_wire(gc_stream_batch *, uint32_t w, gc_wire *out);
/* {L0, L0 ^ R} of the named global wires as gc_wire [sessions][n] in device memory — what gc_cot_multi_send_pads_dev consumes
 * for the peer's inputs; asynchronous (ids[] may be reused on return) */
int gc_stream_batch_gather_wires(gc_stream_batch *, const uint32_t *ids, uint32_t n, void *d_wires_out);
/* read-only counters of the handle's circuit cache (any pointer may be NULL): entries / bytes = what it holds now, in the
 * device bytes that count against GC_STREAM_BATCH_CACHE_BYTES; loads = steps whose circuit was not cached and was kept;
 * evictions = entries freed to stay within the budget.  A refused step moves none of them. */
int gc_stream_batch_cache_stats(const gc_stream_batch *, uint64_t *entries, uint64_t *bytes, uint64_t *loads, uint64_t *evictions);

/* the evaluator's side: the store of circuit.StreamEval for `sessions` sessions; d_keys as above */
gc_stream_eval_batch *gc_stream_eval_batch_create(gc_ctx *, uint32_t sessions, const void *d_keys, size_t keylen, int *status);
void gc_stream_eval_batch_free(gc_stream_eval_batch *);
/* input labels (OT results): d_labels = gc_label [sessions][n] for the wires ids[0 .. n); asynchronous */
int gc_stream_eval_batch_set_wires(gc_stream_eval_batch *, const uint32_t *ids, uint32_t n, const void *d_labels);
/* out[sessions]: the active label of wire w in every session; waits for the ctx stream */
int gc_stream_eval_batch_get_wire(gc_stream_eval_batch *, uint32_t w, gc_label *out);
/* the evaluator's counterpart of gc_stream_batch_cache_stats (its cache holds the circuits of the parsed blocks) */
int gc_stream_eval_batch_cache_stats(const gc_stream_eval_batch *, uint64_t *entries, uint64_t *bytes, uint64_t *loads,
                                     uint64_t *evictions);
/* ONE OpCircuit block of every session (the per-gate loop of StreamEvaluator, stream_evaluator.go:270-432).  ref_block: a
 * HOST copy of any one session's block bytes; it is parsed and checked as gc_stream_eval_circuit parses a block, with the same
 * refusals (GC_E_GATE, GC_E_ROWS, GC_E_ARG) and the same size checks before anything is sized by the peer's data.  d_blocks:
 * all blocks in device memory, `stride` bytes apart (a multiple of 4, >= len).  On the device: every session's bytes
 * outside the table rows are compared with ref_block's — d_bad[s] (u32 [sessions], zeroed by the call) = the number of
 * differing bytes —, its rows are taken at ref_block's offsets, inputs gathered, the keyed pass, outputs scattered.  A
 * session with d_bad[s] != 0 is the caller's to run again through gc_stream_eval_*: its output wires are unspecified, and
 * nothing was read outside [0, len) of its block or written outside its own column of the store (every offset comes from
 * ref_block); every other session is exact.  A changed ROW byte is data, not structure: d_bad stays 0 and the labels are what
 * StreamEvaluator computes from those bytes.  *consumed = bytes of a block.  GC_E_ARG with a gc_last_error() text for a
 * block whose circuit is outside gc_batch_keyed_supported. */
int gc_stream_eval_batch_circuit(gc_stream_eval_batch *, uint32_t ngates, uint32_t ntmp, uint32_t nwires, const uint8_t *ref_block,
                                 size_t len, const void *d_blocks, size_t stride, void *d_bad, size_t *consumed);

/* ---- the other two phases of a session and the way to host memory (additive).  Every rule above holds: not
 * inside a pipeline capture (GC_E_ARG), GC_E_ARG for a wire id >= GC_STREAM_MAX_WIRES, the store grows with the largest id
 * as in gc_stream_batch_gather_wires. ---- */
/* The garbler's own input labels (compiler/ssa/streamer.go:79-102: L1 if inputs.Bit(i), else L0) for all sessions:
 *  d_bits        u8 [sessions][n], a non-zero byte is 1 (as gc_batch_select_inputs reads its bits)
 *  d_labels_out  gc_label [sessions][n] = L0 of wire ids[j] in session s, ^ R[s] where the bit is 1
 * A wire never set gives 0 or R[s] (the label form of gc_stream_batch_gather_wires).  ids may repeat; n = 0 is GC_OK.
 * Asynchronous on the ctx stream; ids[] may be reused on return. */
int gc_stream_batch_select_labels_dev(gc_stream_batch *, const uint32_t *ids, uint32_t n, const void *d_bits, void *d_labels_out);
/* The result (streamer.go:563-579: label.Equal(wire.L0) -> 0, wire.L1 -> 1, else "unknown label") for all sessions:
 *  d_labels    gc_label [sessions][n], what the peers sent back for the wires ids[0 .. n)
 *  d_bits_out  u8 [sessions][n]: 0, 1, or 0xff where the label is neither (as gc_batch_decode writes its bits)
 *  d_bad       u32 [sessions], zeroed by the call: the number of session s's 0xff entries
 * ids may repeat; n = 0 zeroes d_bad and is GC_OK.  Asynchronous on the ctx stream; ids[] may be reused on return. */
int gc_stream_batch_decode_dev(gc_stream_batch *, const uint32_t *ids, uint32_t n, const void *d_labels, void *d_bits_out, void *d_bad);
/* the host forms of the two: host pointers, synchronous, staged as the host forms of the OT family are */
int gc_stream_batch_select_labels(gc_stream_batch *, const uint32_t *ids, uint32_t n, const uint8_t *bits, gc_label *labels_out);
int gc_stream_batch_decode(gc_stream_batch *, const uint32_t *ids, uint32_t n, const gc_label *labels, uint8_t *bits_out,
                           uint32_t *bad_out);

/* The garbler's stream bytes in windows of pinned host memory.  All sessions of a handle write the same number of bytes per
 * step, so their streams advance in lock step: a window is a device array [sessions][cap] plus a pinned host array of the same
 * shape, cap = window_bytes rounded up to 16; nwindows >= 2 (else GC_E_ARG).  The steps fill one window after the other; a
 * window is SEALED when it is exactly full, when the next step does not fit behind what it holds, or by _flush if it holds any
 * byte.  Sealing records an event on the ctx stream; a second stream of the handle waits for it and copies the window's used
 * columns to the host (GC_STREAM_BATCH_OUT_WHOLE_ROWS=1: the whole array in one piece) while the ctx stream goes on into the
 * next free window.  A step is never split over two windows.
 *  _create   NULL + *status on failure (GC_E_ARG, GC_E_NOMEM, GC_E_HIP)
 *  _free     waits for its copies; free it before the gc_stream_batch
 *  _garble   gc_stream_batch_garble with d_out = the filling window at its running offset and stride = cap.  prefix[0 ..
 *            prefix_len), prefix_len 0 .. 64 (else GC_E_ARG), is written to every session in front of the step's bytes — the
 *            20-byte OpCircuit header of streamer.go:679-693, so that a window is what goes onto a socket; *written includes
 *            it.  A step larger than cap grows the EMPTY filling window alone, to the step rounded up to 4 096 (counted in
 *            `grown`); a failed allocation there is GC_E_NOMEM and nothing has changed.  When no window is free it returns
 *            GC_E_BUSY: nothing has happened — the store is unchanged, nothing is queued, `busy` is counted — and the caller
 *            releases a window and repeats the call.  It never waits for the caller, only for the device.
 *  _flush    seals the filling window if it holds any byte (else nothing)
 *  _next     hands out the oldest sealed window not yet handed out and waits for its copy: session s's next *len bytes are at
 *            *base + s * *stride.  With nothing sealed: GC_OK with *len = 0, without waiting.
 *  _release  returns the oldest handed-out window to the ring; several may be out at once and they come back in order.  With
 *            nothing handed out: GC_E_ARG.
 *  _stats    windows sealed, bytes per session accepted by _garble, windows grown, GC_E_BUSY answers (any pointer may be NULL)
 * One thread on _garble / _flush and one other on _next / _release may use a handle at the same time (_next waits outside the
 * handle's lock).  gc_stream_batch_garble on the same gc_stream_batch stays legal meanwhile; its bytes go where its caller says
 * and are part of no window. */
typedef struct gc_stream_batch_out gc_stream_batch_out;
gc_stream_batch_out *gc_stream_batch_out_create(gc_stream_batch *, size_t window_bytes, uint32_t nwindows, int *status);
void gc_stream_batch_out_free(gc_stream_batch_out *);
int gc_stream_batch_out_garble(gc_stream_batch_out *, const uint8_t *prefix, size_t prefix_len, const gc_gate *gates, uint32_t ngates,
                               uint32_t nwires, const uint32_t *in, uint32_t nin, const uint32_t *out, uint32_t nout, size_t *written);
int gc_stream_batch_out_flush(gc_stream_batch_out *);
int gc_stream_batch_out_next(gc_stream_batch_out *, const uint8_t **base, size_t *stride, size_t *len);
int gc_stream_batch_out_release(gc_stream_batch_out *);
int gc_stream_batch_out_stats(const gc_stream_batch_out *, uint64_t *sealed, uint64_t *bytes_per_session, uint64_t *grown, uint64_t *busy);

/* The SPLIT form of the window handle (additive): a gc_stream_batch_out whose mode is fixed at creation and
 * whose every other call is the one above.  It differs in what _garble does with a step of n bytes per session (prefix
 * included): the bytes go behind what the filling window holds, at `off`, and on into the windows after it from their byte 0 —
 * segments [0, min(n, cap - off)), then runs of cap bytes, then the rest, k = ceil((off + n) / cap) windows in all.  Every
 * touched window that becomes exactly full is sealed (if off + n is a multiple of cap the last one too, and no empty window
 * is touched); no window is sealed short but by _flush and none ever grows (`grown` stays 0), so the handle pins
 * nwindows * sessions * cap bytes whatever the steps are and every handed-out window but a flushed one is exactly cap bytes
 * long.  The keyed pass, the scatter into the store and the step's constants run once per step and the serialiser once per
 * segment; a window's seal is queued right behind the launch of its segment, so window j leaves for the host while segment
 * j + 1 is written.  For every session the windows in the order they are handed out are byte for byte `prefix | step` over
 * the steps: what the unsplit handle delivers.
 *   The step needs the filling window and the k - 1 windows behind it to be free; if they are not: GC_E_BUSY under the rule
 * above (nothing has happened).  n > (nwindows - 1) * cap can never be guaranteed that room: GC_E_ARG with a gc_last_error()
 * text that names both numbers, nothing has happened and the handle stays usable; any smaller step fits once enough windows
 * are released (off < cap).  _create_split refuses what _create refuses.
 *  _split_stats  steps that touched more than one window, serialiser launches (any pointer may be NULL); zeros on an unsplit
 *                handle */
gc_stream_batch_out *gc_stream_batch_out_create_split(gc_stream_batch *, size_t window_bytes, uint32_t nwindows, int *status);
int gc_stream_batch_out_split_stats(const gc_stream_batch_out *, uint64_t *split_steps, uint64_t *segments);
/* The fallback of the two handles: with on != 0, a step (a block) whose circuit is outside gc_batch_keyed_supported at this
 * number of sessions for the ONE reason that its wires are in LDS and the tile's key table does not fit behind them is loaded
 * with gc_batch_set_keyed_path(batch, 2) and runs on the keyed HBM-wire kernels — the same bytes and labels, cached and
 * counted like any other step.  The setting holds for circuits loaded after the call; the default is 0: the refusal above.
 * The evaluator's covers _circuit, _circuit_host and the intake. */
int gc_stream_batch_set_fallback(gc_stream_batch *, int on);
int gc_stream_eval_batch_set_fallback(gc_stream_eval_batch *, int on);

/* gc_stream_eval_batch_circuit with the blocks in HOST memory: session s's block at blocks + s * stride, any stride >= len (the
 * layout of a garbler window: *base + offset of gc_stream_batch_out_next is a valid argument).  Session ref_session's bytes
 * are the reference block, parsed and refused exactly as there; the rest of the step is the same.  The blocks go into a ring
 * of two device buffers of the handle on a stream of their own, so block k + 1 uploads while block k evaluates.  Pinned
 * memory (gc_host_is_pinned) is copied by DMA straight from the caller's pages: it must stay valid and unchanged until
 * gc_stream_eval_batch_uploads_wait, _bad or _free returns.  Pageable memory goes through pinned staging of the handle, and
 * the call returns when `blocks` may be reused.  The count of differing structure bytes is ADDED into an array of the handle:
 * _bad waits and returns the sums since create (bad_out[sessions]); a session that differed once stays marked, and its later
 * labels are unspecified. */
int gc_stream_eval_batch_circuit_host(gc_stream_eval_batch *, uint32_t ngates, uint32_t ntmp, uint32_t nwires, const uint8_t *blocks,
                                      size_t stride, size_t len, uint32_t ref_session, size_t *consumed);
int gc_stream_eval_batch_uploads_wait(gc_stream_eval_batch *);
int gc_stream_eval_batch_bad(gc_stream_eval_batch *, uint32_t *bad_out /* [sessions] */);

/* The evaluator driven from what arrives on a wire (additive): the result labels and the chunked intake. */

/* OpReturn (circuit/stream_evaluator.go:434-461: one label per output wire id) for all sessions:
 *  d_labels_out  gc_label [sessions][n] = the active label of global wire ids[j] in session s — the array
 *                gc_stream_batch_decode_dev reads
 * A wire never set gives what gc_stream_eval_batch_get_wire gives for it (zero).  ids may repeat; n = 0 is GC_OK.  Not inside
 * a pipeline capture and no id >= GC_STREAM_MAX_WIRES (GC_E_ARG); the store grows as in gc_stream_eval_batch_set_wires.
 * Asynchronous on the ctx stream; ids[] may be reused on return.  The second form takes a host pointer and is synchronous,
 * staged as the host forms of the OT family are. */
int gc_stream_eval_batch_return_labels_dev(gc_stream_eval_batch *, const uint32_t *ids, uint32_t n, void *d_labels_out);
int gc_stream_eval_batch_return_labels(gc_stream_eval_batch *, const uint32_t *ids, uint32_t n, gc_label *labels_out);

/* The intake: the next bytes of every session's stream, in chunks that respect no step boundary.  The streams are in lock step
 * (one program, the same number of bytes per step in every session), so the message loop of stream_evaluator.go:227-249 runs
 * once, over session ref_session's bytes: BE32 op, and for OpCircuit (1) BE32 step, numGates, numTmpWires, numWires and the
 * block.  Every complete OpCircuit message in the bytes held so far is evaluated, in stream order, exactly as
 * gc_stream_eval_batch_circuit_host evaluates it: the same refusals and size checks before anything is sized by peer data,
 * every offset from the reference session, the per-session count of differing structure bytes — the 20 header bytes
 * included — added into the sums of gc_stream_eval_batch_bad.
 *  _create  max_message_bytes (20 .. 2^31 - 2, else GC_E_ARG) bounds what the handle holds of ONE unfinished message, header
 *           included; NULL + *status on failure
 *  _free    waits for its uploads; free it before the gc_stream_eval_batch
 *  _feed    session s's next len bytes are at chunk + s * stride, any stride >= len (*base of gc_stream_batch_out_next is a
 *           valid argument); pinned and pageable memory follow the rules of gc_stream_eval_batch_circuit_host.  The chunk is
 *           uploaded ONCE, on the handle's upload stream, behind the bytes of the unfinished message of earlier feeds, and
 *           its blocks are ingested in place.  A message that the chunk does not complete — it may end in the header, in a
 *           gate's op byte, in an id or in a row, and span any number of feeds — is no error: its bytes are kept, *taken = len
 *           and *next_op = 1.  At the first complete op word that is not OpCircuit the feed stops in front of it: *next_op =
 *           that word, *taken = the bytes of this chunk in front of it, and nothing is kept; the caller reads that message
 *           itself (OpReturn: gc_stream_eval_batch_return_labels) and feeds again from the next op word.  (A word that began
 *           in an earlier chunk gives *taken = 0; the bytes of it that earlier feeds took — the sum of their *taken minus
 *           bytes_per_session of _stats — are dropped.)  An op the reference would refuse is reported the same way, not
 *           judged.  A message the parser refuses returns the code of gc_stream_eval_batch_circuit_host (GC_E_GATE,
 *           GC_E_ARG, GC_E_ROWS for a header whose numGates cannot fit under max_message_bytes, or when the kept bytes would
 *           exceed it): the messages before it stay evaluated, *taken = the bytes of this chunk in front of it, nothing is
 *           kept and the handle stays usable.  Nothing is allocated from numGates before the bytes are there.
 *  _stats   messages evaluated, their bytes per session, chunks uploaded, bytes per session kept at the end of a feed summed
 *           over the feeds (any pointer may be NULL)
 * One thread feeds a handle at a time.  gc_stream_eval_batch_circuit_host stays legal on the same gc_stream_eval_batch while no
 * intake holds an unfinished message; _bad and _uploads_wait also wait for the intake's uploads. */
typedef struct gc_stream_eval_batch_in gc_stream_eval_batch_in;
gc_stream_eval_batch_in *gc_stream_eval_batch_in_create(gc_stream_eval_batch *, uint32_t ref_session, size_t max_message_bytes, int *status);
void gc_stream_eval_batch_in_free(gc_stream_eval_batch_in *);
int gc_stream_eval_batch_in_feed(gc_stream_eval_batch_in *, const uint8_t *chunk, size_t stride, size_t len, size_t *taken,
                                 uint32_t *next_op);
int gc_stream_eval_batch_in_stats(const gc_stream_eval_batch_in *, uint64_t *steps, uint64_t *bytes_per_session, uint64_t *uploads,
                                  uint64_t *carried_bytes);

/* ------------------------------------------------------------------------------------------
 * IKNP OT extension + MITCCRH (ot/iknp.go, ot/mitccrh.go, ot/cot.go)
 * ------------------------------------------------------------------------------------------ */
typedef struct gc_iknp gc_iknp;

/* Receiver state after the base OTs: replaces the tail of NewIKNPReceiver (iknp.go:347-356):
 * base[128] are the (L0,L1) pairs sent through the base OT; column PRGs g0/g1 are keyed by them */
gc_iknp *gc_iknp_receiver_create(gc_ctx *, const gc_wire *base, int *status);
/* Sender state: replaces the tail of NewIKNPSender (iknp.go:104-122): delta and the 128 labels
 * k0[i] received from the base OT with choice bits delta.Bit(i) */
gc_iknp *gc_iknp_sender_create(gc_ctx *, const gc_label *delta, const gc_label *k0, int *status);
void gc_iknp_free(gc_iknp *);

/* bytes of u-matrix data exchanged for n OTs (sum of the chunk lengths of iknp.go:482-505) */
size_t gc_iknp_u_bytes(size_t n);
/* Replaces the body of (*IKNPReceiver).receive(b, result)   ot/iknp.go:468-511
 *  choice  bool per OT (n bytes, non-zero = true)
 *  u_out   the chunks the Go loop would SendData, concatenated (gc_iknp_u_bytes(n) bytes); the
 *          shim frames them as ≤8 KiB messages exactly like iknp.go:499
 *  labels_out [n]                                                                         */
int gc_iknp_receive(gc_iknp *, const uint8_t *choice, size_t n, uint8_t *u_out, gc_label *labels_out);
/* Replaces the body of (*IKNPSender).send(n)   ot/iknp.go:197-226 (u_in = the received chunks, concatenated) */
int gc_iknp_send(gc_iknp *, const uint8_t *u_in, size_t u_len, size_t n, gc_label *labels_out);
/* Device-resident forms of the two calls above (pipelines that keep the u-matrix and the labels in HBM, e.g.
 * labels that feed gc_batch_set_inputs / the COT kernels directly): all pointers are DEVICE pointers,
 * d_choice_packed = the choice bits packed LSB-first, 64 bytes per 512-OT chunk (iknp.go:472-477; zero-padded to
 * a whole chunk); asynchronous on the ctx stream, no allocation after the first call of a given size.
 * gc_iknp_last_ms: HIP-event time of the kernels of the most recent *_dev call. */
int gc_iknp_receive_dev(gc_iknp *, const void *d_choice_packed, size_t n, void *d_u_out, void *d_labels_out);
int gc_iknp_send_dev(gc_iknp *, const void *d_u_in, size_t n, void *d_labels_out);
float gc_iknp_last_ms(gc_iknp *);

/* bit-COT: bodies of (*IKNPReceiver).ReceiveBits (ot/iknp.go:554-620) and
 * (*IKNPSender).SendBits (ot/iknp.go:259-310); choices / result are packed little-endian u64 bit vectors.
 * The reference only folds WHOLE 64-bit choice words into u (iknp.go:583-597); reproduced as is. */
int gc_iknp_receive_bits(gc_iknp *, const uint64_t *choices, size_t n, uint8_t *u_out, uint64_t *result);
int gc_iknp_send_bits(gc_iknp *, const uint8_t *u_in, size_t u_len, size_t n, uint64_t *result);

/* the same two bodies with the choice words, the u-matrix and the result words in HBM (device pointers, asynchronous on
 * the ctx stream; the labels stay in the handle's device workspace) */
int gc_iknp_receive_bits_dev(gc_iknp *, const void *d_choices, size_t n, void *d_u_out, void *d_result);
int gc_iknp_send_bits_dev(gc_iknp *, const void *d_u_in, size_t n, void *d_result);

/* KOS consistency check of the malicious variant: the chi-PRG + GF(2^128) inner products of
 * (*IKNPReceiver).Receive (ot/iknp.go:405-465) and (*IKNPSender).Send (ot/iknp.go:138-194; gf128.go:14-27,
 * mul128_generic.go).  chi_i = label i of the AES-128-CTR stream keyed by seed2: 0..n-1 for `result`,
 * n..n+255 for the 256-label random choice vector.
 *  receiver: x = XOR_{b_i} chi_i, (t0,t1) = XOR_i chi_i * result_i (256-bit, no reduction)
 *  sender:   *ok = ((q0,q1) ^ x*Delta == (t0,t1)) with (q0,q1) the same sum over its own labels;
 *            ok == 0 is the reference's "OT extension check failed" */
int gc_kos_receiver_tags(gc_ctx *, const gc_label *seed2, const gc_label *result, const uint8_t *b, size_t n,
                         const gc_label *choice_vec, const uint8_t *bcv /*256*/, gc_label *x, gc_label *t0,
                         gc_label *t1);
int gc_kos_sender_check(gc_ctx *, const gc_label *seed2, const gc_label *result, size_t n,
                        const gc_label *choice_vec /*256*/, const gc_label *delta, const gc_label *x,
                        const gc_label *t0, const gc_label *t1, int *ok);
/* the same two checks over labels (and the receiver's choice bytes) that are already in HBM — the outputs of
 * gc_iknp_receive_dev / gc_iknp_send_dev; d_result [n] gc_label, d_b [n] bytes are DEVICE pointers (additive) */
int gc_kos_receiver_tags_dev(gc_ctx *, const gc_label *seed2, const void *d_result, const void *d_b, size_t n,
                             const gc_label *choice_vec, const uint8_t *bcv /*256*/, gc_label *x, gc_label *t0,
                             gc_label *t1);
int gc_kos_sender_check_dev(gc_ctx *, const gc_label *seed2, const void *d_result, size_t n,
                            const gc_label *choice_vec /*256*/, const gc_label *delta, const gc_label *x,
                            const gc_label *t0, const gc_label *t1, int *ok);

/* Replaces (*MITCCRH).Hash over a whole COT/ROT run (mitccrh.go:93-128 as driven by cot.go:160-171,
 * 203-211): OT j (key index gid0+j, key = BE(Label{D0:gid,D1:0} ^ seed)) hashes its h consecutive
 * blocks in place: blk ^= AES_key(blk).  blks = [n][h] */
int gc_mitccrh_hash(gc_ctx *, const gc_label *seed, uint64_t gid0, gc_label *blks, size_t n, uint32_t h);
/* Replaces the pad loop of COT.Send (cot.go:155-182): out[2n] = the labels sent on the wire */
int gc_cot_send_pads(gc_ctx *, const gc_label *seed, const gc_label *delta, const gc_label *data,
                     const gc_wire *wires, size_t n, gc_label *out);
/* Replaces the unpad loop of COT.Receive (cot.go:200-232): result[n] in = IKNP output, out = chosen labels */
/* device-resident forms (device pointers, asynchronous on the ctx stream): d_data = the sender's IKNP labels
 * (gc_iknp_send_dev), d_wires = gc_wire [n], d_out = gc_label [2n]; d_flags = u8 [n] choice bits, d_sent = the 2n
 * labels received, d_result = the receiver's IKNP labels in, the chosen wire labels out */
int gc_cot_send_pads_dev(gc_ctx *, const gc_label *seed, const gc_label *delta, const void *d_data,
                         const void *d_wires, size_t n, void *d_out);
int gc_cot_receive_unpad_dev(gc_ctx *, const gc_label *seed, const void *d_flags, const void *d_sent,
                             void *d_result, size_t n);
int gc_cot_receive_unpad(gc_ctx *, const gc_label *seed, const uint8_t *flags, const gc_label *sent,
                         gc_label *result, size_t n);

/* ROT (ot/rot.go:132-202).  Replaces the pad loop of ROT.Send (rot.go:156-172): data = the sender's IKNP
 * labels (IKNPSender.Send), wires_out[j] = {H_j(data_j), H_j(data_j ^ delta)} — the sender's wire labels are OVERWRITTEN
 * with the two hashed pads (rot.go:168-171), nothing but the seed travels — and the loop of ROT.Receive (rot.go:194-199):
 * result[j] = H_j(result[j]) in place (result in = IKNPReceiver.Receive's labels).  H_j(x) = x ^ AES_{key_j}(x), key_j =
 * BE(Label{D0: j, D1: 0} ^ seed), a fresh MITCCRH per call (rot.go:143,191).  The receiver's result[j] equals
 * wires_out[j].L{flag_j} of the sender.  _dev: device pointers, asynchronous on the ctx stream. */
int gc_rot_send(gc_ctx *, const gc_label *seed, const gc_label *delta, const gc_label *data, size_t n, gc_wire *wires_out);
int gc_rot_receive(gc_ctx *, const gc_label *seed, gc_label *result, size_t n);
int gc_rot_send_dev(gc_ctx *, const gc_label *seed, const gc_label *delta, const void *d_data, size_t n, void *d_wires_out);
int gc_rot_receive_dev(gc_ctx *, const gc_label *seed, void *d_result, size_t n);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU (BASELINE config 4: 65 536 instances, 8 192 per GPU): instances are independent
 * (fresh R and labels per Garble call, circuit/garble.go:253-278), so each device garbles / evaluates a contiguous
 * instance range through its own gc_ctx and the ONLY exchange is the terminal all-gather of the decoded output
 * bits (gc_batch_decode) or output labels (gc_batch_gather_outputs) — ncclAllGather of RCCL over xGMI, enqueued on
 * the ctx stream behind the kernels that produce the data.  The reference has no counterpart (single device); a Go
 * host (apps/garbled, circuit/garbler.go:53) calls these next to GarbleBatch / EvalBatch.  librccl is opened on first
 * use; without it every call returns GC_E_HIP (gc_last_error() says why) and the single-GPU path is unaffected.
 * ------------------------------------------------------------------------------------------ */
typedef struct gc_comm gc_comm;
#define GC_COMM_ID_BYTES 128
int gc_comm_available(void); /* 1 if librccl could be opened and has every entry point used here */
int gc_comm_version(void);   /* ncclGetVersion code (e.g. 22707), 0 if unavailable */
/* One process (or OS thread) per GPU: rank 0 draws the id (ncclGetUniqueId), the host hands the 128 bytes to the other
 * ranks over its own control channel, every rank joins with its ctx (ncclCommInitRank; collective, blocks until all
 * nranks have called). */
int gc_comm_get_unique_id(uint8_t *id, size_t len /* >= GC_COMM_ID_BYTES */);
gc_comm *gc_comm_init_rank(gc_ctx *, const uint8_t *id, size_t idlen, int nranks, int rank, int *status);
/* One process driving n devices (one gc_ctx each, distinct devices): ncclCommInitAll; out[n] */
int gc_comm_init_all(gc_ctx *const *ctxs, int n, gc_comm **out);
void gc_comm_destroy(gc_comm *);
int gc_comm_rank(const gc_comm *);
int gc_comm_nranks(const gc_comm *);
/* d_recv[r * bytes .. (r+1) * bytes) = rank r's d_send[0 .. bytes): device pointers, `bytes` equal on all ranks
 * (the host pads the last shard); asynchronous on the ctx stream */
int gc_comm_allgather(gc_comm *, const void *d_send, void *d_recv, size_t bytes);
/* the same for the n communicators of gc_comm_init_all from ONE host thread (ncclGroupStart / ncclGroupEnd) */
int gc_comm_allgather_all(gc_comm *const *comms, int n, const void *const *d_send, void *const *d_recv, size_t bytes);
/* host-side helpers for drivers and the benchmark: *value = max over ranks (synchronous); barrier = every rank's ctx
 * stream has drained */
int gc_comm_allreduce_max(gc_comm *, double *value);
int gc_comm_barrier(gc_comm *);


/* ------------------------------------------------------------------------------------------
 * GMW party engine (gmw/network.go, gmw/triples.go): the online phase of one party of the n-party GMW protocol over a
 * BATCH of independent evaluations of one circuit by the same parties, plus the local folds of the Beaver-triple
 * generation.  The p2p transport and the XOR of the opened values across peers (broadcastXORs, network.go:790-823) stay
 * with the caller; with batch = 1 every buffer below is byte for byte the Go bit vector, so a Go peer cannot tell.
 * All buffers are word-major u64: word index outside, instance inside ([words][batch]).
 * ------------------------------------------------------------------------------------------ */
typedef struct gc_gmw gc_gmw;
typedef struct gc_gmw_info {
    uint32_t ngates, nwires, ninputs, noutputs;
    uint32_t nlevels;         /* Stats[NumLevels] + 1 of AssignLevels(TargetGMW) (circuit.go:206-254) */
    uint32_t n_and_levels;    /* levels with at least one AND = exchange rounds of a pass */
    uint32_t triple_words;    /* TW = sum over levels of ceil(n_AND(level) / 64): whole words per level (triples.go:60-90) */
    uint32_t max_level_words; /* max over levels of ceil(n_AND(level) / 64) */
    uint32_t n_xor, n_xnor, n_and, n_inv;
    uint32_t max_free_depth;  /* longest chain of free gates between two exchanges (workgroup barriers of one step) */
} gc_gmw_info;

/* Host-only plan introspection (no GPU): arrays sized by the caller, any of them may be NULL.
 *  level_of_gate[ngates]      gate.Level of AssignLevels(TargetGMW)
 *  and_index_of_gate[ngates]  AND gate: its bit index k in its level's vectors (network.go:680-700); others 0xffffffff
 *  words_of_level[nlevels]    ceil(n_AND(level) / 64)
 * Checks those of gc_plan_create; OR is GC_E_GATE ("gate OR not supported", network.go:609). */
int gc_gmw_plan_describe(const gc_gate *gates, uint32_t ngates, uint32_t nwires, uint32_t ninputs, uint32_t noutputs,
                         gc_gmw_info *info, uint32_t *level_of_gate, uint32_t *and_index_of_gate, uint32_t *words_of_level);

/* One party (0 <= party < nparties, nparties >= 2) of `batch` instances; the handle keeps its own device state, so
 * several handles may share a ctx.  A pass: gc_gmw_set_inputs, gc_gmw_set_triples, then gc_gmw_step until *words == 0,
 * then gc_gmw_get_outputs.  Replaces the body of (*Network).run's level loop (network.go:563-618) and andBatchFlush
 * (network.go:660-757). */
gc_gmw *gc_gmw_create(gc_ctx *, const gc_gate *gates, uint32_t ngates, uint32_t nwires, uint32_t ninputs,
                      uint32_t noutputs, uint32_t nparties, uint32_t party, uint32_t batch, int *status);
void gc_gmw_free(gc_gmw *);
int gc_gmw_get_info(const gc_gmw *, gc_gmw_info *out);
/* inputs [ceil(ninputs/64)][batch]: this party's share of wires 0..ninputs-1 (the big.Int words of nw.wires after
 * setWires, network.go:560-561).  Starts a new pass; the triples must be set again after it. */
int gc_gmw_set_inputs(gc_gmw *, const uint64_t *inputs);
int gc_gmw_set_inputs_dev(gc_gmw *, const void *d_inputs);
/* a, b, c each [triple_words][batch]: level l uses words [W_l, W_l + w_l) (TriplePool.Get, triples.go:130-142).
 * _dev: read in place during the pass (keep them alive until the last step); host form: copied. */
int gc_gmw_set_triples(gc_gmw *, const uint64_t *a, const uint64_t *b, const uint64_t *c);
int gc_gmw_set_triples_dev(gc_gmw *, const void *d_a, const void *d_b, const void *d_c);
/* One exchange round.  (1) if an AND level is pending, close it: d, e = this party's message XOR the npeers received
 * ones (peer_msgs [npeers][2][w][batch], the layout of msg_out), z = c ^ d&b ^ e&a (^ d&e on party 0)
 * (network.go:735-756); (2) evaluate the free gates up to the next level that has ANDs, or to the end; (3) write that
 * level's d then e to msg_out [2][*words][batch] (SendBitvec2, peer.go:131-163; padding bits past the level's ANDs carry
 * the triples' a / b bits, network.go:695-721), *level = the level.  *words == 0: the pass is complete (*level = nlevels).
 * npeers must be nparties - 1; peer_msgs may be NULL when nothing is pending.  _dev: device pointers, asynchronous on
 * the ctx stream; host form: synchronous. */
int gc_gmw_step(gc_gmw *, const uint64_t *peer_msgs, uint32_t npeers, uint64_t *msg_out, uint32_t *level, size_t *words);
int gc_gmw_step_dev(gc_gmw *, const void *d_peer_msgs, uint32_t npeers, void *d_msg_out, uint32_t *level, size_t *words);
/* [ceil(noutputs/64)][batch]: this party's share of the last noutputs wires (nw.output, network.go:622-624); only after
 * the pass is complete */
int gc_gmw_get_outputs(gc_gmw *, uint64_t *out);
int gc_gmw_get_outputs_dev(gc_gmw *, void *d_out);
uint32_t gc_gmw_last_launches(const gc_gmw *); /* kernel launches of the last pass, input load included */

/* Local arithmetic of tripleBatch (triples.go:287-466) on device words (u64 [words]), asynchronous on the ctx stream;
 * the bit-COT outputs come from gc_iknp_send_bits_dev / gc_iknp_receive_bits_dev. */
int gc_gmw_triples_local_dev(gc_ctx *, const void *d_a, const void *d_b, void *d_c, size_t words);        /* c = a & b */
int gc_gmw_triples_sender_u_dev(gc_ctx *, uint32_t delta_bit, const void *d_a, void *d_u, size_t words); /* u = a ^ (D0 ? ~0 : 0) */
int gc_gmw_triples_sender_fold_dev(gc_ctx *, const void *d_s, const void *d_u, const void *d_v, void *d_c,
                                   size_t words);                                                        /* c ^= s ^ (u & v) */
int gc_gmw_triples_receiver_fold_dev(gc_ctx *, const void *d_r, void *d_c, size_t words);                /* c ^= r */


/* ------------------------------------------------------------------------------------------
 * VOLE over packed IKNP (vole/vole.go, vole/prg.go).  p: the modulus, 32 bytes big-endian, odd, 3 <= p < 2^256
 * (else GC_E_ARG).  Every value is 32 bytes big-endian, element i at [32i, 32i+32): the reference's messages as they are.
 * Sender (Sender.Mul, vole.go:58-97): r_i = BE256(AES-128_{GetData(labels[i])}-CTR(zero IV, 32 zero bytes)) mod p,
 * u_msg_i = (r_i + x_i * (BE256(y_msg_i) mod p)) mod p; labels = the sender's IKNP labels (gc_iknp_send_dev).
 * Receiver (Receiver.Mul, vole.go:182-187): u_i = BE256(u_msg_i) mod p.  x, y and u_msg may be any value below 2^256.
 * p is a host pointer in every form.  Host forms: synchronous, staged through device buffers.  _dev forms: device
 * pointers, asynchronous on the ctx stream; d_u_out may be d_u_msg.  m = 0: GC_OK, nothing written.
 * ------------------------------------------------------------------------------------------ */
int gc_vole_sender_mul(gc_ctx *, const uint8_t *p, const gc_label *labels, const uint8_t *x, const uint8_t *y_msg,
                       size_t m, uint8_t *r_out, uint8_t *u_msg_out);
int gc_vole_sender_mul_dev(gc_ctx *, const uint8_t *p, const void *d_labels, const void *d_x, const void *d_y_msg,
                           size_t m, void *d_r_out, void *d_u_msg_out);
int gc_vole_receiver_reduce(gc_ctx *, const uint8_t *p, const uint8_t *u_msg, size_t m, uint8_t *u_out);
int gc_vole_receiver_reduce_dev(gc_ctx *, const uint8_t *p, const void *d_u_msg, size_t m, void *d_u_out);

/* ------------------------------------------------------------------------------------------
 * Chou-Orlandi base OT on P-256 (ot/co.go, ot/co_helpers.go).  The per-OT work of ONE session (one sender scalar a, one
 * point A), bit-exact with the reference.  crand.Int, the framing and the p2p messages stay with the caller, who passes
 * the scalars it drew.  Several sessions per call are the gc_co_multi_* calls at the end of this section.  Other curves
 * and ot.RSA are not covered.
 *   gc_p256_point  an affine point, x and y as 32 big-endian bytes each (the caller pads big.Int.Bytes() to that width);
 *                  64 zero bytes are the point at infinity, crypto/elliptic's (0, 0).  A point is VALID when 0 <= x, y < p
 *                  and y^2 = x^3 - 3x + b (curve.IsOnCurve): an encoding >= p is refused, not reduced, and so is infinity.
 *   scalars        32 bytes big-endian, any value below 2^256, taken mod N as the curve code does; b = 0 mod N gives
 *                  the point at infinity.
 *   mask(P, id)    deriveMask (co_helpers.go:222-235): SHA-256(x.Bytes() || y.Bytes() || BE64(id))[:16] with
 *                  minimal-length coordinates (infinity: two empty strings).  The id of OT i is id0 + i, so that a caller
 *                  may split a session into chunks.
 * Sender setup (GenerateCOSenderSetup, co_helpers.go:77-101), host only: A = a * G, AaInv = (x(a * A), p - y(a * A)); a = 0 mod N is
 *   GC_E_ARG.
 * Sender encrypt (EncryptCOCiphertexts, co_helpers.go:104-137): S = a * B_i, T = S + AaInv (a complete addition: S = AaInv doubles,
 *   S = -AaInv gives infinity), ct[i] = mask(S, id) ^ GetData(L0) || mask(T, id) ^ GetData(L1), 32 bytes per OT.  A B_i that
 *   is not VALID gets 32 zero bytes.  Host form: GC_E_POINT and *bad_index = the lowest such i (bad_index may be NULL; ct
 *   is written for every good point all the same).  _dev form: d_status is two uint64 in device memory that the call itself
 *   resets and the kernel fills: {number of bad points, lowest bad index (all ones: none)}; read it after gc_ctx_sync.
 *   a = 0 mod N or an AaInv that is not VALID: GC_E_ARG.  wires: the gc_wire array that is also gc_iknp_receiver_create's base.
 * Receiver choices (BuildCOChoices, co_helpers.go:140-177): B_i = b_i * G, + A when choice[i] != 0 (one byte per OT, as gc_iknp_receive).
 * Receiver decrypt (DecryptCOCiphertexts, co_helpers.go:191-219): labels_out[i] = SetData(mask(b_i * A, id) ^ (choice[i] ? ct1 : ct0));
 *   labels_out is gc_iknp_sender_create's k0.  An A that is not VALID: GC_E_POINT, in both receiver calls.
 * a, A and AaInv are host pointers in every form.  Host forms: synchronous, staged through device buffers.  _dev forms:
 * device pointers (16-byte aligned, as gc_dev_alloc returns them), asynchronous on the ctx stream.  n = 0: GC_OK, nothing
 * written.
 * ------------------------------------------------------------------------------------------ */
typedef struct gc_p256_point { uint8_t x[32], y[32]; } gc_p256_point;

/* GenerateCOSenderSetup, ot/co_helpers.go:77-101 (host only) */
int gc_co_sender_setup(const uint8_t *a, gc_p256_point *A_out, gc_p256_point *AaInv_out);
/* EncryptCOCiphertexts, ot/co_helpers.go:104-137, deriveMask ot/co_helpers.go:222-235; ct: 32 bytes per OT */
int gc_co_sender_encrypt(gc_ctx *, const uint8_t *a, const gc_p256_point *AaInv, const gc_p256_point *points,
                         const gc_wire *wires, size_t n, uint64_t id0, uint8_t *ct, size_t *bad_index);
int gc_co_sender_encrypt_dev(gc_ctx *, const uint8_t *a, const gc_p256_point *AaInv, const void *d_points,
                             const void *d_wires, size_t n, uint64_t id0, void *d_ct, void *d_status);
/* BuildCOChoices, ot/co_helpers.go:140-177 */
int gc_co_receiver_choices(gc_ctx *, const gc_p256_point *A, const uint8_t *scalars, const uint8_t *choice, size_t n,
                           gc_p256_point *points_out);
int gc_co_receiver_choices_dev(gc_ctx *, const gc_p256_point *A, const void *d_scalars, const void *d_choice, size_t n,
                               void *d_points_out);
/* DecryptCOCiphertexts, ot/co_helpers.go:191-219, deriveMask ot/co_helpers.go:222-235 */
int gc_co_receiver_decrypt(gc_ctx *, const gc_p256_point *A, const uint8_t *scalars, const uint8_t *choice,
                           const uint8_t *ct, size_t n, uint64_t id0, gc_label *labels_out);
int gc_co_receiver_decrypt_dev(gc_ctx *, const gc_p256_point *A, const void *d_scalars, const void *d_choice,
                               const void *d_ct, size_t n, uint64_t id0, void *d_labels_out);

/* The receiver's side of ONE session behind a handle: the two receiver calls above, byte for byte (scalars mod N, b = 0
 * mod N gives infinity, one choice byte per OT, the id of OT i is id0 + i, host forms synchronous, _dev forms asynchronous
 * on the ctx stream, n = 0: GC_OK and nothing written), with b_i * G and b_i * A summed from fixed-base window tables in
 * device memory instead of walked by double-and-add.  gc_co_base_create checks A (not VALID: NULL and *status =
 * GC_E_POINT), builds A's table on the host (61 440 bytes) and uploads it; the first handle of a ctx also uploads G's table
 * (built once per process), which is freed with the ctx.  Create is synchronous and not allowed between
 * gc_ctx_capture_begin and _end.  Several handles may live on one ctx, one per session, each for any number of calls; free
 * them before the ctx.  A NULL handle or NULL pointer: GC_E_ARG.  The tables are indexed by digits of b_i (as the AES
 * tables are by secret bytes); a caller who does not want that keeps the calls above. */
typedef struct gc_co_base gc_co_base;
gc_co_base *gc_co_base_create(gc_ctx *, const gc_p256_point *A, int *status);
void gc_co_base_free(gc_co_base *); /* waits for the ctx stream first; NULL is a no-op */
int gc_co_base_choices(gc_co_base *, const uint8_t *scalars, const uint8_t *choice, size_t n, gc_p256_point *points_out);
int gc_co_base_choices_dev(gc_co_base *, const void *d_scalars, const void *d_choice, size_t n, void *d_points_out);
int gc_co_base_decrypt(gc_co_base *, const uint8_t *scalars, const uint8_t *choice, const uint8_t *ct, size_t n,
                       uint64_t id0, gc_label *labels_out);
int gc_co_base_decrypt_dev(gc_co_base *, const void *d_scalars, const void *d_choice, const void *d_ct, size_t n,
                           uint64_t id0, void *d_labels_out);

/* S independent sessions in one call: what a caller has who runs S CO.Send / CO.Receive pairs of equal length at once (S
 * instances of a two-party run, S IKNP set-ups, the set-ups of the parties of a GMW network).  Session-major: OT j of
 * session s is element i = s * per + j of every per-OT array (the arrays of the one-session calls), and its id is id0 + j,
 * since Go numbers every session from 0.  Sessions of unequal length are padded by the caller.  The session constants are
 * arrays: a [S][32] bytes big-endian, any value below 2^256; A and AaInv [S] gc_p256_point.  Byte for byte, session s of a
 * multi call is the one-session call on that session alone.
 *   Setup: A_s = a_s * G, AaInv_s = (x, p - y) of a_s * A_s, on the device, one lane per session, from G's window table.
 *   A BAD SESSION gets zero bytes in all its outputs, and its OTs are not counted as bad points.  Sender calls: a_s = 0 mod
 *   N, or (encrypt) an AaInv_s that is not VALID.  Receiver calls: an A_s that is not VALID.  A bad point (B_i not VALID) in
 *   a good session is what it is in gc_co_sender_encrypt: 32 zero bytes and a count.
 *   d_status: four uint64 in device memory, {bad points, lowest bad OT index i, bad sessions, lowest bad session}, which the
 *   call itself resets on the stream to {0, ~0, 0, ~0} and the kernel fills; a session is counted once.  Read it after
 *   gc_ctx_sync.
 * _dev forms: device pointers for EVERY array, the session constants included (16-byte aligned), asynchronous on the ctx
 * stream, one kernel per call.  Host forms: host pointers, synchronous, staged; a bad session returns GC_E_ARG from the
 * sender calls and GC_E_POINT from the receiver calls with *bad_session = the lowest one, a bad point GC_E_POINT with
 * *bad_index = the lowest i; a bad session wins when both occur; every good output is written all the same (bad_index and
 * bad_session may be NULL).  S = 0 or per = 0: GC_OK, nothing written, the status included.  A NULL ctx, a NULL array with
 * S * per > 0, or an S * per * 64 that does not fit size_t: GC_E_ARG.  Setup and choices read G's table: the first such call
 * of a ctx uploads it as gc_co_base_create does (synchronously), and returns GC_E_ARG between gc_ctx_capture_begin and
 * _end.  The receiver's decrypt walks the ladder (gc_co_multi_base_* below reads per-session tables instead); choices index
 * G's table by digits of b_i, as gc_co_base_choices does. */
int gc_co_multi_sender_setup(gc_ctx *, const uint8_t *a, size_t S, gc_p256_point *A_out, gc_p256_point *AaInv_out,
                             size_t *bad_session);
int gc_co_multi_sender_setup_dev(gc_ctx *, const void *d_a, size_t S, void *d_A_out, void *d_AaInv_out, void *d_status);
int gc_co_multi_sender_encrypt(gc_ctx *, const uint8_t *a, const gc_p256_point *AaInv, const gc_p256_point *points,
                               const gc_wire *wires, size_t S, size_t per, uint64_t id0, uint8_t *ct, size_t *bad_index,
                               size_t *bad_session);
int gc_co_multi_sender_encrypt_dev(gc_ctx *, const void *d_a, const void *d_AaInv, const void *d_points, const void *d_wires,
                                   size_t S, size_t per, uint64_t id0, void *d_ct, void *d_status);
int gc_co_multi_receiver_choices(gc_ctx *, const gc_p256_point *A, const uint8_t *scalars, const uint8_t *choice, size_t S,
                                 size_t per, gc_p256_point *points_out, size_t *bad_session);
int gc_co_multi_receiver_choices_dev(gc_ctx *, const void *d_A, const void *d_scalars, const void *d_choice, size_t S,
                                     size_t per, void *d_points_out, void *d_status);
int gc_co_multi_receiver_decrypt(gc_ctx *, const gc_p256_point *A, const uint8_t *scalars, const uint8_t *choice,
                                 const uint8_t *ct, size_t S, size_t per, uint64_t id0, gc_label *labels_out,
                                 size_t *bad_session);
int gc_co_multi_receiver_decrypt_dev(gc_ctx *, const void *d_A, const void *d_scalars, const void *d_choice, const void *d_ct,
                                     size_t S, size_t per, uint64_t id0, void *d_labels_out, void *d_status);

/* The receiver's decrypt of S sessions behind a handle: gc_co_multi_receiver_decrypt / _dev byte for byte and status word for
 * status word (session-major, the id of OT j of a session is id0 + j, scalars mod N, b = 0 mod N gives infinity), with
 * b_i * A_s summed from a fixed-base window table of A_s instead of walked by double-and-add.  S is fixed at create; per and
 * id0 are arguments of each call, so one handle serves any number of calls.
 *   Create checks every A_s (VALID as above: x, y >= p and (0, 0) are refused) and builds the tables of the good sessions ON
 *   THE DEVICE, on the ctx stream: one lane per session walks the 252 doublings, one lane per (session, window) fills the 15
 *   entries of a window and converts them with one inversion.  A handle holds 61 440 bytes of device memory per session
 *   (S * 61 440 + S * 4); while create runs, a workspace of 6 144 bytes per session and 61 440 bytes for each of up to 1 024
 *   sessions is held as well and freed before create returns.  A BAD SESSION does not make create fail: the handle remembers
 *   it, gc_co_multi_base_info reports the count and the lowest one (all ones: none), and every decrypt gives its OTs zero
 *   labels, counts it once in status words 2 and 3 and does not count its OTs as bad points.  Create is synchronous and not
 *   allowed between gc_ctx_capture_begin and _end (GC_E_ARG).  _create_dev reads d_A (S gc_p256_point in device memory,
 *   16-byte aligned) behind what is queued on the ctx stream.  S = 0, a NULL ctx or pointer, or an S * 61 440 that does not
 *   fit size_t: NULL and *status = GC_E_ARG; allocation failure: NULL and GC_E_NOMEM (status may be NULL).  Several handles may
 *   live on one ctx; free them before the ctx.
 *   Decrypt, _dev form: asynchronous on the ctx stream, one kernel; d_status is the four uint64 of the gc_co_multi_*_dev
 *   calls, reset by the call itself on the stream to {0, ~0, 0, ~0}.  Host form: synchronous, staged; a bad session returns
 *   GC_E_POINT with *bad_session = the lowest one (bad_session may be NULL) and every good label is written all the same.
 *   per = 0: GC_OK, nothing written, the status block included.  A NULL handle, a NULL array with S * per > 0, or an
 *   S * per * 64 that does not fit size_t: GC_E_ARG.
 * There is no choices call: gc_co_multi_receiver_choices reads G's table already.  The tables are indexed by digits of b_i
 * (as the AES tables are by secret bytes); a caller who does not want that keeps gc_co_multi_receiver_decrypt. */
typedef struct gc_co_multi_base gc_co_multi_base;
gc_co_multi_base *gc_co_multi_base_create(gc_ctx *, const gc_p256_point *A, size_t S, int *status);
gc_co_multi_base *gc_co_multi_base_create_dev(gc_ctx *, const void *d_A, size_t S, int *status);
void gc_co_multi_base_free(gc_co_multi_base *); /* waits for the ctx stream first; NULL is a no-op */
int gc_co_multi_base_info(const gc_co_multi_base *, size_t *S, size_t *bad_sessions, size_t *lowest_bad);
int gc_co_multi_base_decrypt(gc_co_multi_base *, const uint8_t *scalars, const uint8_t *choice, const uint8_t *ct, size_t per,
                             uint64_t id0, gc_label *labels_out, size_t *bad_session);
int gc_co_multi_base_decrypt_dev(gc_co_multi_base *, const void *d_scalars, const void *d_choice, const void *d_ct, size_t per,
                                 uint64_t id0, void *d_labels_out, void *d_status);

/* ------------------------------------------------------------------------------------------
 * IKNP extension and COT pads for several sessions per call (ot/iknp.go:197-226, ot/iknp.go:468-511, ot/cot.go:136-235; additive)
 * S sessions of `per` OTs each in one call and one kernel: S instances of a two-party run whose base OTs came out of the
 * gc_co_multi_* calls.  Byte for byte, session s of a multi call is gc_iknp_receive / gc_iknp_send / gc_cot_send_pads /
 * gc_cot_receive_unpad on that session alone.  Conventions are those of gc_co_multi_*: session-major (OT j of session s is
 * element s * per + j of every per-OT array), the session constants are arrays, a _dev form takes device pointers for EVERY
 * array (16-byte aligned) and is asynchronous on the ctx stream with one kernel per call, a host form takes host pointers
 * and is synchronous and staged.  Sessions of unequal length and ROT are not offered.  The KOS check of the
 * malicious variant over these arrays is gc_kos_multi_* below, bit-COT on the same handle gc_iknp_multi_*_bits* behind it.
 *   The handle holds copies of the base labels in device memory (sender: delta [S] and k0 [S][128], 2 KiB + 16 bytes per
 *   session; receiver: base [S][128] gc_wire, 4 KiB per session) and no round keys: the kernel expands a column's key in the
 *   lane.  It holds ONE stream position: sessions of equal length advance in lock step, every call advances it by what
 *   gc_iknp_receive advances its own for `per` OTs, and a handle serves any number of calls.  _create_dev copies behind what
 *   is queued on the ctx stream, so d_k0 may be the d_labels_out of gc_co_multi_receiver_decrypt_dev /
 *   gc_co_multi_base_decrypt_dev at per = 128 (and d_base the d_wires of gc_co_multi_sender_encrypt_dev); the host forms of
 *   create are synchronous.  Several handles may live on one ctx; free them before the ctx.
 *   Layouts: u of session s is at byte s * gc_iknp_u_bytes(per), inside a session as gc_iknp_receive has it; the packed
 *   choice bits of session s (_dev form) are at byte s * 64 * ceil(per / 512), LSB first, zero-padded to whole chunks of 64
 *   bytes.  The padding is READ: the kernel loads a chunk's choice bytes as 16-byte words whatever the chunk's length, so
 *   d_choice_packed must be 16-byte aligned and hold all S * 64 * ceil(per / 512) bytes (gc_iknp_receive_dev reads a
 *   ragged chunk byte by byte and asks for less); what the padding holds does not reach any output.  The host form takes one byte per OT, [S][per]; labels are [S][per].  gc_cot_multi_*: seed and delta [S], data /
 *   flags / result [S][per], wires [S][per] gc_wire, out / sent [S][per][2] gc_label; the MITCCRH key index restarts at 0 in
 *   every session.
 *   Errors: per = 0 returns GC_OK and writes nothing (the position stays).  S = 0, a NULL handle, ctx or array, the wrong
 *   role, a u_len other than S * gc_iknp_u_bytes(per), or a size that does not fit size_t: GC_E_ARG (create: NULL and
 *   *status, which may be NULL).  Create and every gc_iknp_multi_receive / _send call, _dev or not, return GC_E_ARG between
 *   gc_ctx_capture_begin and _end (the position is a kernel argument); gc_cot_multi_*_dev may be captured.  Allocation
 *   failure: GC_E_NOMEM.  GC_IKNP_GENERIC=1 has the meaning it has for gc_iknp_*. */
typedef struct gc_iknp_multi gc_iknp_multi;
gc_iknp_multi *gc_iknp_multi_sender_create(gc_ctx *, const gc_label *delta, const gc_label *k0, size_t S, int *status);
gc_iknp_multi *gc_iknp_multi_sender_create_dev(gc_ctx *, const void *d_delta, const void *d_k0, size_t S, int *status);
gc_iknp_multi *gc_iknp_multi_receiver_create(gc_ctx *, const gc_wire *base, size_t S, int *status);
gc_iknp_multi *gc_iknp_multi_receiver_create_dev(gc_ctx *, const void *d_base, size_t S, int *status);
void gc_iknp_multi_free(gc_iknp_multi *); /* waits for the ctx stream first; NULL is a no-op */
int gc_iknp_multi_info(const gc_iknp_multi *, size_t *S, int *receiver, uint64_t *pos);
int gc_iknp_multi_receive(gc_iknp_multi *, const uint8_t *choice, size_t per, uint8_t *u_out, gc_label *labels_out);
int gc_iknp_multi_send(gc_iknp_multi *, const uint8_t *u_in, size_t u_len, size_t per, gc_label *labels_out);
int gc_iknp_multi_receive_dev(gc_iknp_multi *, const void *d_choice_packed, size_t per, void *d_u_out, void *d_labels_out);
int gc_iknp_multi_send_dev(gc_iknp_multi *, const void *d_u_in, size_t per, void *d_labels_out);
int gc_cot_multi_send_pads(gc_ctx *, const gc_label *seed, const gc_label *delta, const gc_label *data, const gc_wire *wires,
                           size_t S, size_t per, gc_label *out);
int gc_cot_multi_send_pads_dev(gc_ctx *, const void *d_seed, const void *d_delta, const void *d_data, const void *d_wires,
                               size_t S, size_t per, void *d_out);
int gc_cot_multi_receive_unpad(gc_ctx *, const gc_label *seed, const uint8_t *flags, const gc_label *sent, gc_label *result,
                               size_t S, size_t per);
int gc_cot_multi_receive_unpad_dev(gc_ctx *, const void *d_seed, const void *d_flags, const void *d_sent, void *d_result,
                                   size_t S, size_t per);

/* ------------------------------------------------------------------------------------------
 * KOS consistency check for several sessions per call (ot/iknp.go:129-194, ot/iknp.go:364-466, ot/gf128.go:14-27; additive)
 * The tags and the check of the
 * malicious variant for the S sessions of a gc_iknp_multi handle, one kernel per call.  Byte for byte, session s of a multi
 * call is gc_kos_receiver_tags / gc_kos_sender_check on that session alone: chi_i is label i of the AES-128-CTR stream keyed
 * by seed2[s], indices 0 .. per-1 go with result[s][.] and per .. per+255 with choice_vec[s][.]; the index restarts in every
 * session and goes on at per, not at a padded length.
 *   Layouts, session-major: seed2 and delta [S]; result [S][per]; choice_vec [S][256]; tags [S][3] gc_label in the order
 *   x, t0, t1.  Host forms take one byte per choice, b [S][per] and bcv [S][256].  _dev forms take the packed buffers the
 *   extension consumed: d_choice_packed is the buffer of gc_iknp_multi_receive_dev at this `per` (session s at byte
 *   s * 64 * ceil(per / 512), LSB first), d_bcv_packed that of the call at per = 256 (64 bytes per session), d_result and
 *   d_choice_vec the d_labels_out of those two calls.  Only the bytes that hold choice bits are read: what the padding holds
 *   reaches no output.  d_ok is [S] bytes, 1 = the check passed; d_status is two uint64 {failed sessions, lowest failing
 *   session (all ones: none)}, reset on the stream by the call as the gc_co_*_dev status blocks are.
 *   The host form of the check returns GC_OK whether or not sessions fail (as gc_kos_sender_check does with *ok = 0) and
 *   writes ok_out [S] and *bad_session (the lowest failing session, (size_t)-1 for none); either may be NULL, not both.
 *   Sizes: per = 0 is valid and sums over the choice vector alone (the per-OT arrays may then be NULL); S = 0 returns GC_OK
 *   and writes nothing.  GC_E_ARG: a NULL ctx, a NULL array that is needed, a device pointer to labels (d_seed2, d_result,
 *   d_choice_vec, d_delta, d_tags, d_tags_out) that is not 16-byte aligned or a d_status that is not 8-byte aligned, a size
 *   that does not fit size_t, a host form between gc_ctx_capture_begin and _end.
 *   The _dev forms are asynchronous on the ctx stream, allocate nothing, wait for nothing, copy nothing to the host and
 *   carry no stream position: they may be captured.  Host forms are synchronous and staged.
 *   A team of lanes owns a session: one wave up to per + 256 = 1 024 labels, a workgroup above.  Sessions so long and so few
 *   that S workgroups cannot fill the device are the ground of the one-session gc_kos_*_dev, which spreads ONE session over
 *   the whole grid; there is no split-session form here. */
int gc_kos_multi_receiver_tags(gc_ctx *, const gc_label *seed2, const gc_label *result, const uint8_t *b,
                               const gc_label *choice_vec, const uint8_t *bcv, size_t S, size_t per, gc_label *tags_out);
int gc_kos_multi_receiver_tags_dev(gc_ctx *, const void *d_seed2, const void *d_result, const void *d_choice_packed,
                                   const void *d_choice_vec, const void *d_bcv_packed, size_t S, size_t per, void *d_tags_out);
int gc_kos_multi_sender_check(gc_ctx *, const gc_label *seed2, const gc_label *result, const gc_label *choice_vec,
                              const gc_label *delta, const gc_label *tags, size_t S, size_t per, uint8_t *ok_out,
                              size_t *bad_session);
int gc_kos_multi_sender_check_dev(gc_ctx *, const void *d_seed2, const void *d_result, const void *d_choice_vec,
                                  const void *d_delta, const void *d_tags, size_t S, size_t per, void *d_ok, void *d_status);

/* ------------------------------------------------------------------------------------------
 * Bit-COT for several sessions per call, and a GMW triple batch over all peers (ot/iknp.go:259-310, ot/iknp.go:554-620,
 * gmw/triples.go:287-466; additive)
 * ReceiveBits / SendBits on the S sessions of a gc_iknp_multi handle, one kernel per call.  Byte for byte, session s is
 * gc_iknp_receive_bits / gc_iknp_send_bits on that session alone from the same stream position; the handle's position
 * advances as it does for the label calls at `per`, and bit calls and label calls on one handle may be mixed.  With
 * W = ceil(per / 64):
 *   result  u64 [S][W]: bit i of session s is bit i % 64 of word s * W + i / 64.  Every one of the S * W words is written,
 *           with zero in the bits at and behind `per`.
 *   u       as for gc_iknp_multi_receive_dev / _send_dev: S * gc_iknp_u_bytes(per) bytes.  The sender reads column 0 of a
 *           chunk only (its first ceil(rows / 8) bytes), and only for sessions whose delta has bit 0 set; the host form
 *           uploads nothing else.
 *   choices u64 words; session s reads W words from word s * choice_stride.  choice_stride = 0: ONE vector of W words for
 *           every session (a party's b in a triple batch).  Otherwise choice_stride >= W.  No byte outside those words is
 *           read, and there is no padding contract.  As in gc_iknp_receive_bits the choice words enter u whole or not at
 *           all: a chunk of r rows folds in floor(ceil(r / 8) / 8) words, so the choice bits of a trailing partial word do
 *           not reach u (iknp.go:577-592).
 *   Errors: per = 0 returns GC_OK and does nothing.  GC_E_ARG with the position unchanged: the wrong role, a NULL handle,
 *   NULL arrays with per > 0, a choice_stride in (0, W), a u_len other than S * gc_iknp_u_bytes(per), a size that does not
 *   fit size_t, a call between gc_ctx_capture_begin and _end.
 *   The _dev forms take device pointers (d_u_*: 16-byte aligned, d_choices / d_result: 8), allocate nothing, wait for
 *   nothing, use no workspace and run one kernel on the ctx stream.  The host forms are synchronous and staged.
 *   GC_IKNP_GENERIC=1 has the meaning it has for gc_iknp_*.
 * gc_gmw_triples_multi_*: the local words of tripleBatch for the S peer sessions at once, one kernel each, asynchronous on
 * the ctx stream (sender_u: the stream of the handle's ctx); all arrays are device u64, [S][words] unless noted.
 *   sender_u       u_s = a ^ (Delta_s.Bit(0) ? ~0 : 0); a is [words]; Delta is read from the sender handle's device copy
 *   sender_fold    c ^= XOR over s of (s_s ^ (u_s & v_s)); c is [words]
 *   receiver_fold  c ^= XOR over s of r_s; c is [words]
 *   words = 0 returns GC_OK; S = 0, a NULL ctx / handle / array, a receiver handle, S * words * 8 past size_t: GC_E_ARG. */
int gc_iknp_multi_receive_bits_dev(gc_iknp_multi *, const void *d_choices, size_t choice_stride, size_t per,
                                   void *d_u_out, void *d_result);
int gc_iknp_multi_send_bits_dev(gc_iknp_multi *, const void *d_u_in, size_t per, void *d_result);
int gc_iknp_multi_receive_bits(gc_iknp_multi *, const uint64_t *choices, size_t choice_stride, size_t per,
                               uint8_t *u_out, uint64_t *result);
int gc_iknp_multi_send_bits(gc_iknp_multi *, const uint8_t *u_in, size_t u_len, size_t per, uint64_t *result);
int gc_gmw_triples_multi_sender_u_dev(gc_iknp_multi *sender, const void *d_a, void *d_u, size_t words);
int gc_gmw_triples_multi_sender_fold_dev(gc_ctx *, const void *d_s, const void *d_u, const void *d_v, void *d_c,
                                         size_t S, size_t words);
int gc_gmw_triples_multi_receiver_fold_dev(gc_ctx *, const void *d_r, void *d_c, size_t S, size_t words);

/* ------------------------------------------------------------------------------------------
 * The four rounds of sha2pc for S sessions per call (sha2pc/garbler.go, evaluator.go, encoding.go; additive)
 * Session s of a call is byte for byte what GarblerRound1 / EvaluatorRound2 / GarblerRound3 / EvaluatorRound4 and
 * EncodeRound1 / 2 / 3 give for that session alone.  Randomness is the caller's, in the reference's consumption order: the
 * sender's scalar a and the session id (Round 1), the receiver's scalars (Round 2), the key and then R and the L0 of every
 * input wire (Round 3: d_rnd is that of gc_batch_garble).
 *   Geometry.  A handle serves one 2-party circuit: ng garbler inputs (wires 0 .. ng), ne evaluator inputs (the next ne),
 *   nout outputs, rows = the plan's slab_rows.  Encoded lengths (gc_sha2pc_layout; index 0 .. 2 = Round 1 .. 3):
 *     Round 1   "R1" sid[8] "\x05P-256" Ax[32] Ay[32]                                   80
 *     Round 2   "R2" sid[8] "\x05P-256" ne x X[32], ceil(ne / 8) sign bytes             16 + 32 ne + ceil(ne / 8)
 *     Round 3   "R3" sid[8] key[32], rows labels, ng labels, nout x (L0, L1), ne x (ct0, ct1)
 *                                                                              42 + 16 rows + 16 ng + 32 nout + 32 ne
 *   (sha256xor: 80, 8 240, 707 146; a 32-byte digest).  A DEVICE array of payloads is [S][stride] bytes, 16-byte aligned,
 *   stride a multiple of 16 and >= lead + len; payload s begins at byte `lead` of its slot: 0 for Rounds 1 and 2, 6 for Round
 *   3, which puts its tables at byte 48 and every label of it on a multiple of 16.  A caller sends and receives slot + lead.
 *   The HOST forms take and give packed arrays [S][len].  Per-OT arrays are session-major as in gc_co_multi_*: OT j of
 *   session s is element s * ne + j, with id j.  d_sid is [S][8] bytes (8-byte aligned), d_keys [S][32], d_a [S][32],
 *   d_scalars [S][ne][32], d_A / d_AaInv [S] gc_p256_point, bits one byte each (non-zero: 1), the digest
 *   [S][ceil(nout / 8)] bytes, bit i of the output in bit i % 8 of byte i / 8; all other device arrays 16-byte aligned.
 *   Create.  The handle owns one keyed gc_batch of S instances (schedule 1) and every scratch array of its rounds, and
 *   uploads G's window table if the ctx has none; synchronous, not between gc_ctx_capture_begin and _end.  NULL and *status =
 *   GC_E_ARG with a gc_last_error() text when gc_batch_keyed_supported is 0 for that batch, when ng + ne is not the
 *   circuit's input count (or ne or the output count is 0), or when a size does not fit size_t (S must fit uint32_t).  One
 *   call at a time per handle; free waits for the ctx stream first (free a handle before its circuit and its ctx); NULL is
 *   a no-op.
 *   _dev calls allocate nothing and wait for nothing: a fixed sequence of launches on the ctx stream.
 *   d_verdict: u32 [S] in device memory, written by every call for every session.  0: good.  Otherwise code | index << 8,
 *   the first check the reference would fail:
 *     GC_SHA2PC_MAGIC    wrong magic
 *     GC_SHA2PC_CURVE    curve chunk other than "\x05P-256"
 *     GC_SHA2PC_SESSION  the payload's sid is not the session's own (garbler.go:91, evaluator.go:73)
 *     GC_SHA2PC_SETUP    a = 0 mod N, or an A / AaInv that is not VALID as gc_co_multi_* define it
 *     GC_SHA2PC_POINT    choice point `index` does not decode: X >= p, or x^3 - 3x + b is no square (lowest index)
 *     GC_SHA2PC_LABEL    output label `index` is neither hint (BitFromLabel; lowest index)
 *   in the order Round 2: MAGIC, CURVE, SETUP; Round 3: MAGIC, CURVE, POINT, SESSION, SETUP; Round 4: MAGIC, SESSION,
 *   SETUP, LABEL; Round 1: SETUP.  A bad session gets zero bytes in every output of that call (a payload over its len
 *   bytes, not the slot's padding) and changes nothing in any other session.
 *   Host forms: host pointers, packed payloads, synchronous, staged.  Every good session is written; with a bad session
 *   the call returns GC_E_POINT (POINT; SETUP in the evaluator's calls) or GC_E_ARG (everything else) for the LOWEST bad
 *   session and *bad_session = its number (verdict [S] and bad_session may be NULL).
 *   Not offered: sessions on different circuits in one handle, other curves, Encode*Session (persistence stays in Go). */
typedef struct gc_sha2pc_garbler gc_sha2pc_garbler;
typedef struct gc_sha2pc_evaluator gc_sha2pc_evaluator;
enum {
    GC_SHA2PC_MAGIC = 1,
    GC_SHA2PC_CURVE = 2,
    GC_SHA2PC_SESSION = 3,
    GC_SHA2PC_SETUP = 4,
    GC_SHA2PC_POINT = 5,
    GC_SHA2PC_LABEL = 6
};
gc_sha2pc_garbler *gc_sha2pc_garbler_create(gc_ctx *, gc_circ *, uint32_t ng, uint32_t ne, size_t S, int *status);
gc_sha2pc_evaluator *gc_sha2pc_evaluator_create(gc_ctx *, gc_circ *, uint32_t ng, uint32_t ne, size_t S, int *status);
void gc_sha2pc_garbler_free(gc_sha2pc_garbler *);
void gc_sha2pc_evaluator_free(gc_sha2pc_evaluator *);
/* len[3], lead[3] of Rounds 1 .. 3 and the digest's bytes (any pointer may be NULL); GC_E_ARG as create.  The _plan form
 * needs no device. */
int gc_sha2pc_layout(const gc_circ *, uint32_t ng, uint32_t ne, size_t len[3], size_t lead[3], size_t *digest_bytes);
int gc_sha2pc_layout_plan(const gc_plan *, uint32_t ng, uint32_t ne, size_t len[3], size_t lead[3], size_t *digest_bytes);

int gc_sha2pc_garbler_round1_dev(gc_sha2pc_garbler *, const void *d_a, const void *d_sid, void *d_A_out, void *d_AaInv_out,
                                 void *d_r1_out, size_t stride1, void *d_verdict);
int gc_sha2pc_evaluator_round2_dev(gc_sha2pc_evaluator *, const void *d_r1, size_t stride1, const void *d_scalars,
                                   const void *d_bits, void *d_A_out, void *d_sid_out, void *d_r2_out, size_t stride2,
                                   void *d_verdict);
int gc_sha2pc_garbler_round3_dev(gc_sha2pc_garbler *, const void *d_a, const void *d_AaInv, const void *d_sid,
                                 const void *d_r2, size_t stride2, const void *d_keys, const void *d_rnd, const void *d_bits,
                                 void *d_r3_out, size_t stride3, void *d_verdict);
int gc_sha2pc_evaluator_round4_dev(gc_sha2pc_evaluator *, const void *d_A, const void *d_sid, const void *d_scalars,
                                   const void *d_bits, const void *d_r3, size_t stride3, void *d_digest_out, void *d_verdict);
int gc_sha2pc_garbler_round1(gc_sha2pc_garbler *, const uint8_t *a, const uint8_t *sid, gc_p256_point *A_out,
                             gc_p256_point *AaInv_out, uint8_t *r1_out, uint32_t *verdict, size_t *bad_session);
int gc_sha2pc_evaluator_round2(gc_sha2pc_evaluator *, const uint8_t *r1, const uint8_t *scalars, const uint8_t *bits,
                               gc_p256_point *A_out, uint8_t *sid_out, uint8_t *r2_out, uint32_t *verdict, size_t *bad_session);
int gc_sha2pc_garbler_round3(gc_sha2pc_garbler *, const uint8_t *a, const gc_p256_point *AaInv, const uint8_t *sid,
                             const uint8_t *r2, const uint8_t *keys, const uint8_t *rnd, const uint8_t *bits, uint8_t *r3_out,
                             uint32_t *verdict, size_t *bad_session);
int gc_sha2pc_evaluator_round4(gc_sha2pc_evaluator *, const gc_p256_point *A, const uint8_t *sid, const uint8_t *scalars,
                               const uint8_t *bits, const uint8_t *r3, uint8_t *digest_out, uint32_t *verdict,
                               size_t *bad_session);

/* ------------------------------------------------------------------------------------------
 * Device random streams: AES-CTR draws for S sessions per call (additive)
 * Every call above takes its randomness as a device array.  A gc_rand handle writes such arrays from S seeds: stream s is
 * what a Go host reads from cipher.StreamReader{S: cipher.NewCTR(aes.NewCipher(seed[s]), iv[s]), R: zeros}, the reader it
 * would set as env.Config.Rand: block j of the stream is AES_seed[s](iv[s] + j), the sum taken on the 16-byte big-endian
 * counter, carry through all 16 bytes, wrapping silently.  The engine invents no entropy: the seeds are the caller's, one
 * per session, never reseeded; a handle serves at most 2^64 - 1 bytes per stream.
 *   Create.  seeds [S][keylen] with keylen 16 / 24 / 32, ivs [S][16] or NULL for all-zero IVs (host arrays, or with _dev
 *   device arrays read behind what is queued on the ctx stream).  Expands the S key schedules on the device into arrays the
 *   handle owns; synchronous, not between gc_ctx_capture_begin and _end.  NULL and *status (which may be NULL): GC_E_KEYSIZE
 *   for another keylen, GC_E_ARG for S = 0 or a NULL ctx or seeds, GC_E_NOMEM.  Free waits for the ctx stream first (free a
 *   handle before its ctx); NULL is a no-op.
 *   Position.  The handle holds ONE byte position for all S streams (as gc_iknp_multi: sessions advance in lock step).  A
 *   draw of n bytes advances it by n, and successive draws continue the streams as successive Reads on the Go reader do,
 *   whatever the block boundaries.  gc_rand_seek sets it, gc_rand_info reads it (any pointer may be NULL).
 *   gc_rand_fill_dev: the next nbytes of stream s go to d_out + s * stride, stride >= nbytes; bytes of a slot behind nbytes
 *   are not written.  One launch on the ctx stream; allocates nothing, waits for nothing.  Slots whose position-aligned
 *   blocks fall on multiples of 16 bytes are written in 16-byte words, any other slot bytewise.  The garbler's order
 *   (circuit/garbler.go:47-53, circuit/garble.go:253,272) is two draws on one handle: (32, d_keys, 32), then
 *   (16 (1 + ninputs), d_rnd, 16 (1 + ninputs)): the d_keys and d_rnd of gc_batch_garble_keyed.
 *   gc_rand_fill: the same into a host array (staged, synchronous).
 *   gc_rand_gmw_shares_dev: tripleBatch's draw loop (gmw/triples.go:301-310): for each of `words` draws of 16 bytes,
 *   a[s][i] = BE64(bytes 0..7), b[s][i] = BE64(bytes 8..15), native u64 [S][words] as gc_gmw_triples_local_dev and
 *   gc_gmw_set_triples_dev take them; advances the position by 16 * words and needs a position that is a multiple of 16.
 *   Errors.  nbytes = 0 and words = 0 return GC_OK and do nothing.  GC_E_ARG, the position unchanged: a NULL handle or
 *   array, stride < nbytes, a position that is no multiple of 16 (shares), a position or size past uint64_t / size_t, any
 *   draw on the handle's position between gc_ctx_capture_begin and _end (that position is a kernel argument; the rule of
 *   gc_iknp_multi_*).
 *   Cursors.  The calls with _cur in their name take the positions from the caller instead: d_cur is uint64_t [S] in device
 *   memory, 8-byte aligned and the caller's, d_cur[s] the byte position of stream s.  They read it and advance it on the
 *   device, so sessions may consume different amounts; they allocate nothing, wait for nothing, leave the handle's own
 *   position alone and are legal between gc_ctx_capture_begin and _end: a replayed graph continues every stream where the
 *   array stands.  d_status is uint64_t [2] = {bad sessions, lowest bad session}, 8-byte aligned; the call resets it on the
 *   stream to {0, ~0} and its kernels fill it.  A BAD session's outputs are left untouched, never zeroed, and its cursor
 *   unchanged; the other sessions are served.
 *   gc_rand_cur_set_dev: d_cur[s] = pos for every s.
 *   gc_rand_fill_cur_dev: bytes [cur[s], cur[s] + nbytes) of stream s go to d_out + s * stride, then cur[s] += nbytes; the
 *   slot rules are gc_rand_fill_dev's, decided per slot.  Bad: cur[s] > 2^64 - 1 - nbytes.  Two launches: the fill, then the
 *   advance of the cursors (several workgroups serve one stream and all of them read its cursor).
 *   gc_rand_scalars_cur_dev: for every session `count` successive crand.Int(reader_s, max) draws as Go's crypto/rand makes
 *   them (GenerateCOSenderSetup ot/co_helpers.go:83: one per session; BuildCOChoices ot/co_helpers.go:150-151: per OT).  max is 32 bytes big-endian on the host, 2 <= max < 2^256.  With bitlen = BitLen(max - 1), k = ceil(bitlen / 8) and
 *   b = bitlen % 8 (8 for 0) a candidate is the next k bytes of the stream, the first byte cut to its low b bits, read
 *   big-endian, and is accepted if < max; a rejected candidate consumes k bytes like an accepted one.  d_out [S][count][32]
 *   takes the first `count` accepted candidates of each session, big-endian, zero-padded on the left: the d_a of
 *   gc_co_multi_sender_setup_dev (count = 1), the d_scalars of gc_co_multi_receiver_choices_dev and of the sha2pc rounds.
 *   cur[s] advances by k * (candidates consumed).  A session looks at no more than cap = 4 * count + 256 candidates: that
 *   bound is part of the contract (a candidate is accepted with probability above 1/2; needing more has probability below
 *   2^-90 for every count).  Bad: a session that would need more, and one with cur[s] > 2^64 - 1 - k * cap.  The second test
 *   is conservative: it asks for room for every candidate the session MAY look at, about twice what it will.
 *   gc_rand_fill_cur, gc_rand_scalars_cur: the same on host arrays (staged, synchronous, not inside a capture); cur is read
 *   and written back.  With a bad session they return GC_E_ARG and *bad_session = the lowest one (bad_session may be NULL);
 *   every good session is written and advanced all the same.
 *   Errors of the _cur calls, checked before anything is launched, nothing changed: GC_E_ARG for a NULL handle, array or
 *   d_status, stride < nbytes, a last slot that ends past size_t, S * count * 32 past size_t, a d_cur or d_status that is
 *   not 8-byte aligned, max of 0 (Go panics) or 1 (Go reads nothing).  nbytes = 0 or count = 0: GC_OK, nothing done, the
 *   status included.
 *   Not offered: gc_rand_gmw_shares_dev on cursors, a draw of one very long session by more than one wave, moduli past
 *   256 bits. */
typedef struct gc_rand gc_rand;
gc_rand *gc_rand_create(gc_ctx *, const uint8_t *seeds, size_t keylen, const uint8_t *ivs, size_t S, int *status);
gc_rand *gc_rand_create_dev(gc_ctx *, const void *d_seeds, size_t keylen, const void *d_ivs, size_t S, int *status);
void gc_rand_free(gc_rand *); /* waits for the ctx stream; NULL is a no-op */
int gc_rand_info(const gc_rand *, size_t *S, size_t *keylen, uint64_t *pos);
int gc_rand_seek(gc_rand *, uint64_t pos); /* byte position of every stream */
int gc_rand_fill_dev(gc_rand *, size_t nbytes, void *d_out, size_t stride);
int gc_rand_fill(gc_rand *, size_t nbytes, uint8_t *out, size_t stride); /* host form, staged */
int gc_rand_gmw_shares_dev(gc_rand *, size_t words, void *d_a, void *d_b);
/* d_status: uint64_t[2] = {bad sessions, lowest bad session}; the call resets it on the stream to {0, ~0} and the kernels
 * fill it */
int gc_rand_cur_set_dev(gc_rand *, void *d_cur, uint64_t pos); /* d_cur[s] = pos for every s */
int gc_rand_fill_cur_dev(gc_rand *, void *d_cur, size_t nbytes, void *d_out, size_t stride, void *d_status);
int gc_rand_scalars_cur_dev(gc_rand *, void *d_cur, const uint8_t max[32], size_t count, void *d_out, void *d_status);
/* host forms: staged and synchronous like gc_rand_fill; cur is in/out */
int gc_rand_fill_cur(gc_rand *, uint64_t *cur, size_t nbytes, uint8_t *out, size_t stride, size_t *bad_session);
int gc_rand_scalars_cur(gc_rand *, uint64_t *cur, const uint8_t max[32], size_t count, uint8_t *out, size_t *bad_session);

/* ------------------------------------------------------------------------------------------
 * circuit.Garbler / circuit.Evaluator for S sessions per call: the messages built and read on the device (additive;
 * DESIGN.md §23; circuit/garbler.go:38-180, circuit/evaluator.go:20-157, framing p2p/protocol.go:216-261)
 * Session s of a call is byte for byte what the two drivers write through p2p.Conn for that session alone.  The OT stays
 * the caller's: the handles hand over and take the arrays of gc_co_multi_* / gc_iknp_multi_* / gc_cot_multi_*.  The 8-byte
 * offset / count exchange (garbler.go:119-131, evaluator.go:92-97) and CO's point framing stay in the Go shim.
 *   Geometry.  A handle serves one 2-party circuit and ONE key length: ng garbler inputs (wires 0 .. ng), ne evaluator
 *   inputs (the next ne), nout outputs (the last nout wires), keylen 16, 24 or 32.  Messages per session (gc_yao_layout;
 *   index 0 .. 2 = M1 .. M3):
 *     M1  garbler -> evaluator   BE32(keylen) key | BE32(ngates) | per gate BE32(rows) rows x 16 | ng x 16
 *                                                                       4 + keylen + gc_tables_wire_bytes() + 16 ng
 *     M2  evaluator -> garbler   nout x 16                              16 nout
 *     M3  garbler -> evaluator   BE32(n) | n bytes of result.Bytes()    a slot of 4 + ceil(nout / 8); 4 + n in len3[s]
 *   A label is BE(D0) || BE(D1) (SendLabel).  result.Bytes() is big-endian and minimal, n = 0 for a zero result; output i is
 *   bit i of the integer.  A DEVICE array of messages is [S][stride] bytes, 16-byte aligned, stride a multiple of 16 and >=
 *   the message's length (M3: its slot); a slot's padding is never written.  The HOST forms take and give packed arrays
 *   [S][len]; M3 is packed at slot size with zeros behind a message, and len3 [S] comes with it.
 *   d_keys u8 [S][keylen] (16-byte aligned); d_rnd that of gc_batch_garble_keyed, circuit.Garbler's read order after the
 *   key; d_bits u8 [S][ng], non-zero: 1 (may be NULL when ng = 0); d_wires_out gc_wire [S][ne] and d_labels gc_label [S][ne],
 *   session-major as gc_co_multi_* / gc_cot_multi_* take and give them; d_bits_out u8 [S][ceil(nout / 8)], output i in bit
 *   i % 8 of byte i / 8 (the sha2pc digest layout); d_len3_out u32 [S].
 *   Create.  The handle owns one keyed gc_batch of S instances (schedule 1; gc_yao_*_batch hands it out for
 *   gc_batch_set_keyed_path / _keyed_hbm_form / gc_batch_last_ms, the handle keeps owning it) and every scratch array;
 *   synchronous, not between gc_ctx_capture_begin and _end.  NULL and *status (which may be NULL): GC_E_KEYSIZE for another
 *   keylen; GC_E_ARG with a gc_last_error() text when gc_batch_keyed_supported is 0 for that batch, when ng + ne is not the
 *   circuit's input count, when ne or nout is 0, when M1 does not fit 32 bits or a size does not fit size_t (S must fit
 *   uint32_t).  ng = 0 is allowed: M1 then carries no labels.  One call at a time per handle; free waits for the ctx stream
 *   first (free a handle before its circuit and its ctx); NULL is a no-op.
 *   _dev calls allocate nothing and wait for nothing: a fixed sequence of launches on the ctx stream, legal between
 *   gc_ctx_capture_begin and _end; a replayed send garbles with whatever d_keys, d_rnd and d_bits hold then.
 *     garbler    send       gc_batch_garble_keyed, then M1
 *                ot_wires   the gc_wire of the evaluator's inputs (oti.Send's argument, garbler.go:132)
 *                result     M2 -> BitFromLabel against the handle's output wires -> bits, M3, len3
 *     evaluator  accept     M1 -> the handle's keys, tables and the garbler's labels
 *                eval       the OT's labels, gc_batch_eval_keyed, then M2
 *                result     M3 -> bits
 *   d_verdict: u32 [S] in device memory, written by every call that takes one for every session.  0: good.  Otherwise
 *   code | index << 8 (the index's low 24 bits), the first check that fails:
 *     GC_YAO_KEY     M1's first word is not keylen: a handle serves one key length (the reference takes any aes.NewCipher does)
 *     GC_YAO_GATES   the gate count is not the circuit's (evaluator.go:45-48)
 *     GC_YAO_ROWS    gate `index` is the lowest whose row word is not its op's row count (gc_batch_ingest_tables' rule)
 *     GC_YAO_LABEL   output `index` is the lowest whose label is neither L0 nor L1 (BitFromLabel, helpers.go:18-27)
 *     GC_YAO_LENGTH  M3's n with 4 + n > stride3; any other n is read as a big-endian integer and the bits at index nout
 *                    and above are dropped, as IO.Split does (ioarg.go:51-65)
 *   A bad session gets zero bytes in every output of that call (M3 over its slot bytes, its bits, its len3) and changes
 *   nothing in any other session.  A session that accept found bad stays bad in the handle until the next accept: eval
 *   writes a zero M2 for it and repeats the verdict.
 *   Host forms: host pointers, packed messages, synchronous, staged, not inside a capture.  Every good session is written;
 *   with a bad session the call returns GC_E_ROWS (GATES, ROWS) or GC_E_ARG (every other code) for the LOWEST bad session
 *   and *bad_session = its number (verdict [S] and bad_session may be NULL).
 *   gc_yao_kernel_shape: sessions per workgroup and bytes per piece of the M1 kernels as create would choose them now
 *   (developer aid; either pointer may be NULL).
 *   Not offered: sessions on different circuits or key lengths in one handle, the OT's own messages, Timing. */
typedef struct gc_yao_garbler gc_yao_garbler;
typedef struct gc_yao_evaluator gc_yao_evaluator;
enum {
    GC_YAO_KEY = 1,
    GC_YAO_GATES = 2,
    GC_YAO_ROWS = 3,
    GC_YAO_LABEL = 4,
    GC_YAO_LENGTH = 5
};
gc_yao_garbler *gc_yao_garbler_create(gc_ctx *, gc_circ *, uint32_t ng, uint32_t ne, size_t keylen, size_t S, int *status);
gc_yao_evaluator *gc_yao_evaluator_create(gc_ctx *, gc_circ *, uint32_t ng, uint32_t ne, size_t keylen, size_t S, int *status);
void gc_yao_garbler_free(gc_yao_garbler *);
void gc_yao_evaluator_free(gc_yao_evaluator *);
/* len[3] of M1, M2 and M3's slot; GC_E_KEYSIZE / GC_E_ARG as create.  The _plan form needs no device. */
int gc_yao_layout(const gc_circ *, uint32_t ng, uint32_t ne, size_t keylen, size_t len[3]);
int gc_yao_layout_plan(const gc_plan *, uint32_t ng, uint32_t ne, size_t keylen, size_t len[3]);
int gc_yao_kernel_shape(uint32_t *session_tile, uint32_t *piece_bytes);
gc_batch *gc_yao_garbler_batch(gc_yao_garbler *);
gc_batch *gc_yao_evaluator_batch(gc_yao_evaluator *);

int gc_yao_garbler_send_dev(gc_yao_garbler *, const void *d_keys, const void *d_rnd, const void *d_bits, void *d_m1_out,
                            size_t stride1);
int gc_yao_garbler_ot_wires_dev(gc_yao_garbler *, void *d_wires_out);
int gc_yao_garbler_result_dev(gc_yao_garbler *, const void *d_m2, size_t stride2, void *d_m3_out, size_t stride3,
                              void *d_len3_out, void *d_bits_out, void *d_verdict);
int gc_yao_evaluator_accept_dev(gc_yao_evaluator *, const void *d_m1, size_t stride1, void *d_verdict);
int gc_yao_evaluator_eval_dev(gc_yao_evaluator *, const void *d_labels, void *d_m2_out, size_t stride2, void *d_verdict);
int gc_yao_evaluator_result_dev(gc_yao_evaluator *, const void *d_m3, size_t stride3, void *d_bits_out, void *d_verdict);
int gc_yao_garbler_send(gc_yao_garbler *, const uint8_t *keys, const uint8_t *rnd, const uint8_t *bits, uint8_t *m1_out);
int gc_yao_garbler_ot_wires(gc_yao_garbler *, gc_wire *wires_out);
int gc_yao_garbler_result(gc_yao_garbler *, const uint8_t *m2, uint8_t *m3_out, uint32_t *len3_out, uint8_t *bits_out,
                          uint32_t *verdict, size_t *bad_session);
int gc_yao_evaluator_accept(gc_yao_evaluator *, const uint8_t *m1, uint32_t *verdict, size_t *bad_session);
int gc_yao_evaluator_eval(gc_yao_evaluator *, const gc_label *labels, uint8_t *m2_out, uint32_t *verdict, size_t *bad_session);
int gc_yao_evaluator_result(gc_yao_evaluator *, const uint8_t *m3, uint8_t *bits_out, uint32_t *verdict, size_t *bad_session);

#ifdef __cplusplus
}
#endif
#endif /* GCENGINE_H */
