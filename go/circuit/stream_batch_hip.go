//go:build gchip

package circuit

/*
#include "gcengine.h"
*/
import "C"

import (
	"fmt"
	"io"
	"unsafe"

	"github.com/markkurossi/mpc/ot"
)

// SOURCE ONLY (no Go toolchain in the build image).  S sessions of ONE streamed program per call (additive to the reference:
// a host that gathers S concurrent two-party sessions onto one GPU).  Every session runs the same SSA step
// (compiler/ssa/streamer.go:412-524) on the same circuit with the same in[] / out[]; they differ in key, R and labels.  A
// step is one keyed batch pass over S instances; session s's bytes and wires are those of Streaming.Garble
// (circuit/stream_garble.go:161-192) for that session alone.  Keys, random streams, byte streams and OT labels stay in device
// buffers (DevBuf); the host moves the bytes to its S connections.

// StreamingBatch is the garbler's side: NewStreaming + Garble + GetInput for S sessions.
type StreamingBatch struct {
	ctx      *C.gc_ctx
	h        *C.gc_stream_batch
	sessions int
}

// wireIDs is ws as the uint32 array the C calls take (never empty, so that its first element has an address).
func wireIDs(ws []Wire) *C.uint32_t {
	ids := make([]uint32, len(ws)+1)
	for i, w := range ws {
		ids[i] = uint32(w)
	}
	return (*C.uint32_t)(unsafe.Pointer(&ids[0]))
}

// NewStreamingBatch replaces NewStreaming (stream_garble.go:41-75) for `sessions` sessions.  keys: [sessions][keylen] u8,
// rnd: [sessions][1+len(inputs)][16] — per session R, then one L0 per input, as cfg.GetRandom() would deliver them.  ctx is
// a gc_ctx* as an unsafe.Pointer (see NewDevBuf).
func NewStreamingBatch(ctx unsafe.Pointer, sessions int, keys *DevBuf, keylen int, rnd *DevBuf, inputs []Wire) (*StreamingBatch, error) {
	if keys.Size() < sessions*keylen || rnd.Size() < sessions*(1+len(inputs))*16 {
		return nil, fmt.Errorf("NewStreamingBatch: keys or random streams shorter than %d sessions need", sessions)
	}
	var st C.int
	p := wireIDs(inputs)
	h := C.gc_stream_batch_create((*C.gc_ctx)(ctx), C.uint32_t(sessions), keys.Ptr(), C.size_t(keylen), rnd.Ptr(), p,
		C.uint32_t(len(inputs)), &st)
	if h == nil {
		return nil, statusError(st)
	}
	return &StreamingBatch{ctx: (*C.gc_ctx)(ctx), h: h, sessions: sessions}, nil
}

// Close releases the wire store and the cached circuits.
func (s *StreamingBatch) Close() {
	if s.h != nil {
		C.gc_stream_batch_free(s.h)
		s.h = nil
	}
}

// StepBytes is the number of bytes Garble writes for this step — the same for every session (host only).
func StepBytes(c *Circuit, in, out []Wire) int {
	pi := wireIDs(in)
	po := wireIDs(out)
	n := C.gc_stream_batch_step_bytes((*C.gc_gate)(unsafe.Pointer(&c.Gates[0])), C.uint32_t(len(c.Gates)),
		C.uint32_t(c.NumWires), pi, C.uint32_t(len(in)), po, C.uint32_t(len(out)))
	return int(n)
}

// Garble is (*Streaming).Garble(c, in, out) (stream_garble.go:161-192) for every session: session k's bytes land at
// dst.At(off + k*stride), exactly as :391-446 writes them into conn.WriteBuf.  Queued on the ctx stream; the returned byte
// count is known at once.  stride: a multiple of 4 that holds the steps the caller appends.
func (s *StreamingBatch) Garble(c *Circuit, in, out []Wire, dst *DevBuf, off, stride int) (int, error) {
	if len(c.Gates) == 0 {
		return 0, nil
	}
	pi := wireIDs(in)
	po := wireIDs(out)
	var n C.size_t
	st := C.gc_stream_batch_garble(s.h, (*C.gc_gate)(unsafe.Pointer(&c.Gates[0])), C.uint32_t(len(c.Gates)),
		C.uint32_t(c.NumWires), pi, C.uint32_t(len(in)), po, C.uint32_t(len(out)), dst.At(off), C.size_t(stride), &n)
	if st != C.GC_OK {
		return int(n), statusError(st)
	}
	return int(n), nil
}

// GetInput is (*Streaming).GetInput(w) (stream_garble.go:117-119) of every session.
func (s *StreamingBatch) GetInput(w Wire) ([]ot.Wire, error) {
	out := make([]ot.Wire, s.sessions)
	if st := C.gc_stream_batch_get_wire(s.h, C.uint32_t(w), (*C.gc_wire)(unsafe.Pointer(&out[0]))); st != C.GC_OK {
		return nil, statusError(st)
	}
	return out, nil
}

// GatherWires writes both labels of the named wires as ot.Wire [sessions][len(ws)] into dst: what the multi-session COT
// sender (ot.COTMultiSendPads) consumes for the peers' inputs (garbler.go:102-132 per session).
func (s *StreamingBatch) GatherWires(ws []Wire, dst *DevBuf) error {
	if dst.Size() < s.sessions*len(ws)*32 {
		return fmt.Errorf("GatherWires: %d bytes for %d x %d wires", dst.Size(), s.sessions, len(ws))
	}
	p := wireIDs(ws)
	st := C.gc_stream_batch_gather_wires(s.h, p, C.uint32_t(len(ws)), dst.Ptr())
	if st != C.GC_OK {
		return statusError(st)
	}
	return nil
}

// StreamEvalBatch is the evaluator's side: the store of circuit.StreamEval (stream_evaluator.go:29-96) for S sessions.
type StreamEvalBatch struct {
	ctx      *C.gc_ctx
	h        *C.gc_stream_eval_batch
	sessions int
}

// NewStreamEvalBatch replaces NewStreamEval (stream_evaluator.go:37-50) for `sessions` sessions; keys as NewStreamingBatch.
func NewStreamEvalBatch(ctx unsafe.Pointer, sessions int, keys *DevBuf, keylen int) (*StreamEvalBatch, error) {
	if keys.Size() < sessions*keylen {
		return nil, fmt.Errorf("NewStreamEvalBatch: keys shorter than %d sessions need", sessions)
	}
	var st C.int
	h := C.gc_stream_eval_batch_create((*C.gc_ctx)(ctx), C.uint32_t(sessions), keys.Ptr(), C.size_t(keylen), &st)
	if h == nil {
		return nil, statusError(st)
	}
	return &StreamEvalBatch{ctx: (*C.gc_ctx)(ctx), h: h, sessions: sessions}, nil
}

// Close releases the wire store and the cached circuits.
func (e *StreamEvalBatch) Close() {
	if e.h != nil {
		C.gc_stream_eval_batch_free(e.h)
		e.h = nil
	}
}

// SetWires sets the wires ws of every session from labels: ot.Label [sessions][len(ws)] in device memory (the OT results).
func (e *StreamEvalBatch) SetWires(ws []Wire, labels *DevBuf) error {
	if labels.Size() < e.sessions*len(ws)*16 {
		return fmt.Errorf("SetWires: %d bytes for %d x %d labels", labels.Size(), e.sessions, len(ws))
	}
	p := wireIDs(ws)
	st := C.gc_stream_eval_batch_set_wires(e.h, p, C.uint32_t(len(ws)), labels.Ptr())
	if st != C.GC_OK {
		return statusError(st)
	}
	return nil
}

// Get is StreamEval.Get(false, w) (stream_evaluator.go:61-66) of every session.
func (e *StreamEvalBatch) Get(w Wire) ([]ot.Label, error) {
	out := make([]ot.Label, e.sessions)
	if st := C.gc_stream_eval_batch_get_wire(e.h, C.uint32_t(w), (*C.gc_label)(unsafe.Pointer(&out[0]))); st != C.GC_OK {
		return nil, statusError(st)
	}
	return out, nil
}

// EvalBlock is InitCircuit + the gate loop of the OpCircuit case (stream_evaluator.go:269-432) for every session.  ref holds
// one session's block bytes on the host; blocks holds all of them, stride bytes apart from offset off.  bad receives one
// u32 per session: the structure bytes in which its block differs from ref — such a session is run again through
// StreamEval.evalBlock by the caller.  Returns the bytes one block takes.
func (e *StreamEvalBatch) EvalBlock(numGates, numTmpWires, numWires int, ref []byte, blocks *DevBuf, off, stride int, bad *DevBuf) (int, error) {
	if bad.Size() < 4*e.sessions || len(ref) == 0 {
		return 0, fmt.Errorf("EvalBlock: no reference block, or %d bytes for %d counters", bad.Size(), e.sessions)
	}
	var used C.size_t
	st := C.gc_stream_eval_batch_circuit(e.h, C.uint32_t(numGates), C.uint32_t(numTmpWires), C.uint32_t(numWires),
		(*C.uint8_t)(unsafe.Pointer(&ref[0])), C.size_t(len(ref)), blocks.At(off), C.size_t(stride), bad.Ptr(), &used)
	if st != C.GC_OK {
		return 0, statusError(st)
	}
	return int(used), nil
}

// SelectLabels writes the garbler's own input labels (compiler/ssa/streamer.go:79-102: L1 if inputs.Bit(i), else L0) of every
// session into dst as ot.Label [sessions][len(ws)]; bits holds one byte per input, [sessions][len(ws)], non-zero = 1.  Queued.
func (s *StreamingBatch) SelectLabels(ws []Wire, bits, dst *DevBuf) error {
	if bits.Size() < s.sessions*len(ws) || dst.Size() < s.sessions*len(ws)*16 {
		return fmt.Errorf("SelectLabels: %d bits, %d label bytes for %d x %d wires", bits.Size(), dst.Size(), s.sessions, len(ws))
	}
	p := wireIDs(ws)
	if st := C.gc_stream_batch_select_labels_dev(s.h, p, C.uint32_t(len(ws)), bits.Ptr(), dst.Ptr()); st != C.GC_OK {
		return statusError(st)
	}
	return nil
}

// SelectLabelsHost is SelectLabels for host slices: bits [sessions][len(ws)], the labels in the same order.
func (s *StreamingBatch) SelectLabelsHost(ws []Wire, bits []byte) ([]ot.Label, error) {
	if len(ws) == 0 || len(bits) != s.sessions*len(ws) {
		return nil, fmt.Errorf("SelectLabelsHost: %d bits for %d x %d wires", len(bits), s.sessions, len(ws))
	}
	out := make([]ot.Label, len(bits))
	p := wireIDs(ws)
	st := C.gc_stream_batch_select_labels(s.h, p, C.uint32_t(len(ws)), (*C.uint8_t)(unsafe.Pointer(&bits[0])),
		(*C.gc_label)(unsafe.Pointer(&out[0])))
	if st != C.GC_OK {
		return nil, statusError(st)
	}
	return out, nil
}

// Decode is the result loop of streamer.go:563-579 for every session: labels holds ot.Label [sessions][len(ws)] as the peers
// sent them; bitsOut receives 0, 1 or 0xff ("unknown label") per label and bad one u32 per session, its number of 0xff.  Queued.
func (s *StreamingBatch) Decode(ws []Wire, labels, bitsOut, bad *DevBuf) error {
	if labels.Size() < s.sessions*len(ws)*16 || bitsOut.Size() < s.sessions*len(ws) || bad.Size() < 4*s.sessions {
		return fmt.Errorf("Decode: buffers too small for %d x %d labels", s.sessions, len(ws))
	}
	p := wireIDs(ws)
	if st := C.gc_stream_batch_decode_dev(s.h, p, C.uint32_t(len(ws)), labels.Ptr(), bitsOut.Ptr(), bad.Ptr()); st != C.GC_OK {
		return statusError(st)
	}
	return nil
}

// DecodeHost is Decode for host slices; it returns the bits [sessions][len(ws)] and the count of unknown labels per session.
func (s *StreamingBatch) DecodeHost(ws []Wire, labels []ot.Label) ([]byte, []uint32, error) {
	if len(ws) == 0 || len(labels) != s.sessions*len(ws) {
		return nil, nil, fmt.Errorf("DecodeHost: %d labels for %d x %d wires", len(labels), s.sessions, len(ws))
	}
	bits := make([]byte, len(labels))
	bad := make([]uint32, s.sessions)
	p := wireIDs(ws)
	st := C.gc_stream_batch_decode(s.h, p, C.uint32_t(len(ws)), (*C.gc_label)(unsafe.Pointer(&labels[0])),
		(*C.uint8_t)(unsafe.Pointer(&bits[0])), (*C.uint32_t)(unsafe.Pointer(&bad[0])))
	if st != C.GC_OK {
		return nil, nil, statusError(st)
	}
	return bits, bad, nil
}

// ErrWindowsBusy is GC_E_BUSY of (*StreamingBatchOut).Garble: no window is free and nothing has happened.
var ErrWindowsBusy = fmt.Errorf("stream batch: no free output window")

// StreamingBatchOut writes the steps of a StreamingBatch into a ring of windows whose bytes arrive in pinned host memory
// while the next window fills: what conn.WriteBuf is to one session (compiler/ssa/streamer.go:679-693 writes the OpCircuit
// header that Garble takes as prefix).  One goroutine may call Garble / Flush while one other calls Next / Release.
type StreamingBatchOut struct {
	h        *C.gc_stream_batch_out
	sessions int
}

// NewStreamingBatchOut makes nwindows (>= 2) windows of windowBytes per session; Close it before its StreamingBatch.
func NewStreamingBatchOut(s *StreamingBatch, windowBytes, nwindows int) (*StreamingBatchOut, error) {
	var st C.int
	h := C.gc_stream_batch_out_create(s.h, C.size_t(windowBytes), C.uint32_t(nwindows), &st)
	if h == nil {
		return nil, statusError(st)
	}
	return &StreamingBatchOut{h: h, sessions: s.sessions}, nil
}

// NewStreamingBatchOutSplit is NewStreamingBatchOut with the split rule: a step is cut over the windows, so every window but a
// flushed one leaves exactly full and none grows.  A step larger than (nwindows-1) windows is refused.
func NewStreamingBatchOutSplit(s *StreamingBatch, windowBytes, nwindows int) (*StreamingBatchOut, error) {
	var st C.int
	h := C.gc_stream_batch_out_create_split(s.h, C.size_t(windowBytes), C.uint32_t(nwindows), &st)
	if h == nil {
		return nil, statusError(st)
	}
	return &StreamingBatchOut{h: h, sessions: s.sessions}, nil
}

// SplitStats returns the steps that touched more than one window and the serialiser launches so far (zeros on a handle of
// NewStreamingBatchOut).
func (o *StreamingBatchOut) SplitStats() (splitSteps, segments uint64, err error) {
	var a, b C.uint64_t
	if st := C.gc_stream_batch_out_split_stats(o.h, &a, &b); st != C.GC_OK {
		return 0, 0, statusError(st)
	}
	return uint64(a), uint64(b), nil
}

// SetFallback sends circuits loaded from now on that the key table alone keeps out of the keyed scope to the HBM-wire kernels.
func (s *StreamingBatch) SetFallback(on bool) error {
	v := C.int(0)
	if on {
		v = 1
	}
	if st := C.gc_stream_batch_set_fallback(s.h, v); st != C.GC_OK {
		return statusError(st)
	}
	return nil
}

// SetFallback is (*StreamingBatch).SetFallback for the evaluator: EvalBlock, EvalBlockHost and the intake.
func (e *StreamEvalBatch) SetFallback(on bool) error {
	v := C.int(0)
	if on {
		v = 1
	}
	if st := C.gc_stream_eval_batch_set_fallback(e.h, v); st != C.GC_OK {
		return statusError(st)
	}
	return nil
}

// Close waits for the copies in flight and frees the windows.
func (o *StreamingBatchOut) Close() {
	if o.h != nil {
		C.gc_stream_batch_out_free(o.h)
		o.h = nil
	}
}

// Garble queues prefix (at most 64 bytes) and the step's bytes for every session and returns their number per session.
// ErrWindowsBusy: release a window and call again.
func (o *StreamingBatchOut) Garble(prefix []byte, c *Circuit, in, out []Wire) (int, error) {
	if len(c.Gates) == 0 {
		return 0, nil
	}
	pre := append([]byte{}, prefix...)
	pre = append(pre, 0)
	pi := wireIDs(in)
	po := wireIDs(out)
	var n C.size_t
	st := C.gc_stream_batch_out_garble(o.h, (*C.uint8_t)(unsafe.Pointer(&pre[0])), C.size_t(len(prefix)),
		(*C.gc_gate)(unsafe.Pointer(&c.Gates[0])), C.uint32_t(len(c.Gates)), C.uint32_t(c.NumWires), pi, C.uint32_t(len(in)), po,
		C.uint32_t(len(out)), &n)
	if st == C.GC_E_BUSY {
		return 0, ErrWindowsBusy
	}
	if st != C.GC_OK {
		return int(n), statusError(st)
	}
	return int(n), nil
}

// Flush seals the filling window if it holds any byte.
func (o *StreamingBatchOut) Flush() error {
	if st := C.gc_stream_batch_out_flush(o.h); st != C.GC_OK {
		return statusError(st)
	}
	return nil
}

// Next hands out the oldest sealed window, its copy complete: session k's bytes are base[k*stride : k*stride+n].  n == 0:
// nothing is sealed.  The memory is the handle's and valid until Release.
func (o *StreamingBatchOut) Next() (base unsafe.Pointer, stride, n int, err error) {
	var p *C.uint8_t
	var cs, cn C.size_t
	if st := C.gc_stream_batch_out_next(o.h, &p, &cs, &cn); st != C.GC_OK {
		return nil, 0, 0, statusError(st)
	}
	return unsafe.Pointer(p), int(cs), int(cn), nil
}

// Release returns the oldest handed-out window to the ring.
func (o *StreamingBatchOut) Release() error {
	if st := C.gc_stream_batch_out_release(o.h); st != C.GC_OK {
		return statusError(st)
	}
	return nil
}

// Stats returns the windows sealed, the bytes per session, the windows grown and the ErrWindowsBusy answers so far.
func (o *StreamingBatchOut) Stats() (sealed, bytesPerSession, grown, busy uint64, err error) {
	var a, b, c, d C.uint64_t
	if st := C.gc_stream_batch_out_stats(o.h, &a, &b, &c, &d); st != C.GC_OK {
		return 0, 0, 0, 0, statusError(st)
	}
	return uint64(a), uint64(b), uint64(c), uint64(d), nil
}

// EvalBlockHost is EvalBlock with every session's block in host memory: session k's at unsafe.Add(blocks, k*stride), n bytes
// each — a window of the garbler's StreamingBatchOut, or what S connections delivered.  Session refSession's bytes are the
// reference block.  Pinned memory (AllocPinned) is read by DMA and must stay untouched until UploadsWait or Bad returns.
func (e *StreamEvalBatch) EvalBlockHost(numGates, numTmpWires, numWires int, blocks unsafe.Pointer, stride, n, refSession int) (int, error) {
	var used C.size_t
	st := C.gc_stream_eval_batch_circuit_host(e.h, C.uint32_t(numGates), C.uint32_t(numTmpWires), C.uint32_t(numWires),
		(*C.uint8_t)(blocks), C.size_t(stride), C.size_t(n), C.uint32_t(refSession), &used)
	if st != C.GC_OK {
		return 0, statusError(st)
	}
	return int(used), nil
}

// UploadsWait returns when every block handed to EvalBlockHost has left the caller's memory.
func (e *StreamEvalBatch) UploadsWait() error {
	if st := C.gc_stream_eval_batch_uploads_wait(e.h); st != C.GC_OK {
		return statusError(st)
	}
	return nil
}

// Bad waits and returns, per session, the structure bytes that differed from the reference block in any EvalBlockHost so
// far: a session that differed once stays marked and is run again through StreamEval.evalBlock by the caller.
func (e *StreamEvalBatch) Bad() ([]uint32, error) {
	bad := make([]uint32, e.sessions)
	if st := C.gc_stream_eval_batch_bad(e.h, (*C.uint32_t)(unsafe.Pointer(&bad[0]))); st != C.GC_OK {
		return nil, statusError(st)
	}
	return bad, nil
}

// ReturnLabels is the OpReturn handler (stream_evaluator.go:434-461) for every session at once: the active label of each
// wire of ids, labels[k*len(ids)+j] for session k — one label per id, in the order the garbler named them; a wire never set
// gives the zero label, as streaming.Get does on a fresh store.  It waits for the evaluation queued so far.
func (e *StreamEvalBatch) ReturnLabels(ids []Wire) ([]ot.Label, error) {
	if len(ids) == 0 {
		return nil, nil
	}
	labels := make([]ot.Label, e.sessions*len(ids))
	st := C.gc_stream_eval_batch_return_labels(e.h, wireIDs(ids), C.uint32_t(len(ids)), (*C.gc_label)(unsafe.Pointer(&labels[0])))
	if st != C.GC_OK {
		return nil, statusError(st)
	}
	return labels, nil
}

// ReturnLabelsDev leaves the same array in device memory, where StreamingBatch.DecodeDev of a garbler on the same GPU reads
// it; asynchronous.
func (e *StreamEvalBatch) ReturnLabelsDev(ids []Wire, labels *DevBuf) error {
	if labels.Size() < e.sessions*len(ids)*16 {
		return fmt.Errorf("ReturnLabelsDev: the buffer is shorter than %d sessions x %d labels", e.sessions, len(ids))
	}
	if st := C.gc_stream_eval_batch_return_labels_dev(e.h, wireIDs(ids), C.uint32_t(len(ids)), labels.Ptr()); st != C.GC_OK {
		return statusError(st)
	}
	return nil
}

// StreamEvalBatchIn drives a StreamEvalBatch from S connections: it reads what each of them has to give, in chunks that
// respect no step boundary, and hands the chunks to gc_stream_eval_batch_in_feed, which evaluates every complete OpCircuit
// message (the loop of stream_evaluator.go:227-249) and keeps an unfinished one.  The sessions run one program in lock
// step: every reader delivers the same number of bytes per message.
type StreamEvalBatchIn struct {
	e       *StreamEvalBatch
	h       *C.gc_stream_eval_batch_in
	readers []io.Reader
	chunk   []byte // [sessions][chunkBytes], filled up to `have` per session, of which `at` are consumed
	stride  int
	have    int
	at      int
	fed     uint64 // bytes per session that Feed has taken
}

// NewStreamEvalBatchIn wraps one reader per session.  refSession's bytes are the ones the framing is read from;
// maxMessageBytes bounds what the handle keeps of one unfinished message; chunkBytes is how much is read per session and call.
func (e *StreamEvalBatch) NewStreamEvalBatchIn(readers []io.Reader, refSession, maxMessageBytes, chunkBytes int) (*StreamEvalBatchIn, error) {
	if len(readers) != e.sessions || chunkBytes < 4 {
		return nil, fmt.Errorf("NewStreamEvalBatchIn: %d readers for %d sessions, chunks of %d bytes", len(readers), e.sessions, chunkBytes)
	}
	var st C.int
	h := C.gc_stream_eval_batch_in_create(e.h, C.uint32_t(refSession), C.size_t(maxMessageBytes), &st)
	if h == nil {
		return nil, statusError(st)
	}
	return &StreamEvalBatchIn{e: e, h: h, readers: readers, chunk: make([]byte, e.sessions*chunkBytes), stride: chunkBytes}, nil
}

// Close waits for the uploads in flight and frees the intake; close it before its StreamEvalBatch.
func (in *StreamEvalBatchIn) Close() {
	if in.h != nil {
		C.gc_stream_eval_batch_in_free(in.h)
		in.h = nil
	}
}

// Feed hands the next n bytes of every session (session k's at chunk[k*stride:]) to the handle.  taken: the bytes of the
// chunk that were consumed; nextOp: OpCircuit while all of them were, else the op word the feed stopped in front of.
func (in *StreamEvalBatchIn) Feed(chunk []byte, stride, n int) (taken int, nextOp uint32, err error) {
	if n == 0 {
		return 0, uint32(OpCircuit), nil
	}
	var t C.size_t
	var op C.uint32_t
	st := C.gc_stream_eval_batch_in_feed(in.h, (*C.uint8_t)(unsafe.Pointer(&chunk[0])), C.size_t(stride), C.size_t(n), &t, &op)
	in.fed += uint64(t)
	if st != C.GC_OK {
		return int(t), uint32(op), statusError(st)
	}
	return int(t), uint32(op), nil
}

// Stats returns the messages evaluated, their bytes per session, the chunks uploaded and the bytes kept over the feeds.
func (in *StreamEvalBatchIn) Stats() (steps, bytesPerSession, uploads, carried uint64, err error) {
	var a, b, c, d C.uint64_t
	if st := C.gc_stream_eval_batch_in_stats(in.h, &a, &b, &c, &d); st != C.GC_OK {
		return 0, 0, 0, 0, statusError(st)
	}
	return uint64(a), uint64(b), uint64(c), uint64(d), nil
}

// Run reads and feeds until a message that is not OpCircuit stands at the head of every stream, and returns its op.  The
// bytes behind the op word stay with the intake: ReadUint32s reads them.  Every session must deliver as many bytes as the
// reference session does; io.EOF in front of a complete op word is an error.
func (in *StreamEvalBatchIn) Run() (uint32, error) {
	for {
		if in.at == in.have {
			n, err := in.fill()
			if err != nil {
				return 0, err
			}
			in.at, in.have = 0, n
		}
		taken, op, err := in.Feed(in.chunk[in.at:], in.stride, in.have-in.at)
		if err != nil {
			return 0, err
		}
		in.at += taken
		if op == uint32(OpCircuit) {
			continue
		}
		// the word: all four bytes lie in this chunk, or its first ones went with earlier feeds and were dropped there
		_, evaluated, _, _, err := in.Stats()
		if err != nil {
			return 0, err
		}
		in.at += 4 - int(in.fed-evaluated)
		in.fed = evaluated
		return op, nil
	}
}

// fill reads the next chunk of every session: as many bytes as session 0 has to give, at most one chunk.
func (in *StreamEvalBatchIn) fill() (int, error) {
	n, err := in.readers[0].Read(in.chunk[:in.stride])
	if n == 0 {
		if err == nil {
			err = io.ErrNoProgress
		}
		return 0, err
	}
	for k := 1; k < len(in.readers); k++ {
		if _, err := io.ReadFull(in.readers[k], in.chunk[k*in.stride:k*in.stride+n]); err != nil {
			return 0, err
		}
	}
	return n, nil
}

// ReadUint32s reads count big-endian words of every session from behind the stop (the wire ids of OpReturn) and returns
// session 0's; a session whose words differ is an error.
func (in *StreamEvalBatchIn) ReadUint32s(count int) ([]uint32, error) {
	out := make([]uint32, count)
	var word [4]byte
	for i := range out {
		for b := 0; b < 4; b++ {
			if in.at == in.have {
				n, err := in.fill()
				if err != nil {
					return nil, err
				}
				in.at, in.have = 0, n
			}
			word[b] = in.chunk[in.at]
			for k := 1; k < len(in.readers); k++ {
				if in.chunk[k*in.stride+in.at] != word[b] {
					return nil, fmt.Errorf("session %d names other wires than session 0", k)
				}
			}
			in.at++
		}
		out[i] = uint32(word[0])<<24 | uint32(word[1])<<16 | uint32(word[2])<<8 | uint32(word[3])
	}
	return out, nil
}

// Return answers OpReturn for every session: it reads numOutputs wire ids from behind the op word and returns
// labels[k*numOutputs+j], the label session k sends back for the j-th id (behind OpResult, one SendLabel each).
func (in *StreamEvalBatchIn) Return(numOutputs int) ([]ot.Label, error) {
	ids, err := in.ReadUint32s(numOutputs)
	if err != nil {
		return nil, err
	}
	ws := make([]Wire, len(ids))
	for i, id := range ids {
		ws[i] = Wire(id)
	}
	return in.e.ReturnLabels(ws)
}
