//go:build gchip

package circuit

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../mpc_amd/csrc -lgcengine -Wl,-rpath,${SRCDIR}/../../mpc_amd/csrc
#include "gcengine.h"
*/
import "C"

import (
	"fmt"
	"math/big"
	"unsafe"

	"github.com/markkurossi/mpc/ot"
)

// SOURCE ONLY (no Go toolchain in the build image).  Garbler and Evaluator of this package for S sessions of one circuit per
// call (gcengine.h: gc_yao_*): message s of a call is byte for byte what Garbler (garbler.go:38-180) / Evaluator
// (evaluator.go:20-157) write through p2p.Conn for session s alone.  The host gathers S connections, hands the engine what S
// readers delivered and writes what it gets back to the S connections; the OT between Send and Result stays in package ot
// (ot.CO / ot.COT on the wires of OTWires, or their gc_co_multi_* / gc_cot_multi_* forms), and so do the two words of
// garbler.go:119-131 / evaluator.go:92-97 and CO's point framing.
//
// A failed check of the reference is an error of THAT session: errs[s] is non-nil, its outputs are zero, the other sessions
// are untouched.

// YaoSessionError is a check that session s of a batch call failed.
type YaoSessionError struct {
	Code  int // GC_YAO_*
	Index int // the gate or the output, for GC_YAO_ROWS and GC_YAO_LABEL
}

func (e *YaoSessionError) Error() string {
	switch e.Code {
	case C.GC_YAO_KEY:
		return "key length is not the batch's"
	case C.GC_YAO_GATES:
		return "wrong number of gates"
	case C.GC_YAO_ROWS:
		return fmt.Sprintf("corrupted circuit: gate %d", e.Index)
	case C.GC_YAO_LABEL:
		return fmt.Sprintf("label of output %d matches neither wire label", e.Index)
	}
	return "result does not fit its message"
}

func yaoErrors(v []uint32) []error {
	errs := make([]error, len(v))
	for s, w := range v {
		if w != 0 {
			errs[s] = &YaoSessionError{Code: int(w & 0xff), Index: int(w >> 8)}
		}
	}
	return errs
}

// a host form's status: a bad session is in errs, anything else is the call's error
func yaoStatus(st C.int, v []uint32) ([]error, error) {
	errs := yaoErrors(v)
	if st != C.GC_OK {
		for _, e := range errs {
			if e != nil {
				return errs, nil
			}
		}
		return nil, statusError(st)
	}
	return errs, nil
}

type yaoGeom struct {
	ng, ne, nout, keylen, S int
	len                    [3]int // M1, M2, M3's slot
}

func (c *Circuit) yaoLoad(device int, keylen, S int) (*C.gc_ctx, *C.gc_circ, yaoGeom, error) {
	var st C.int
	g := yaoGeom{ng: int(c.Inputs[0].Type.Bits), ne: int(c.Inputs[1].Type.Bits), nout: c.Outputs.Size(), keylen: keylen, S: S}
	ctx := C.gc_ctx_create(C.int(device), &st)
	if ctx == nil {
		return nil, nil, g, statusError(st)
	}
	circ := C.gc_circ_load(ctx, (*C.gc_gate)(unsafe.Pointer(&c.Gates[0])), C.uint32_t(len(c.Gates)),
		C.uint32_t(c.NumWires), C.uint32_t(c.Inputs.Size()), C.uint32_t(c.Outputs.Size()), &st)
	if circ == nil {
		C.gc_ctx_destroy(ctx)
		return nil, nil, g, statusError(st)
	}
	var ln [3]C.size_t
	if st = C.gc_yao_layout(circ, C.uint32_t(g.ng), C.uint32_t(g.ne), C.size_t(keylen), &ln[0]); st != C.GC_OK {
		C.gc_circ_free(circ)
		C.gc_ctx_destroy(ctx)
		return nil, nil, g, statusError(st)
	}
	g.len = [3]int{int(ln[0]), int(ln[1]), int(ln[2])}
	return ctx, circ, g, nil
}

// YaoGarblerBatch serves S garbler sessions of one circuit per call.  Not safe for concurrent use.
type YaoGarblerBatch struct {
	ctx  *C.gc_ctx
	circ *C.gc_circ
	h    *C.gc_yao_garbler
	g    yaoGeom
}

// YaoEvaluatorBatch serves S evaluator sessions of one circuit per call.  Not safe for concurrent use.
type YaoEvaluatorBatch struct {
	ctx  *C.gc_ctx
	circ *C.gc_circ
	h    *C.gc_yao_evaluator
	g    yaoGeom
}

// NewYaoGarblerBatch loads the circuit on `device` for S sessions with keys of keylen bytes (Garbler draws 32).
func (c *Circuit) NewYaoGarblerBatch(device, keylen, S int) (*YaoGarblerBatch, error) {
	ctx, circ, g, err := c.yaoLoad(device, keylen, S)
	if err != nil {
		return nil, err
	}
	var st C.int
	h := C.gc_yao_garbler_create(ctx, circ, C.uint32_t(g.ng), C.uint32_t(g.ne), C.size_t(keylen), C.size_t(S), &st)
	if h == nil {
		C.gc_circ_free(circ)
		C.gc_ctx_destroy(ctx)
		return nil, statusError(st)
	}
	return &YaoGarblerBatch{ctx: ctx, circ: circ, h: h, g: g}, nil
}

// NewYaoEvaluatorBatch is the evaluator's side of NewYaoGarblerBatch.
func (c *Circuit) NewYaoEvaluatorBatch(device, keylen, S int) (*YaoEvaluatorBatch, error) {
	ctx, circ, g, err := c.yaoLoad(device, keylen, S)
	if err != nil {
		return nil, err
	}
	var st C.int
	h := C.gc_yao_evaluator_create(ctx, circ, C.uint32_t(g.ng), C.uint32_t(g.ne), C.size_t(keylen), C.size_t(S), &st)
	if h == nil {
		C.gc_circ_free(circ)
		C.gc_ctx_destroy(ctx)
		return nil, statusError(st)
	}
	return &YaoEvaluatorBatch{ctx: ctx, circ: circ, h: h, g: g}, nil
}

// Close frees the handle before its circuit and its ctx.
func (b *YaoGarblerBatch) Close() {
	C.gc_yao_garbler_free(b.h)
	C.gc_circ_free(b.circ)
	C.gc_ctx_destroy(b.ctx)
	b.h, b.circ, b.ctx = nil, nil, nil
}

// Close frees the handle before its circuit and its ctx.
func (b *YaoEvaluatorBatch) Close() {
	C.gc_yao_evaluator_free(b.h)
	C.gc_circ_free(b.circ)
	C.gc_ctx_destroy(b.ctx)
	b.h, b.circ, b.ctx = nil, nil, nil
}

func inputBits(inputs []*big.Int, n int) []byte {
	bits := make([]byte, len(inputs)*n+1)
	for s, v := range inputs {
		for i := 0; i < n; i++ {
			bits[s*n+i] = byte(v.Bit(i))
		}
	}
	return bits
}

// Send garbles every session and returns what Garbler writes before the OT (garbler.go:64-102), M1 of session s in
// m1[s].  keys is S x keylen and rnd S x 16 (1 + inputs) bytes: what session s's cfg.GetRandom() delivers, in Garbler's
// read order.
func (b *YaoGarblerBatch) Send(keys, rnd []byte, inputs []*big.Int) ([][]byte, error) {
	g := b.g
	if len(keys) != g.S*g.keylen || len(rnd) != g.S*16*(1+g.ng+g.ne) || len(inputs) != g.S {
		return nil, fmt.Errorf("circuit: YaoGarblerBatch.Send: sizes do not match %d sessions", g.S)
	}
	bits := inputBits(inputs, g.ng)
	flat := make([]byte, g.S*g.len[0])
	st := C.gc_yao_garbler_send(b.h, (*C.uint8_t)(unsafe.Pointer(&keys[0])), (*C.uint8_t)(unsafe.Pointer(&rnd[0])),
		(*C.uint8_t)(unsafe.Pointer(&bits[0])), (*C.uint8_t)(unsafe.Pointer(&flat[0])))
	if st != C.GC_OK {
		return nil, statusError(st)
	}
	m1 := make([][]byte, g.S)
	for s := range m1 {
		m1[s] = flat[s*g.len[0] : (s+1)*g.len[0]]
	}
	return m1, nil
}

// OTWires returns garbled.Wires[offset : offset+count] of every session, session-major: oti.Send's argument (garbler.go:132).
func (b *YaoGarblerBatch) OTWires() ([]ot.Wire, error) {
	w := make([]ot.Wire, b.g.S*b.g.ne)
	if st := C.gc_yao_garbler_ot_wires(b.h, (*C.gc_wire)(unsafe.Pointer(&w[0]))); st != C.GC_OK {
		return nil, statusError(st)
	}
	return w, nil
}

// Result takes the evaluators' output labels (m2[s]: Outputs.Size() x 16 bytes) and returns the result messages
// (garbler.go:166-167) and circ.Outputs.Split(result) of every session.
func (b *YaoGarblerBatch) Result(c *Circuit, m2 [][]byte) (m3 [][]byte, results [][]*big.Int, errs []error, err error) {
	g := b.g
	flat := make([]byte, g.S*g.len[1])
	for s := range m2 {
		copy(flat[s*g.len[1]:(s+1)*g.len[1]], m2[s])
	}
	out, len3, bits, v := make([]byte, g.S*g.len[2]), make([]uint32, g.S), make([]byte, g.S*(g.len[2]-4)), make([]uint32, g.S)
	var bad C.size_t
	st := C.gc_yao_garbler_result(b.h, (*C.uint8_t)(unsafe.Pointer(&flat[0])), (*C.uint8_t)(unsafe.Pointer(&out[0])),
		(*C.uint32_t)(unsafe.Pointer(&len3[0])), (*C.uint8_t)(unsafe.Pointer(&bits[0])), (*C.uint32_t)(unsafe.Pointer(&v[0])), &bad)
	if errs, err = yaoStatus(st, v); err != nil {
		return nil, nil, nil, err
	}
	m3, results = make([][]byte, g.S), make([][]*big.Int, g.S)
	for s := 0; s < g.S; s++ {
		if errs[s] == nil {
			m3[s] = out[s*g.len[2] : s*g.len[2]+int(len3[s])]
			results[s] = c.Outputs.Split(bitsInt(bits[s*(g.len[2]-4) : (s+1)*(g.len[2]-4)]))
		}
	}
	return m3, results, errs, nil
}

// output i in bit i % 8 of byte i / 8 -> the integer Garbler builds with SetBit
func bitsInt(bits []byte) *big.Int {
	be := make([]byte, len(bits))
	for i, v := range bits {
		be[len(bits)-1-i] = v
	}
	return new(big.Int).SetBytes(be)
}

// Accept takes M1 of every session (evaluator.go:31-77): key, tables and the garbler's labels stay on the device.
func (b *YaoEvaluatorBatch) Accept(m1 [][]byte) ([]error, error) {
	g := b.g
	flat := make([]byte, g.S*g.len[0])
	for s := range m1 {
		copy(flat[s*g.len[0]:(s+1)*g.len[0]], m1[s])
	}
	v := make([]uint32, g.S)
	var bad C.size_t
	st := C.gc_yao_evaluator_accept(b.h, (*C.uint8_t)(unsafe.Pointer(&flat[0])), (*C.uint32_t)(unsafe.Pointer(&v[0])), &bad)
	return yaoStatus(st, v)
}

// Eval evaluates every session with the labels oti.Receive delivered (session-major, Inputs[1] bits each) and returns the
// output labels Evaluator sends (evaluator.go:129-139); a session Accept found bad gets zeros and its error again.
func (b *YaoEvaluatorBatch) Eval(labels []ot.Label) ([][]byte, []error, error) {
	g := b.g
	if len(labels) != g.S*g.ne {
		return nil, nil, fmt.Errorf("circuit: YaoEvaluatorBatch.Eval: %d labels for %d sessions", len(labels), g.S)
	}
	flat, v := make([]byte, g.S*g.len[1]), make([]uint32, g.S)
	var bad C.size_t
	st := C.gc_yao_evaluator_eval(b.h, (*C.gc_label)(unsafe.Pointer(&labels[0])), (*C.uint8_t)(unsafe.Pointer(&flat[0])),
		(*C.uint32_t)(unsafe.Pointer(&v[0])), &bad)
	errs, err := yaoStatus(st, v)
	if err != nil {
		return nil, nil, err
	}
	m2 := make([][]byte, g.S)
	for s := range m2 {
		m2[s] = flat[s*g.len[1] : (s+1)*g.len[1]]
	}
	return m2, errs, nil
}

// Result reads the garblers' result messages (evaluator.go:144-156): circ.Outputs.Split(raw) of every session.  A message
// longer than 4 + ceil(Outputs.Size() / 8) bytes does not fit a slot and is that session's error.
func (b *YaoEvaluatorBatch) Result(c *Circuit, m3 [][]byte) ([][]*big.Int, []error, error) {
	g := b.g
	flat, bits, v := make([]byte, g.S*g.len[2]), make([]byte, g.S*(g.len[2]-4)), make([]uint32, g.S)
	for s := range m3 {
		if len(m3[s]) > g.len[2] { // the length word alone: the engine reports it
			copy(flat[s*g.len[2]:s*g.len[2]+4], m3[s][:4])
			continue
		}
		copy(flat[s*g.len[2]:(s+1)*g.len[2]], m3[s])
	}
	var bad C.size_t
	st := C.gc_yao_evaluator_result(b.h, (*C.uint8_t)(unsafe.Pointer(&flat[0])), (*C.uint8_t)(unsafe.Pointer(&bits[0])),
		(*C.uint32_t)(unsafe.Pointer(&v[0])), &bad)
	errs, err := yaoStatus(st, v)
	if err != nil {
		return nil, nil, err
	}
	results := make([][]*big.Int, g.S)
	for s := range results {
		if errs[s] == nil {
			results[s] = c.Outputs.Split(bitsInt(bits[s*(g.len[2]-4) : (s+1)*(g.len[2]-4)]))
		}
	}
	return results, errs, nil
}
