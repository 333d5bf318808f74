//go:build gchip

package sha2pc

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../mpc_amd/csrc -lgcengine -Wl,-rpath,${SRCDIR}/../../mpc_amd/csrc
#include "gcengine.h"
*/
import "C"

import (
	"crypto/elliptic"
	crand "crypto/rand"
	"crypto/sha256"
	"errors"
	"fmt"
	"io"
	"unsafe"
)

// SOURCE ONLY (no Go toolchain in the build image).  The four rounds of this package for S sessions per call, each round
// ONE engine call (gcengine.h: gc_sha2pc_*): GarblerRound1Batch, EvaluatorRound2Batch, GarblerRound3Batch,
// EvaluatorRound4Batch work on the ENCODED payloads, which is what a server holds: payload s of a batch call is byte for
// byte EncodeRoundN of what GarblerRound1 / EvaluatorRound2 / GarblerRound3 would return for session s alone, and the
// digest of session s is EvaluatorRound4's.  The randomness of session s is drawn from rngs[s] in the order the
// one-session functions draw it: the scalar a (crand.Int) and 8 bytes of session id in round 1, one scalar per choice in
// round 2, the 32-byte key and then R and the L0 of every input wire in round 3.
//
// A failed check of the reference is an error of THAT session: errs[s] is non-nil and payload s is nil, the other
// sessions are untouched.  Session persistence (EncodeGarblerSession / EncodeEvaluatorSession) works on the sessions below
// as it does on the one-session ones and stays in Go.

const (
	round1Len = 80
	round2Len = 16 + 32*hashInputBitCount + hashInputBitCount/8
)

// BatchSessionError is a check of the reference that session s of a batch call failed.
type BatchSessionError struct {
	Code  int // GC_SHA2PC_*
	Index int // the choice point or output label, for GC_SHA2PC_POINT and GC_SHA2PC_LABEL
}

func (e *BatchSessionError) Error() string {
	switch e.Code {
	case C.GC_SHA2PC_MAGIC:
		return "invalid round magic"
	case C.GC_SHA2PC_CURVE:
		return "sha2pc: curve mismatch"
	case C.GC_SHA2PC_SESSION:
		return "session id mismatch"
	case C.GC_SHA2PC_SETUP:
		return "ot: point not on curve"
	case C.GC_SHA2PC_POINT:
		return fmt.Sprintf("failed to decompress evaluator choice %d", e.Index)
	}
	return fmt.Sprintf("output label %d matches neither hint", e.Index)
}

func verdictErrors(v []uint32) []error {
	errs := make([]error, len(v))
	for s, w := range v {
		if w != 0 {
			errs[s] = &BatchSessionError{Code: int(w & 0xff), Index: int(w >> 8)}
		}
	}
	return errs
}

func statusError(what string, st C.int) error {
	return fmt.Errorf("%s: %s (%s)", what, C.GoString(C.gc_strerror(st)), C.GoString(C.gc_last_error()))
}

// GarblerBatchSession is the GarblerSession of one session of a batch: what round 3 needs of round 1.
type GarblerBatchSession struct {
	SessionID [8]byte
	Scalar    [32]byte
	AaInv     [64]byte
}

// EvaluatorBatchSession is the EvaluatorSession of one session of a batch.
type EvaluatorBatchSession struct {
	SessionID [8]byte
	A         [64]byte
	Scalars   []byte // hashInputBitCount x 32
	Bits      []byte // hashInputBitCount, one byte each
}

// GarblerBatch serves S garbler sessions of sha256xor per call.  Not safe for concurrent use.
type GarblerBatch struct {
	ctx  *C.gc_ctx
	circ *C.gc_circ
	h    *C.gc_sha2pc_garbler
	S    int
	len3 int
}

// EvaluatorBatch serves S evaluator sessions of sha256xor per call.  Not safe for concurrent use.
type EvaluatorBatch struct {
	ctx  *C.gc_ctx
	circ *C.gc_circ
	h    *C.gc_sha2pc_evaluator
	S    int
	len3 int
}

func loadCircuit(device int) (*C.gc_ctx, *C.gc_circ, int, error) {
	var st C.int
	ctx := C.gc_ctx_create(C.int(device), &st)
	if ctx == nil {
		return nil, nil, 0, statusError("gc_ctx_create", st)
	}
	c := sha256xorCircuit
	circ := C.gc_circ_load(ctx, (*C.gc_gate)(unsafe.Pointer(&c.Gates[0])), C.uint32_t(len(c.Gates)),
		C.uint32_t(c.NumWires), C.uint32_t(c.Inputs.Size()), C.uint32_t(c.Outputs.Size()), &st)
	if circ == nil {
		C.gc_ctx_destroy(ctx)
		return nil, nil, 0, statusError("gc_circ_load", st)
	}
	var lens [3]C.size_t
	if st = C.gc_sha2pc_layout(circ, C.uint32_t(hashInputBitCount), C.uint32_t(hashInputBitCount), &lens[0], nil, nil); st != C.GC_OK {
		C.gc_circ_free(circ)
		C.gc_ctx_destroy(ctx)
		return nil, nil, 0, statusError("gc_sha2pc_layout", st)
	}
	return ctx, circ, int(lens[2]), nil
}

// NewGarblerBatch loads sha256xor on `device` and allocates the state of S sessions.
func NewGarblerBatch(device, S int) (*GarblerBatch, error) {
	ctx, circ, len3, err := loadCircuit(device)
	if err != nil {
		return nil, err
	}
	var st C.int
	h := C.gc_sha2pc_garbler_create(ctx, circ, C.uint32_t(hashInputBitCount), C.uint32_t(hashInputBitCount), C.size_t(S), &st)
	if h == nil {
		C.gc_circ_free(circ)
		C.gc_ctx_destroy(ctx)
		return nil, statusError("gc_sha2pc_garbler_create", st)
	}
	return &GarblerBatch{ctx: ctx, circ: circ, h: h, S: S, len3: len3}, nil
}

// NewEvaluatorBatch loads sha256xor on `device` and allocates the state of S sessions.
func NewEvaluatorBatch(device, S int) (*EvaluatorBatch, error) {
	ctx, circ, len3, err := loadCircuit(device)
	if err != nil {
		return nil, err
	}
	var st C.int
	h := C.gc_sha2pc_evaluator_create(ctx, circ, C.uint32_t(hashInputBitCount), C.uint32_t(hashInputBitCount), C.size_t(S), &st)
	if h == nil {
		C.gc_circ_free(circ)
		C.gc_ctx_destroy(ctx)
		return nil, statusError("gc_sha2pc_evaluator_create", st)
	}
	return &EvaluatorBatch{ctx: ctx, circ: circ, h: h, S: S, len3: len3}, nil
}

// Close frees the handle, the circuit and the context.
func (g *GarblerBatch) Close() {
	C.gc_sha2pc_garbler_free(g.h)
	C.gc_circ_free(g.circ)
	C.gc_ctx_destroy(g.ctx)
}

// Close frees the handle, the circuit and the context.
func (e *EvaluatorBatch) Close() {
	C.gc_sha2pc_evaluator_free(e.h)
	C.gc_circ_free(e.circ)
	C.gc_ctx_destroy(e.ctx)
}

// a call's return code: a bad session is reported through the verdicts, anything else is the call's own failure
func batchStatus(what string, st C.int, bad C.size_t) error {
	if st == C.GC_OK || ((st == C.GC_E_ARG || st == C.GC_E_POINT) && bad != ^C.size_t(0)) {
		return nil
	}
	return statusError(what, st)
}

func split(flat []byte, per int, errs []error) [][]byte {
	out := make([][]byte, len(errs))
	for s := range out {
		if errs[s] == nil {
			out[s] = flat[s*per : (s+1)*per]
		}
	}
	return out
}

func p256Only(curve elliptic.Curve) error {
	if curve == nil {
		return errNilCurve
	}
	if curve.Params().Name != "P-256" {
		return errors.New("sha2pc: the batch rounds serve P-256 only")
	}
	return nil
}

// GarblerRound1Batch is GarblerRound1 + EncodeRound1 for every rngs[s].
func (g *GarblerBatch) GarblerRound1Batch(rngs []io.Reader, curve elliptic.Curve) ([][]byte, []*GarblerBatchSession, []error, error) {
	if err := p256Only(curve); err != nil {
		return nil, nil, nil, err
	}
	S := g.S
	if len(rngs) != S {
		return nil, nil, nil, fmt.Errorf("sha2pc: %d readers for %d sessions", len(rngs), S)
	}
	a := make([]byte, 32*S)
	sid := make([]byte, 8*S)
	for s, rng := range rngs {
		if rng == nil {
			return nil, nil, nil, errNilRandomSource
		}
		k, err := crand.Int(rng, curve.Params().N)
		if err != nil {
			return nil, nil, nil, err
		}
		k.FillBytes(a[32*s : 32*s+32])
		if _, err := io.ReadFull(rng, sid[8*s:8*s+8]); err != nil {
			return nil, nil, nil, fmt.Errorf("failed to read session id: %w", err)
		}
	}
	A := make([]C.gc_p256_point, S)
	ainv := make([]C.gc_p256_point, S)
	r1 := make([]byte, round1Len*S)
	v := make([]uint32, S)
	bad := ^C.size_t(0)
	st := C.gc_sha2pc_garbler_round1(g.h, (*C.uint8_t)(unsafe.Pointer(&a[0])), (*C.uint8_t)(unsafe.Pointer(&sid[0])), &A[0], &ainv[0],
		(*C.uint8_t)(unsafe.Pointer(&r1[0])), (*C.uint32_t)(unsafe.Pointer(&v[0])), &bad)
	if err := batchStatus("gc_sha2pc_garbler_round1", st, bad); err != nil {
		return nil, nil, nil, err
	}
	errs := verdictErrors(v)
	sessions := make([]*GarblerBatchSession, S)
	for s := range sessions {
		if errs[s] != nil {
			continue
		}
		ses := &GarblerBatchSession{}
		copy(ses.SessionID[:], sid[8*s:])
		copy(ses.Scalar[:], a[32*s:])
		copy(ses.AaInv[:], (*[64]byte)(unsafe.Pointer(&ainv[s]))[:])
		sessions[s] = ses
	}
	return split(r1, round1Len, errs), sessions, errs, nil
}

// EvaluatorRound2Batch is DecodeRound1 + EvaluatorRound2 + EncodeRound2 for every session.
func (e *EvaluatorBatch) EvaluatorRound2Batch(rngs []io.Reader, curve elliptic.Curve, round1 [][]byte, preimageParts [][sha256.Size]byte) ([][]byte, []*EvaluatorBatchSession, []error, error) {
	if err := p256Only(curve); err != nil {
		return nil, nil, nil, err
	}
	S := e.S
	if len(rngs) != S || len(round1) != S || len(preimageParts) != S {
		return nil, nil, nil, fmt.Errorf("sha2pc: %d readers, %d payloads, %d inputs for %d sessions", len(rngs), len(round1), len(preimageParts), S)
	}
	n := hashInputBitCount
	r1 := make([]byte, round1Len*S)
	scalars := make([]byte, 32*n*S)
	bits := make([]byte, n*S)
	for s := range rngs {
		if rngs[s] == nil {
			return nil, nil, nil, errNilRandomSource
		}
		if len(round1[s]) != round1Len {
			return nil, nil, nil, fmt.Errorf("sha2pc: round1 payload %d has %d bytes", s, len(round1[s]))
		}
		copy(r1[round1Len*s:], round1[s])
		for i, b := range bytesToBitsLittle(preimageParts[s][:]) {
			if b {
				bits[n*s+i] = 1
			}
			k, err := crand.Int(rngs[s], curve.Params().N)
			if err != nil {
				return nil, nil, nil, err
			}
			k.FillBytes(scalars[32*(n*s+i) : 32*(n*s+i)+32])
		}
	}
	A := make([]C.gc_p256_point, S)
	sid := make([]byte, 8*S)
	r2 := make([]byte, round2Len*S)
	v := make([]uint32, S)
	bad := ^C.size_t(0)
	st := C.gc_sha2pc_evaluator_round2(e.h, (*C.uint8_t)(unsafe.Pointer(&r1[0])), (*C.uint8_t)(unsafe.Pointer(&scalars[0])),
		(*C.uint8_t)(unsafe.Pointer(&bits[0])), &A[0], (*C.uint8_t)(unsafe.Pointer(&sid[0])), (*C.uint8_t)(unsafe.Pointer(&r2[0])),
		(*C.uint32_t)(unsafe.Pointer(&v[0])), &bad)
	if err := batchStatus("gc_sha2pc_evaluator_round2", st, bad); err != nil {
		return nil, nil, nil, err
	}
	errs := verdictErrors(v)
	sessions := make([]*EvaluatorBatchSession, S)
	for s := range sessions {
		if errs[s] != nil {
			continue
		}
		ses := &EvaluatorBatchSession{Scalars: scalars[32*n*s : 32*n*(s+1)], Bits: bits[n*s : n*(s+1)]}
		copy(ses.SessionID[:], sid[8*s:])
		copy(ses.A[:], (*[64]byte)(unsafe.Pointer(&A[s]))[:])
		sessions[s] = ses
	}
	return split(r2, round2Len, errs), sessions, errs, nil
}

// GarblerRound3Batch is DecodeRound2 + GarblerRound3 + EncodeRound3 for every session.
func (g *GarblerBatch) GarblerRound3Batch(rngs []io.Reader, curve elliptic.Curve, states []*GarblerBatchSession, preimageParts [][sha256.Size]byte, round2 [][]byte) ([][]byte, []error, error) {
	if err := p256Only(curve); err != nil {
		return nil, nil, err
	}
	S := g.S
	if len(rngs) != S || len(states) != S || len(preimageParts) != S || len(round2) != S {
		return nil, nil, fmt.Errorf("sha2pc: %d readers, %d sessions, %d inputs, %d payloads for %d sessions", len(rngs), len(states), len(preimageParts), len(round2), S)
	}
	n := hashInputBitCount
	per := 16 * (1 + 2*n)
	a := make([]byte, 32*S)
	ainv := make([]C.gc_p256_point, S)
	sid := make([]byte, 8*S)
	r2 := make([]byte, round2Len*S)
	keys := make([]byte, 32*S)
	rnd := make([]byte, per*S)
	bits := make([]byte, n*S)
	for s := range rngs {
		if rngs[s] == nil {
			return nil, nil, errNilRandomSource
		}
		if states[s] == nil || len(round2[s]) != round2Len {
			return nil, nil, fmt.Errorf("sha2pc: invalid garbler session or round2 payload %d", s)
		}
		copy(a[32*s:], states[s].Scalar[:])
		copy((*[64]byte)(unsafe.Pointer(&ainv[s]))[:], states[s].AaInv[:])
		copy(sid[8*s:], states[s].SessionID[:])
		copy(r2[round2Len*s:], round2[s])
		if _, err := io.ReadFull(rngs[s], keys[32*s:32*s+32]); err != nil {
			return nil, nil, fmt.Errorf("failed to read garbling key: %w", err)
		}
		if _, err := io.ReadFull(rngs[s], rnd[per*s:per*(s+1)]); err != nil {
			return nil, nil, err
		}
		for i, b := range bytesToBitsLittle(preimageParts[s][:]) {
			if b {
				bits[n*s+i] = 1
			}
		}
	}
	r3 := make([]byte, g.len3*S)
	v := make([]uint32, S)
	bad := ^C.size_t(0)
	st := C.gc_sha2pc_garbler_round3(g.h, (*C.uint8_t)(unsafe.Pointer(&a[0])), &ainv[0], (*C.uint8_t)(unsafe.Pointer(&sid[0])),
		(*C.uint8_t)(unsafe.Pointer(&r2[0])), (*C.uint8_t)(unsafe.Pointer(&keys[0])), (*C.uint8_t)(unsafe.Pointer(&rnd[0])),
		(*C.uint8_t)(unsafe.Pointer(&bits[0])), (*C.uint8_t)(unsafe.Pointer(&r3[0])), (*C.uint32_t)(unsafe.Pointer(&v[0])), &bad)
	if err := batchStatus("gc_sha2pc_garbler_round3", st, bad); err != nil {
		return nil, nil, err
	}
	errs := verdictErrors(v)
	return split(r3, g.len3, errs), errs, nil
}

// EvaluatorRound4Batch is DecodeRound3 + EvaluatorRound4 for every session.
func (e *EvaluatorBatch) EvaluatorRound4Batch(curve elliptic.Curve, states []*EvaluatorBatchSession, round3 [][]byte) ([][sha256.Size]byte, []error, error) {
	if err := p256Only(curve); err != nil {
		return nil, nil, err
	}
	S := e.S
	if len(states) != S || len(round3) != S {
		return nil, nil, fmt.Errorf("sha2pc: %d sessions, %d payloads for %d sessions", len(states), len(round3), S)
	}
	n := hashInputBitCount
	A := make([]C.gc_p256_point, S)
	sid := make([]byte, 8*S)
	scalars := make([]byte, 32*n*S)
	bits := make([]byte, n*S)
	r3 := make([]byte, e.len3*S)
	for s := range states {
		if states[s] == nil || len(states[s].Scalars) != 32*n || len(states[s].Bits) != n {
			return nil, nil, fmt.Errorf("invalid evaluator state for round 4")
		}
		if len(round3[s]) != e.len3 {
			return nil, nil, fmt.Errorf("sha2pc: round3 payload mismatch: got %d want %d", len(round3[s]), e.len3)
		}
		copy((*[64]byte)(unsafe.Pointer(&A[s]))[:], states[s].A[:])
		copy(sid[8*s:], states[s].SessionID[:])
		copy(scalars[32*n*s:], states[s].Scalars)
		copy(bits[n*s:], states[s].Bits)
		copy(r3[e.len3*s:], round3[s])
	}
	digests := make([][sha256.Size]byte, S)
	v := make([]uint32, S)
	bad := ^C.size_t(0)
	st := C.gc_sha2pc_evaluator_round4(e.h, &A[0], (*C.uint8_t)(unsafe.Pointer(&sid[0])), (*C.uint8_t)(unsafe.Pointer(&scalars[0])),
		(*C.uint8_t)(unsafe.Pointer(&bits[0])), (*C.uint8_t)(unsafe.Pointer(&r3[0])), (*C.uint8_t)(unsafe.Pointer(&digests[0])),
		(*C.uint32_t)(unsafe.Pointer(&v[0])), &bad)
	if err := batchStatus("gc_sha2pc_evaluator_round4", st, bad); err != nil {
		return nil, nil, err
	}
	return digests, verdictErrors(v), nil
}
