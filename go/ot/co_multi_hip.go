//go:build gchip

package ot

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../mpc_amd/csrc -lgcengine -Wl,-rpath,${SRCDIR}/../../mpc_amd/csrc
#include "gcengine.h"
*/
import "C"

import (
	crand "crypto/rand"
	"fmt"
	"math/big"
	"unsafe"
)

// SOURCE ONLY (no Go toolchain in the build image).  S sessions of (*CO).Send / (*CO).Receive (ot/co.go:263-361) at once:
// cos[s] is the CO of session s with its own IO and its own rand, every session carries the same number of wires, and
// each protocol message of all S sessions costs ONE engine call (gcengine.h: gc_co_multi_*) instead of S.  That is the
// shape of a batch: S runs of apps/garbled or sha2pc, S IKNP set-ups, the 2*(P-1) set-ups of a party of a GMW network.
// A session that is shorter than the others is padded by the caller.
//
// Session s sees on its IO exactly the bytes that sendHIP / receiveHIP of co_hip.go put there, in the same order: the
// scalars are drawn per session, in order, from cos[s].rand with crand.Int as GenerateCOSenderSetup (co_helpers.go:83) and
// BuildCOChoices (:151) draw them, and Go numbers the OTs of every session from 0 (id0 = 0).  Layout: session-major, OT j
// of session s is element s*per + j.

// coMultiBaseMinPer is the session length from which ReceiveMultiHIP decrypts through a gc_co_multi_base handle: the
// smallest measured per at S = 1 024 from which building the tables and decrypting from them took less time than the
// ladder decrypt (profiles/co_multi_base_bench.jsonl, the row named in DESIGN.md section 11).
const coMultiBaseMinPer = 8

func coMultiCheck(cos []*CO, per int, lens func(s int) int) error {
	for s := range cos {
		if lens(s) != per {
			return fmt.Errorf("co multi: session %d has %d OTs, session 0 has %d", s, lens(s), per)
		}
	}
	return nil
}

func coSendPoint(io IO, pt *C.gc_p256_point) error {
	b := (*[64]byte)(unsafe.Pointer(pt))
	if err := io.SendData(new(big.Int).SetBytes(b[:32]).Bytes()); err != nil {
		return err
	}
	return io.SendData(new(big.Int).SetBytes(b[32:]).Bytes())
}

// SendMultiHIP is (*CO).Send of every cos[s] on wires[s].
func SendMultiHIP(ctx *C.gc_ctx, cos []*CO, wires [][]Wire) error {
	S := len(cos)
	if S == 0 || len(wires) != S {
		return fmt.Errorf("co multi: %d sessions, %d wire slices", S, len(wires))
	}
	per := len(wires[0])
	if err := coMultiCheck(cos, per, func(s int) int { return len(wires[s]) }); err != nil {
		return err
	}

	// GenerateCOSenderSetup (co_helpers.go:77-101) of every session: one scalar each, then one call for all A and AaInv
	a := make([]byte, 32*S)
	for s, co := range cos {
		v, err := crand.Int(co.rand, co.curve.Params().N)
		if err != nil {
			return err
		}
		v.FillBytes(a[32*s : 32*s+32])
	}
	A := make([]C.gc_p256_point, S)
	AaInv := make([]C.gc_p256_point, S)
	var badSession C.size_t
	if st := C.gc_co_multi_sender_setup(ctx, (*C.uint8_t)(unsafe.Pointer(&a[0])), C.size_t(S), &A[0], &AaInv[0],
		&badSession); st != C.GC_OK {
		return coErr(st)
	}
	for s, co := range cos {
		if err := coSendPoint(co.io, &A[s]); err != nil {
			return err
		}
		if err := co.io.Flush(); err != nil {
			return err
		}
	}

	// every session's choice points
	points := make([]C.gc_p256_point, S*per+1)
	onCurve := true
	for s, co := range cos {
		for j := 0; j < per; j++ {
			xData, err := co.io.ReceiveData()
			if err != nil {
				return err
			}
			yData, err := co.io.ReceiveData()
			if err != nil {
				return err
			}
			if !coPoint(new(big.Int).SetBytes(xData), new(big.Int).SetBytes(yData), &points[s*per+j]) {
				onCurve = false
			}
		}
	}
	if !onCurve {
		return ErrPointNotOnCurve
	}
	if per == 0 {
		for _, co := range cos {
			if err := co.io.Flush(); err != nil {
				return err
			}
		}
		return nil
	}

	// EncryptCOCiphertexts (co_helpers.go:104-137) of every session
	flat := make([]Wire, 0, S*per)
	for s := range cos {
		flat = append(flat, wires[s]...)
	}
	ct := make([]byte, 32*S*per)
	var bad C.size_t
	st := C.gc_co_multi_sender_encrypt(ctx, (*C.uint8_t)(unsafe.Pointer(&a[0])), &AaInv[0], &points[0],
		(*C.gc_wire)(unsafe.Pointer(&flat[0])), C.size_t(S), C.size_t(per), C.uint64_t(0), (*C.uint8_t)(unsafe.Pointer(&ct[0])),
		&bad, &badSession)
	if st != C.GC_OK {
		return coErr(st) // GC_E_POINT: ErrPointNotOnCurve, as the session of OT `bad` would have returned
	}
	for s, co := range cos {
		for j := 0; j < per; j++ {
			i := s*per + j
			if err := co.io.SendData(ct[32*i : 32*i+16]); err != nil {
				return err
			}
			if err := co.io.SendData(ct[32*i+16 : 32*i+32]); err != nil {
				return err
			}
		}
		if err := co.io.Flush(); err != nil {
			return err
		}
	}
	return nil
}

// ReceiveMultiHIP is (*CO).Receive of every cos[s] on flags[s] into result[s].
func ReceiveMultiHIP(ctx *C.gc_ctx, cos []*CO, flags [][]bool, result [][]Label) error {
	S := len(cos)
	if S == 0 || len(flags) != S || len(result) != S {
		return fmt.Errorf("co multi: %d sessions, %d flag slices, %d result slices", S, len(flags), len(result))
	}
	per := len(flags[0])
	if err := coMultiCheck(cos, per, func(s int) int { return len(flags[s]) }); err != nil {
		return err
	}

	// every sender's A; ensureOnCurve (co_helpers.go:144) is the engine's: an A that is not on the curve is a bad session
	A := make([]C.gc_p256_point, S)
	for s, co := range cos {
		Ax, err := ReceiveBigInt(co.io)
		if err != nil {
			return err
		}
		Ay, err := ReceiveBigInt(co.io)
		if err != nil {
			return err
		}
		if !coPoint(Ax, Ay, &A[s]) {
			return ErrPointNotOnCurve
		}
	}

	// Sessions of coMultiBaseMinPer OTs or more decrypt through a handle whose per-session window tables are built on the
	// device now, while this side still draws its scalars (gcengine.h: gc_co_multi_base_*); shorter ones keep the ladder call
	var base *C.gc_co_multi_base
	if per >= coMultiBaseMinPer {
		var status C.int
		base = C.gc_co_multi_base_create(ctx, &A[0], C.size_t(S), &status)
		if base == nil {
			return coErr(status)
		}
		defer C.gc_co_multi_base_free(base)
	}

	// BuildCOChoices (co_helpers.go:140-177): one crand.Int per OT, in order, from the session's own rand
	n := S * per
	scalars := make([]byte, 32*n+1)
	choice := make([]byte, n+1)
	for s, co := range cos {
		order := co.curve.Params().N
		for j, bit := range flags[s] {
			b, err := crand.Int(co.rand, order)
			if err != nil {
				return err
			}
			i := s*per + j
			b.FillBytes(scalars[32*i : 32*i+32])
			if bit {
				choice[i] = 1
			}
		}
	}
	points := make([]C.gc_p256_point, n+1)
	var badSession C.size_t
	st := C.gc_co_multi_receiver_choices(ctx, &A[0], (*C.uint8_t)(unsafe.Pointer(&scalars[0])),
		(*C.uint8_t)(unsafe.Pointer(&choice[0])), C.size_t(S), C.size_t(per), &points[0], &badSession)
	if st != C.GC_OK {
		return coErr(st)
	}
	for s, co := range cos {
		for j := 0; j < per; j++ {
			if err := coSendPoint(co.io, &points[s*per+j]); err != nil {
				return err
			}
		}
		if err := co.io.Flush(); err != nil {
			return err
		}
	}

	ct := make([]byte, 32*n+1)
	for s, co := range cos {
		for j := 0; j < per; j++ {
			i := s*per + j
			zero, err := co.io.ReceiveData()
			if err != nil {
				return err
			}
			copy(ct[32*i:32*i+16], zero)
			one, err := co.io.ReceiveData()
			if err != nil {
				return err
			}
			copy(ct[32*i+16:32*i+32], one)
		}
	}

	// DecryptCOCiphertexts (co_helpers.go:191-219) of every session
	labels := make([]Label, n+1)
	if base != nil {
		st = C.gc_co_multi_base_decrypt(base, (*C.uint8_t)(unsafe.Pointer(&scalars[0])),
			(*C.uint8_t)(unsafe.Pointer(&choice[0])), (*C.uint8_t)(unsafe.Pointer(&ct[0])), C.size_t(per), C.uint64_t(0),
			(*C.gc_label)(unsafe.Pointer(&labels[0])), &badSession)
	} else {
		st = C.gc_co_multi_receiver_decrypt(ctx, &A[0], (*C.uint8_t)(unsafe.Pointer(&scalars[0])),
			(*C.uint8_t)(unsafe.Pointer(&choice[0])), (*C.uint8_t)(unsafe.Pointer(&ct[0])), C.size_t(S), C.size_t(per),
			C.uint64_t(0), (*C.gc_label)(unsafe.Pointer(&labels[0])), &badSession)
	}
	if st != C.GC_OK {
		return coErr(st)
	}
	for s := range cos {
		if len(result[s]) != per {
			return fmt.Errorf("label count mismatch: session %d got %d want %d", s, per, len(result[s]))
		}
		copy(result[s], labels[s*per:(s+1)*per])
	}
	return nil
}
