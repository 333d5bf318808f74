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

// SOURCE ONLY (no Go toolchain in the build image).  Drop-in bodies of (*CO).Send and (*CO).Receive (ot/co.go:263-361)
// with the per-OT elliptic-curve and SHA-256 work on MI355X (gcengine.h: gc_co_*; the receiver goes through a gc_co_base
// handle, which owns the window table of the session's A).  The scalars are drawn here with
// crand.Int exactly as GenerateCOSenderSetup (co_helpers.go:83) and BuildCOChoices (:151) draw them — one per OT, in
// order, from co.rand — and every SendData / ReceiveData / Flush is the reference's, so a Go peer sees the same bytes.
// A maintainer replaces
//
//	co.go:264-308   the body of (*CO).Send      by   return co.sendHIP(ctx, wires)
//	co.go:313-360   the body of (*CO).Receive   by   return co.receiveHIP(ctx, flags, result)
//
// The device takes P-256 only (co.curve of NewCO).  Points cross as gc_p256_point: big.Int.Bytes() padded to 32 bytes
// on the way in, stripped again on the way out.  A coordinate longer than 32 bytes cannot be a P-256 coordinate:
// ErrPointNotOnCurve, as curve.IsOnCurve would say.

func coErr(st C.int) error {
	if st == C.GC_E_POINT {
		return ErrPointNotOnCurve
	}
	return fmt.Errorf("gcengine: %s: %s", C.GoString(C.gc_strerror(st)), C.GoString(C.gc_last_error()))
}

// coFixed writes v as 32 big-endian bytes; false: v does not fit.
func coFixed(v *big.Int, out []byte) bool {
	if v.Sign() < 0 || v.BitLen() > 256 {
		return false
	}
	v.FillBytes(out)
	return true
}

func coPoint(x, y *big.Int, out *C.gc_p256_point) bool {
	b := (*[64]byte)(unsafe.Pointer(out))
	return coFixed(x, b[:32]) && coFixed(y, b[32:])
}

// sendHIP is the body of (*CO).Send (co.go:263-309).
func (co *CO) sendHIP(ctx *C.gc_ctx, wires []Wire) error {
	// GenerateCOSenderSetup (co_helpers.go:77-101)
	a, err := crand.Int(co.rand, co.curve.Params().N)
	if err != nil {
		return err
	}
	var ab [32]byte
	a.FillBytes(ab[:])
	var A, AaInv C.gc_p256_point
	if st := C.gc_co_sender_setup((*C.uint8_t)(unsafe.Pointer(&ab[0])), &A, &AaInv); st != C.GC_OK {
		return coErr(st)
	}
	Ab := (*[64]byte)(unsafe.Pointer(&A))
	if err := co.io.SendData(new(big.Int).SetBytes(Ab[:32]).Bytes()); err != nil {
		return err
	}
	if err := co.io.SendData(new(big.Int).SetBytes(Ab[32:]).Bytes()); err != nil {
		return err
	}
	if err := co.io.Flush(); err != nil {
		return err
	}

	n := len(wires)
	points := make([]C.gc_p256_point, n)
	onCurve := true
	for i := 0; i < n; i++ {
		xData, err := co.io.ReceiveData()
		if err != nil {
			return err
		}
		x := new(big.Int).SetBytes(xData)
		yData, err := co.io.ReceiveData()
		if err != nil {
			return err
		}
		y := new(big.Int).SetBytes(yData)
		if !coPoint(x, y, &points[i]) {
			onCurve = false
		}
	}
	if !onCurve {
		return ErrPointNotOnCurve
	}
	if n == 0 {
		return co.io.Flush()
	}

	// EncryptCOCiphertexts (co_helpers.go:104-137)
	ct := make([]byte, 32*n)
	var bad C.size_t
	st := C.gc_co_sender_encrypt(ctx, (*C.uint8_t)(unsafe.Pointer(&ab[0])), &AaInv, &points[0],
		(*C.gc_wire)(unsafe.Pointer(&wires[0])), C.size_t(n), C.uint64_t(0), (*C.uint8_t)(unsafe.Pointer(&ct[0])), &bad)
	if st != C.GC_OK {
		return coErr(st)
	}
	for i := 0; i < n; i++ {
		if err := co.io.SendData(ct[32*i : 32*i+16]); err != nil {
			return err
		}
		if err := co.io.SendData(ct[32*i+16 : 32*i+32]); err != nil {
			return err
		}
	}
	return co.io.Flush()
}

// receiveHIP is the body of (*CO).Receive (co.go:312-361).
func (co *CO) receiveHIP(ctx *C.gc_ctx, flags []bool, result []Label) error {
	Ax, err := ReceiveBigInt(co.io)
	if err != nil {
		return err
	}
	Ay, err := ReceiveBigInt(co.io)
	if err != nil {
		return err
	}
	var A C.gc_p256_point
	if !coPoint(Ax, Ay, &A) {
		return ErrPointNotOnCurve
	}
	// The session's handle: A is checked once (ensureOnCurve, co_helpers.go:144) and its fixed-base window table is built
	// and owned by the handle; both receiver calls below sum b*G and b*A from tables instead of walking the ladder.  With
	// the create included the handle is the faster way from a single OT on (DESIGN.md section 11), so it is used for
	// every n.  The deferred free runs on every exit path.
	var st C.int
	base := C.gc_co_base_create(ctx, &A, &st)
	if base == nil {
		return coErr(st)
	}
	defer C.gc_co_base_free(base)

	// BuildCOChoices (co_helpers.go:140-177): one crand.Int per OT, in order
	n := len(flags)
	order := co.curve.Params().N
	scalars := make([]byte, 32*n+1)
	choice := make([]byte, n+1)
	for i, bit := range flags {
		b, err := crand.Int(co.rand, order)
		if err != nil {
			return err
		}
		b.FillBytes(scalars[32*i : 32*i+32])
		if bit {
			choice[i] = 1
		}
	}
	points := make([]C.gc_p256_point, n+1)
	st = C.gc_co_base_choices(base, (*C.uint8_t)(unsafe.Pointer(&scalars[0])), (*C.uint8_t)(unsafe.Pointer(&choice[0])),
		C.size_t(n), &points[0])
	if st != C.GC_OK {
		return coErr(st)
	}
	for i := 0; i < n; i++ {
		pb := (*[64]byte)(unsafe.Pointer(&points[i]))
		if err := co.io.SendData(new(big.Int).SetBytes(pb[:32]).Bytes()); err != nil {
			return err
		}
		if err := co.io.SendData(new(big.Int).SetBytes(pb[32:]).Bytes()); err != nil {
			return err
		}
	}
	if err := co.io.Flush(); err != nil {
		return err
	}

	ct := make([]byte, 32*n+1)
	for i := 0; i < n; i++ {
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

	// DecryptCOCiphertexts (co_helpers.go:191-219)
	labels := make([]Label, n+1)
	st = C.gc_co_base_decrypt(base, (*C.uint8_t)(unsafe.Pointer(&scalars[0])), (*C.uint8_t)(unsafe.Pointer(&choice[0])),
		(*C.uint8_t)(unsafe.Pointer(&ct[0])), C.size_t(n), C.uint64_t(0), (*C.gc_label)(unsafe.Pointer(&labels[0])))
	if st != C.GC_OK {
		return coErr(st)
	}
	if n != len(result) {
		return fmt.Errorf("label count mismatch: got %d want %d", n, len(result))
	}
	copy(result, labels[:n])
	return nil
}
