//go:build gchip

// Package vole — drop-in bodies of (*Sender).Mul and (*Receiver).Mul (vole/vole.go) on MI355X
// (gcengine.h: gc_vole_*).  SOURCE ONLY here (no Go toolchain in the build image); see INTEGRATION.md.
//
// The IKNP calls (already on the device, go/ot/iknp_hip.go), SendData / ReceiveData / Flush, the length
// checks and their error strings stay the reference's Go, so a Go peer sees the same bytes.  A maintainer
// replaces
//
//	vole.go:44-106   the body of (*Sender).Mul     by   return e.mulHIP(inputs, p)
//	vole.go:136-188  the body of (*Receiver).Mul   by   return e.mulHIP(inputs, p)
//
// The device runs the per-label work: one AES-128 key schedule and two AES-CTR blocks per label, the
// reductions mod p, the product and the sum.  It takes an odd modulus 3 <= p < 2^256; for any other p the
// reference's math/big loops below run instead.
package vole

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../mpc_amd/csrc -lgcengine -Wl,-rpath,${SRCDIR}/../../mpc_amd/csrc
#include "gcengine.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"math/big"
	"unsafe"

	"github.com/markkurossi/mpc/ot"
)

var hipCtx *C.gc_ctx

func hipErr(st C.int) error {
	return fmt.Errorf("gcengine: %s: %s", C.GoString(C.gc_strerror(st)), C.GoString(C.gc_last_error()))
}

func hipContext() (*C.gc_ctx, error) {
	if hipCtx == nil {
		var st C.int
		hipCtx = C.gc_ctx_create(0, &st)
		if hipCtx == nil {
			return nil, hipErr(st)
		}
	}
	return hipCtx, nil
}

var big3 = big.NewInt(3)

// modulusBytes returns p as the 32 big-endian bytes the device takes, or false for a p it refuses
// (even, below 3, or 2^256 and above).
func modulusBytes(p *big.Int) ([]byte, bool) {
	if p.Cmp(big3) < 0 || p.Bit(0) == 0 || p.BitLen() > 256 {
		return nil, false
	}
	return p.FillBytes(make([]byte, 32)), true
}

// mulHIP is the body of (*Sender).Mul (vole.go:43-107).
func (e *Sender) mulHIP(inputs []*big.Int, p *big.Int) ([]*big.Int, error) {
	m := len(inputs)
	if m == 0 {
		return nil, nil
	}

	labels, err := e.iknp.Send(m, false)
	if err != nil {
		return nil, fmt.Errorf("vole: ExpandSend: %w", err)
	}
	if len(labels) != m {
		return nil, fmt.Errorf("vole: ExpandSend returned %d wires, want %d", len(labels), m)
	}

	yb, err := e.conn.ReceiveData()
	if err != nil {
		return nil, fmt.Errorf("vole: MulSender receive y-vector: %w", err)
	}
	if len(yb) != m*32 {
		return nil, fmt.Errorf("vole: MulSender expected %d bytes for y-vector, got %d", m*32, len(yb))
	}

	rs := make([]*big.Int, m)
	var out []byte
	if pb, ok := modulusBytes(p); ok {
		ctx, err := hipContext()
		if err != nil {
			return nil, err
		}
		// x * (y mod p) mod p == (x mod p) * y mod p: an x outside [0, 2^256) is reduced here first
		xb := make([]byte, m*32)
		for i, x := range inputs {
			if x.Sign() < 0 || x.BitLen() > 256 {
				x = new(big.Int).Mod(x, p)
			}
			x.FillBytes(xb[i*32 : i*32+32])
		}
		rb := make([]byte, m*32)
		out = make([]byte, m*32)
		st := C.gc_vole_sender_mul(ctx, (*C.uint8_t)(unsafe.Pointer(&pb[0])),
			(*C.gc_label)(unsafe.Pointer(&labels[0])), (*C.uint8_t)(unsafe.Pointer(&xb[0])),
			(*C.uint8_t)(unsafe.Pointer(&yb[0])), C.size_t(m), (*C.uint8_t)(unsafe.Pointer(&rb[0])),
			(*C.uint8_t)(unsafe.Pointer(&out[0])))
		if st != C.GC_OK {
			return nil, hipErr(st)
		}
		for i := 0; i < m; i++ {
			rs[i] = new(big.Int).SetBytes(rb[i*32 : i*32+32])
		}
	} else {
		// the reference's loops (vole.go:60-97)
		for i := 0; i < m; i++ {
			var ld ot.LabelData
			labels[i].GetData(&ld)
			var pad [32]byte
			prgExpandLabel(ld, &pad)
			rs[i] = new(big.Int).SetBytes(pad[:])
			rs[i].Mod(rs[i], p)
		}
		out = make([]byte, 0, m*32)
		for i := 0; i < m; i++ {
			y := new(big.Int).SetBytes(yb[i*32 : i*32+32])
			y.Mod(y, p)
			tmp := new(big.Int).Mul(inputs[i], y)
			tmp.Mod(tmp, p)
			ui := new(big.Int).Add(rs[i], tmp)
			ui.Mod(ui, p)
			out = append(out, bytes32(ui)...)
		}
	}

	if err := e.conn.SendData(out); err != nil {
		return nil, fmt.Errorf("vole: MulSender send u-vector: %w", err)
	}
	if err := e.conn.Flush(); err != nil {
		return nil, fmt.Errorf("vole: MulSender flush u-vector: %w", err)
	}
	return rs, nil
}

// mulHIP is the body of (*Receiver).Mul (vole.go:134-189).
func (e *Receiver) mulHIP(inputs []*big.Int, p *big.Int) ([]*big.Int, error) {
	if e == nil {
		return nil, errors.New("vole: nil Ext")
	}
	m := len(inputs)
	if m == 0 {
		return nil, nil
	}

	flags := make([]bool, m)
	labels := make([]ot.Label, m)
	err := e.iknp.Receive(flags, labels, false)
	if err != nil {
		return nil, fmt.Errorf("vole: ExpandReceive: %w", err)
	}
	if len(labels) != m {
		return nil, fmt.Errorf("vole: ExpandReceive returned %d labels, want %d", len(labels), m)
	}

	// bytes32 as the reference calls it: |y| for a negative y, a panic for y >= 2^256
	outY := make([]byte, 0, m*32)
	for i := 0; i < m; i++ {
		outY = append(outY, bytes32(inputs[i])...)
	}
	if err := e.conn.SendData(outY); err != nil {
		return nil, fmt.Errorf("vole: MulReceiver send y-vector: %w", err)
	}
	if err := e.conn.Flush(); err != nil {
		return nil, fmt.Errorf("vole: MulReceiver flush y-vector: %w", err)
	}

	ub, err := e.conn.ReceiveData()
	if err != nil {
		return nil, fmt.Errorf("vole: MulReceiver receive u-vector: %w", err)
	}
	if len(ub) != m*32 {
		return nil, fmt.Errorf("vole: MulReceiver expected %d bytes for u-vector, got %d", m*32, len(ub))
	}
	us := make([]*big.Int, m)
	if pb, ok := modulusBytes(p); ok {
		ctx, err := hipContext()
		if err != nil {
			return nil, err
		}
		uo := make([]byte, m*32)
		st := C.gc_vole_receiver_reduce(ctx, (*C.uint8_t)(unsafe.Pointer(&pb[0])), (*C.uint8_t)(unsafe.Pointer(&ub[0])),
			C.size_t(m), (*C.uint8_t)(unsafe.Pointer(&uo[0])))
		if st != C.GC_OK {
			return nil, hipErr(st)
		}
		for i := 0; i < m; i++ {
			us[i] = new(big.Int).SetBytes(uo[i*32 : i*32+32])
		}
	} else {
		for i := 0; i < m; i++ { // vole.go:182-187
			us[i] = new(big.Int).SetBytes(ub[i*32 : i*32+32])
			us[i].Mod(us[i], p)
		}
	}
	return us, nil
}
