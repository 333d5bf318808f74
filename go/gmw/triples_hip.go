//go:build gchip

// Package gmw — the local word loops of tripleBatch (triples.go:287-466) on MI355X.
// SOURCE ONLY here (no Go toolchain in the build image); see INTEGRATION.md.
//
// The bit-COT itself runs through gc_iknp_send_bits / gc_iknp_receive_bits (go/ot/iknp_hip.go); the
// vectors u and v are still sent in the clear exactly as the reference sends them.  These calls take
// device words: the shim keeps a, b, c, u and the COT outputs of one batch in gc_dev_alloc buffers.
package gmw

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../mpc_amd/csrc -lgcengine -Wl,-rpath,${SRCDIR}/../../mpc_amd/csrc
#include "gcengine.h"
*/
import "C"

import "unsafe"

// devWords is one batch's vector of uint64 words in device memory.
type devWords struct {
	p     unsafe.Pointer
	words int
}

func newDevWords(words int) (*devWords, error) {
	var st C.int
	p := C.gc_dev_alloc(hipCtx, C.size_t(8*words), &st)
	if p == nil {
		return nil, hipErr(st)
	}
	return &devWords{p: p, words: words}, nil
}

func (d *devWords) free() { C.gc_dev_free(hipCtx, d.p) }

func (d *devWords) upload(src []uint64) error {
	if st := C.gc_dev_upload(hipCtx, d.p, unsafe.Pointer(&src[0]), C.size_t(8*len(src))); st != C.GC_OK {
		return hipErr(st)
	}
	return nil
}

func (d *devWords) download(dst []uint64) error {
	if st := C.gc_dev_download(hipCtx, unsafe.Pointer(&dst[0]), d.p, C.size_t(8*len(dst))); st != C.GC_OK {
		return hipErr(st)
	}
	return nil
}

// tripleLocal: c = a & b (triples.go:312-315)
func tripleLocal(a, b, c *devWords) error {
	if st := C.gc_gmw_triples_local_dev(hipCtx, a.p, b.p, c.p, C.size_t(a.words)); st != C.GC_OK {
		return hipErr(st)
	}
	return nil
}

// tripleSenderU: u = a ^ (Delta.Bit(0) ? ~0 : 0) (triples.go:340-349, 428-435)
func tripleSenderU(deltaBit uint, a, u *devWords) error {
	if st := C.gc_gmw_triples_sender_u_dev(hipCtx, C.uint32_t(deltaBit), a.p, u.p, C.size_t(a.words)); st != C.GC_OK {
		return hipErr(st)
	}
	return nil
}

// tripleSenderFold: c ^= s ^ (u & v) (triples.go:362-364, 445-447)
func tripleSenderFold(s, u, v, c *devWords) error {
	if st := C.gc_gmw_triples_sender_fold_dev(hipCtx, s.p, u.p, v.p, c.p, C.size_t(c.words)); st != C.GC_OK {
		return hipErr(st)
	}
	return nil
}

// tripleReceiverFold: c ^= r (triples.go:387-389, 413-415)
func tripleReceiverFold(r, c *devWords) error {
	if st := C.gc_gmw_triples_receiver_fold_dev(hipCtx, r.p, c.p, C.size_t(c.words)); st != C.GC_OK {
		return hipErr(st)
	}
	return nil
}
