//go:build gchip

// Package gmw — the local word loops of tripleBatch (triples.go:287-466) on MI355X.
// SOURCE ONLY here (no Go toolchain in the build image); see INTEGRATION.md.
//
// The bit-COT itself runs through gc_iknp_send_bits / gc_iknp_receive_bits (go/ot/iknp_hip.go); the
// vectors u and v are still sent in the clear exactly as the reference sends them.  These calls take
// device words: the shim keeps a, b, c, u and the COT outputs of one batch in gc_dev_alloc buffers.
//
// tripleBatchMulti is the batch over ALL peers: the party's peer sessions sit in one ot.IKNPMulti per role, so the
// batch is one receive-bits call with the shared choice vector b, one send-bits call and three folds, whatever P is.
package gmw

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../mpc_amd/csrc -lgcengine -Wl,-rpath,${SRCDIR}/../../mpc_amd/csrc
#include "gcengine.h"
*/
import "C"

import (
	"unsafe"

	"github.com/markkurossi/mpc/ot"
)

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

// tripleMultiSenderU: u[s] = a ^ (Delta_s.Bit(0) ? ~0 : 0) for every session of snd; Delta stays on the device
func tripleMultiSenderU(snd *ot.IKNPMulti, a, u *devWords) error {
	if st := C.gc_gmw_triples_multi_sender_u_dev((*C.gc_iknp_multi)(snd.Handle()), a.p, u.p, C.size_t(a.words)); st != C.GC_OK {
		return hipErr(st)
	}
	return nil
}

// tripleMultiSenderFold: c ^= XOR over s of (s[s] ^ (u[s] & v[s]))
func tripleMultiSenderFold(s, u, v, c *devWords, sessions int) error {
	if st := C.gc_gmw_triples_multi_sender_fold_dev(hipCtx, s.p, u.p, v.p, c.p, C.size_t(sessions), C.size_t(c.words)); st != C.GC_OK {
		return hipErr(st)
	}
	return nil
}

// tripleMultiReceiverFold: c ^= XOR over s of r[s]
func tripleMultiReceiverFold(r, c *devWords, sessions int) error {
	if st := C.gc_gmw_triples_multi_receiver_fold_dev(hipCtx, r.p, c.p, C.size_t(sessions), C.size_t(c.words)); st != C.GC_OK {
		return hipErr(st)
	}
	return nil
}

// triplePeer is one peer of a batch: its id, the IO of its two IKNP sessions and the offline connection's bit vectors.
// Session k of snd / rcv is peers[k].
type triplePeer struct {
	id         int
	iknpS      ot.IO // the session in which this party is the IKNP sender
	iknpR      ot.IO // ... the receiver
	sendBitvec func([]uint64) error
	recvBitvec func([]uint64) error
}

// tripleBatchMulti is tripleBatch (triples.go:287-466) over all peers at once.  a and b are the party's random words, c
// comes back as its share.  On every peer connection the messages keep the reference's order: for self < peer the
// IKNP sender's term first (:328-389), else the receiver's (:391-448).  That is possible with one device call per role
// because no message depends on a COT output: the u-matrices of ReceiveBits need b alone, u = a ^ Delta needs no COT, and
// the COT words only enter the folds behind the last message.
func tripleBatchMulti(self int, peers []triplePeer, snd, rcv *ot.IKNPMulti, size int, a, b, c []uint64) error {
	S := len(peers)
	words := (size + 63) / 64
	if S == 0 || snd.Sessions() != S || rcv.Sessions() != S || len(a) != words || len(b) != words || len(c) != words {
		panic("tripleBatchMulti: sessions and words")
	}
	ub := ot.UBytes(size)

	// the receiver's term of every peer: one call, b shared (stride 0)
	rBits := make([]uint64, S*words)
	uMine, err := rcv.ReceiveBits(b, 0, size, rBits)
	if err != nil {
		return err
	}

	// u_s = a ^ Delta_s on the device, downloaded to be sent
	dA, err := newDevWords(words)
	if err != nil {
		return err
	}
	defer dA.free()
	dU, err := newDevWords(S * words)
	if err != nil {
		return err
	}
	defer dU.free()
	if err := dA.upload(a); err != nil {
		return err
	}
	if err := tripleMultiSenderU(snd, dA, dU); err != nil {
		return err
	}
	u := make([]uint64, S*words)
	if err := dU.download(u); err != nil {
		return err
	}

	// the messages, peer by peer in the reference's order
	uTheirs := make([]byte, S*ub)
	v := make([]uint64, S*words)
	scratch := make([]uint64, words)
	asSender := func(k int) error { // triples.go:335-359 / :422-443
		p := &peers[k]
		if err := ot.ReceiveU(p.iknpS, uTheirs[k*ub:(k+1)*ub]); err != nil {
			return err
		}
		if err := p.sendBitvec(u[k*words : (k+1)*words]); err != nil {
			return err
		}
		return p.recvBitvec(v[k*words : (k+1)*words])
	}
	asReceiver := func(k int) error { // triples.go:371-384 / :398-411
		p := &peers[k]
		if err := ot.SendU(p.iknpR, uMine[k*ub:(k+1)*ub]); err != nil {
			return err
		}
		if err := p.sendBitvec(b); err != nil {
			return err
		}
		return p.recvBitvec(scratch) // u = a_peer ^ Delta: read and, as in the reference, not used
	}
	for k := range peers {
		first, second := asSender, asReceiver
		if self > peers[k].id {
			first, second = asReceiver, asSender
		}
		if err := first(k); err != nil {
			return err
		}
		if err := second(k); err != nil {
			return err
		}
	}

	// the sender's term of every peer: one call over the u-matrices read above
	sBits := make([]uint64, S*words)
	if err := snd.SendBits(uTheirs, size, sBits); err != nil {
		return err
	}

	// c = a & b ^ XOR_s (s_s ^ (u_s & v_s)) ^ XOR_s r_s
	dB, err := newDevWords(words)
	if err != nil {
		return err
	}
	defer dB.free()
	dC, err := newDevWords(words)
	if err != nil {
		return err
	}
	defer dC.free()
	dS, err := newDevWords(S * words)
	if err != nil {
		return err
	}
	defer dS.free()
	dV, err := newDevWords(S * words)
	if err != nil {
		return err
	}
	defer dV.free()
	if err := dB.upload(b); err != nil {
		return err
	}
	if err := tripleLocal(dA, dB, dC); err != nil {
		return err
	}
	if err := dS.upload(sBits); err != nil {
		return err
	}
	if err := dV.upload(v); err != nil {
		return err
	}
	if err := tripleMultiSenderFold(dS, dU, dV, dC, S); err != nil {
		return err
	}
	if err := dS.upload(rBits); err != nil { // stream order: behind the fold that read s
		return err
	}
	if err := tripleMultiReceiverFold(dS, dC, S); err != nil {
		return err
	}
	return dC.download(c)
}
