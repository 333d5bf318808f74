//go:build gchip

// Package gmw — drop-in body of the online phase of a GMW party on MI355X (gcengine.h: gc_gmw_*).
// SOURCE ONLY here (no Go toolchain in the build image); see INTEGRATION.md.
//
// Replaces the level loop of (*Network).run (network.go:563-618) and the body of andBatchFlush
// (network.go:660-757).  Input sharing, broadcastXORs and the p2p framing stay in Go: with batch = 1 the
// engine's d / e words are the bit vectors SendBitvec2 sends (peer.go:131-163), so the wire bytes are
// unchanged and a Go peer cannot tell the difference.
package gmw

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

	"github.com/markkurossi/mpc/circuit"
)

var hipCtx *C.gc_ctx

func hipErr(st C.int) error {
	return fmt.Errorf("gcengine: %s", C.GoString(C.gc_strerror(st)))
}

// bigWords returns the little-endian uint64 words of x, zero-padded to n words (big.Int.Bits order on
// 64-bit hosts).
func bigWords(x *big.Int, n int) []uint64 {
	out := make([]uint64, n)
	for i, w := range x.Bits() {
		if i < n {
			out[i] = uint64(w)
		}
	}
	return out
}

// runLevelsHIP is the level loop of (*Network).run (network.go:563-618) for one instance: nw.wires holds
// this party's input shares (setWires, network.go:560-561); on return nw.output holds its output shares.
func (nw *Network) runLevelsHIP() error {
	if hipCtx == nil {
		var st C.int
		hipCtx = C.gc_ctx_create(0, &st)
		if hipCtx == nil {
			return hipErr(st)
		}
	}
	gates := nw.circ.Gates
	nin := nw.circ.Inputs.Size()
	nout := nw.circ.Outputs.Size()
	var st C.int
	g := C.gc_gmw_create(hipCtx, (*C.gc_gate)(unsafe.Pointer(&gates[0])), C.uint32_t(len(gates)),
		C.uint32_t(nw.circ.NumWires), C.uint32_t(nin), C.uint32_t(nout), C.uint32_t(len(nw.peers)),
		C.uint32_t(nw.self.id), C.uint32_t(1), &st)
	if g == nil {
		return hipErr(st)
	}
	defer C.gc_gmw_free(g)
	var info C.gc_gmw_info
	if st = C.gc_gmw_get_info(g, &info); st != C.GC_OK {
		return hipErr(st)
	}

	in := bigWords(nw.wires, (nin+63)/64+1)
	if st = C.gc_gmw_set_inputs(g, (*C.uint64_t)(unsafe.Pointer(&in[0]))); st != C.GC_OK {
		return hipErr(st)
	}
	// one pool fetch per AND level, whole words each (TriplePool.Get, triples.go:130-142)
	tw := int(info.triple_words)
	a := make([]uint64, tw+1)
	b := make([]uint64, tw+1)
	c := make([]uint64, tw+1)
	ofs := 0
	levelWords := make([]int, 0, int(info.n_and_levels))
	for _, w := range nw.andLevelWords() {
		nw.Pool.Get(w*64, nw.triples)
		copy(a[ofs:], nw.triples.A[:w])
		copy(b[ofs:], nw.triples.B[:w])
		copy(c[ofs:], nw.triples.C[:w])
		nw.triples.Clear()
		ofs += w
		levelWords = append(levelWords, w)
	}
	if st = C.gc_gmw_set_triples(g, (*C.uint64_t)(unsafe.Pointer(&a[0])), (*C.uint64_t)(unsafe.Pointer(&b[0])),
		(*C.uint64_t)(unsafe.Pointer(&c[0]))); st != C.GC_OK {
		return hipErr(st)
	}

	npeers := len(nw.peers) - 1
	maxw := int(info.max_level_words)
	msg := make([]uint64, 2*maxw+1)
	peerMsgs := make([]uint64, npeers*2*maxw+1)
	for {
		var level C.uint32_t
		var words C.size_t
		st = C.gc_gmw_step(g, (*C.uint64_t)(unsafe.Pointer(&peerMsgs[0])), C.uint32_t(npeers),
			(*C.uint64_t)(unsafe.Pointer(&msg[0])), &level, &words)
		if st != C.GC_OK {
			return hipErr(st)
		}
		w := int(words)
		if w == 0 {
			break
		}
		nw.andBatchCount++
		// broadcastXORs exchanges d and e with every peer (network.go:790-823); the engine XORs them itself,
		// so the received vectors are only collected
		k := 0
		for _, peer := range nw.peers {
			if peer.id == nw.self.id {
				continue
			}
			dR := peerMsgs[k*2*w : k*2*w+w]
			eR := peerMsgs[k*2*w+w : (k+1)*2*w]
			if err := nw.exchangeBitvec2(peer, msg[:w], msg[w:2*w], dR, eR); err != nil {
				return err
			}
			k++
		}
	}
	out := make([]uint64, (nout+63)/64+1)
	if st = C.gc_gmw_get_outputs(g, (*C.uint64_t)(unsafe.Pointer(&out[0]))); st != C.GC_OK {
		return hipErr(st)
	}
	bits := make([]big.Word, len(out))
	for i, w := range out {
		bits[i] = big.Word(w)
	}
	nw.output = new(big.Int).SetBits(bits)
	return nil
}

// exchangeBitvec2 is one peer's leg of broadcastXORs (network.go:800-818): the lower id sends first.
func (nw *Network) exchangeBitvec2(peer *Peer, d, e, dR, eR []uint64) error {
	if nw.self.id < peer.id {
		if err := peer.SendBitvec2(peer.online, d, e); err != nil {
			return err
		}
		return peer.ReceiveBitvec2(peer.online, dR, eR)
	}
	if err := peer.ReceiveBitvec2(peer.online, dR, eR); err != nil {
		return err
	}
	return peer.SendBitvec2(peer.online, d, e)
}

// andLevelWords lists ceil(n_AND / 64) of every level that has ANDs, in level order (the pool fetches of
// andBatchFlush, network.go:673).
func (nw *Network) andLevelWords() []int {
	var info C.gc_gmw_info
	gates := nw.circ.Gates
	nwires := nw.circ.NumWires
	levels := int(nw.circ.Stats[circuit.NumLevels]) + 1
	perLevel := make([]C.uint32_t, levels)
	st := C.gc_gmw_plan_describe((*C.gc_gate)(unsafe.Pointer(&gates[0])), C.uint32_t(len(gates)), C.uint32_t(nwires),
		C.uint32_t(nw.circ.Inputs.Size()), C.uint32_t(nw.circ.Outputs.Size()), &info, nil, nil,
		(*C.uint32_t)(unsafe.Pointer(&perLevel[0])))
	if st != C.GC_OK {
		return nil
	}
	var out []int
	for _, w := range perLevel[:int(info.nlevels)] {
		if w != 0 {
			out = append(out, int(w))
		}
	}
	return out
}
