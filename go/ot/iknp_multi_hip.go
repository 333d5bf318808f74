//go:build gchip

// Package ot — S IKNP sessions of equal length per device call (gc_iknp_multi_*, gc_cot_multi_*): S instances of a
// two-party run whose 128 base OTs each came out of the gc_co_multi_* calls (co_multi_hip.go).
// SOURCE ONLY here (no Go toolchain in the build image); see INTEGRATION.md.
//
// Every session keeps its own ot.IO and is framed on it exactly as iknp.go:499 / :203 frame one session, so each of the S
// peers may be an unmodified Go party.  Arrays are session-major: OT j of session s is element s*per + j.
// ReceiveBits / SendBits are bit-COT (iknp.go:554-620, :259-310) for all S sessions in one device call each; a GMW party
// holds its P - 1 peer sessions in one handle per role (go/gmw/triples_hip.go).
// receiveMalicious / sendMalicious add the malicious branch of Receive / Send (iknp.go:373-465, :138-194) for all S
// sessions: a second extension at 256 and the KOS tags / check of every session in one device call (gc_kos_multi_*).
package ot

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../mpc_amd/csrc -lgcengine -Wl,-rpath,${SRCDIR}/../../mpc_amd/csrc
#include "gcengine.h"
*/
import "C"

import (
	"fmt"
	"io"
	"unsafe"
)

// hipIKNPMulti holds the base labels of S sessions and the one stream position they share.
type hipIKNPMulti struct {
	ctx *C.gc_ctx
	h   *C.gc_iknp_multi
	s   int
}

func multiErr(st C.int) error {
	return fmt.Errorf("gcengine: %s", C.GoString(C.gc_strerror(st)))
}

// after base.Send(wires[:]) of every session (iknp.go:337-356): wires holds S * K pairs
func newHipMultiReceiver(ctx *C.gc_ctx, wires []Wire) (*hipIKNPMulti, error) {
	if len(wires) == 0 || len(wires)%K != 0 {
		return nil, fmt.Errorf("invalid base wire count: %v", len(wires))
	}
	var st C.int
	h := C.gc_iknp_multi_receiver_create(ctx, (*C.gc_wire)(unsafe.Pointer(&wires[0])), C.size_t(len(wires)/K), &st)
	if h == nil {
		return nil, multiErr(st)
	}
	return &hipIKNPMulti{ctx: ctx, h: h, s: len(wires) / K}, nil
}

// after base.Receive(flags[:], k0[:]) of every session (iknp.go:112-122): one delta and K labels per session
func newHipMultiSender(ctx *C.gc_ctx, deltas []Label, k0 []Label) (*hipIKNPMulti, error) {
	if len(deltas) == 0 || len(k0) != len(deltas)*K {
		return nil, fmt.Errorf("invalid base label count: %v for %v sessions", len(k0), len(deltas))
	}
	var st C.int
	h := C.gc_iknp_multi_sender_create(ctx, (*C.gc_label)(unsafe.Pointer(&deltas[0])),
		(*C.gc_label)(unsafe.Pointer(&k0[0])), C.size_t(len(deltas)), &st)
	if h == nil {
		return nil, multiErr(st)
	}
	return &hipIKNPMulti{ctx: ctx, h: h, s: len(deltas)}, nil
}

// the base labels straight from device memory: dK0 is the d_labels_out of gc_co_multi_receiver_decrypt_dev /
// gc_co_multi_base_decrypt_dev at per = K (co_multi_hip.go), dDelta S labels; copied behind what the ctx stream holds
func newHipMultiSenderDev(ctx *C.gc_ctx, dDelta, dK0 unsafe.Pointer, sessions int) (*hipIKNPMulti, error) {
	var st C.int
	h := C.gc_iknp_multi_sender_create_dev(ctx, dDelta, dK0, C.size_t(sessions), &st)
	if h == nil {
		return nil, multiErr(st)
	}
	return &hipIKNPMulti{ctx: ctx, h: h, s: sessions}, nil
}

// dBase: the S * K gc_wire that gc_co_multi_sender_encrypt_dev read as d_wires
func newHipMultiReceiverDev(ctx *C.gc_ctx, dBase unsafe.Pointer, sessions int) (*hipIKNPMulti, error) {
	var st C.int
	h := C.gc_iknp_multi_receiver_create_dev(ctx, dBase, C.size_t(sessions), &st)
	if h == nil {
		return nil, multiErr(st)
	}
	return &hipIKNPMulti{ctx: ctx, h: h, s: sessions}, nil
}

func (m *hipIKNPMulti) free() {
	C.gc_iknp_multi_free(m.h)
	m.h = nil
}

// position reports the bytes every column stream of every session has given out
func (m *hipIKNPMulti) position() (uint64, error) {
	var sessions C.size_t
	var receiver C.int
	var pos C.uint64_t
	if st := C.gc_iknp_multi_info(m.h, &sessions, &receiver, &pos); st != C.GC_OK {
		return 0, multiErr(st)
	}
	return uint64(pos), nil
}

// receive runs (*IKNPReceiver).receive (iknp.go:468-511) for every session: b and result hold S * per elements, and
// session s sends its u-matrix on ios[s] in the messages of iknp.go:499
func (m *hipIKNPMulti) receive(ios []IO, b []bool, per int, result []Label) error {
	if len(ios) != m.s || len(b) != m.s*per || len(result) != len(b) {
		panic("len(b) != len(result)")
	}
	if per == 0 {
		for _, io := range ios {
			if err := io.Flush(); err != nil {
				return err
			}
		}
		return nil
	}
	ub := int(C.gc_iknp_u_bytes(C.size_t(per)))
	u := make([]byte, m.s*ub)
	// []bool is one byte per element (0/1): it crosses cgo as the choice array
	st := C.gc_iknp_multi_receive(m.h, (*C.uint8_t)(unsafe.Pointer(&b[0])), C.size_t(per),
		(*C.uint8_t)(unsafe.Pointer(&u[0])), (*C.gc_label)(unsafe.Pointer(&result[0])))
	if st != C.GC_OK {
		return multiErr(st)
	}
	for s, io := range ios {
		us := u[s*ub : (s+1)*ub]
		for ofs := 0; ofs < len(us); ofs += chunkSize { // same framing as iknp.go:499
			end := ofs + chunkSize
			if end > len(us) {
				end = len(us)
			}
			if err := io.SendData(us[ofs:end]); err != nil {
				return err
			}
		}
		if err := io.Flush(); err != nil {
			return err
		}
	}
	return nil
}

// send runs (*IKNPSender).send (iknp.go:197-226) for every session: session s reads its u-matrix from ios[s]
func (m *hipIKNPMulti) send(ios []IO, per int) ([]Label, error) {
	if len(ios) != m.s {
		panic("len(ios) != sessions")
	}
	result := make([]Label, m.s*per)
	ub := int(C.gc_iknp_u_bytes(C.size_t(per)))
	u := make([]byte, 0, m.s*ub)
	for s, io := range ios {
		for len(u) < (s+1)*ub {
			chunk, err := io.ReceiveData()
			if err != nil {
				return nil, err
			}
			if len(chunk)%K != 0 || len(u)+len(chunk) > (s+1)*ub {
				return nil, fmt.Errorf("invalid chunk size: %v", len(chunk))
			}
			u = append(u, chunk...)
		}
	}
	if per == 0 {
		return result, nil
	}
	st := C.gc_iknp_multi_send(m.h, (*C.uint8_t)(unsafe.Pointer(&u[0])), C.size_t(len(u)), C.size_t(per),
		(*C.gc_label)(unsafe.Pointer(&result[0])))
	if st != C.GC_OK {
		return nil, multiErr(st) // (the lengths were checked above: a wrong u_len cannot be the cause)
	}
	return result, nil
}

// device-resident forms: every array stays in HBM (d_* as in gcengine.h), asynchronous on the ctx stream
func (m *hipIKNPMulti) receiveDev(dChoicePacked unsafe.Pointer, per int, dU, dLabels unsafe.Pointer) error {
	if st := C.gc_iknp_multi_receive_dev(m.h, dChoicePacked, C.size_t(per), dU, dLabels); st != C.GC_OK {
		return multiErr(st)
	}
	return nil
}

func (m *hipIKNPMulti) sendDev(dU unsafe.Pointer, per int, dLabels unsafe.Pointer) error {
	if st := C.gc_iknp_multi_send_dev(m.h, dU, C.size_t(per), dLabels); st != C.GC_OK {
		return multiErr(st)
	}
	return nil
}

// IKNPMulti is the handle as other packages of the shim see it (go/gmw holds one per role over a party's peers).
type IKNPMulti = hipIKNPMulti

// Sessions reports S.
func (m *hipIKNPMulti) Sessions() int { return m.s }

// Handle is the gc_iknp_multi pointer for calls from another cgo package (C types are per package).
func (m *hipIKNPMulti) Handle() unsafe.Pointer { return unsafe.Pointer(m.h) }

// UBytes is the length of one session's u-matrix at per OTs.
func UBytes(per int) int { return int(C.gc_iknp_u_bytes(C.size_t(per))) }

// ReceiveBits runs (*IKNPReceiver).ReceiveBits (iknp.go:554-620) for every session in one device call.  choices holds the
// words of session s from word s*stride on; stride 0 is one vector of (per+63)/64 words for every session.  result holds
// S * ((per+63)/64) words.  The u-matrices come back session after session, UBytes(per) bytes each, for the caller to
// frame on each session's IO with SendU: the order of the messages on a connection is the caller's.
func (m *hipIKNPMulti) ReceiveBits(choices []uint64, stride, per int, result []uint64) ([]byte, error) {
	words := (per + 63) / 64
	if len(result) < m.s*words {
		return nil, fmt.Errorf("result buffer len=%v too short for n=%v", len(result), per)
	}
	need := words
	if stride != 0 {
		need = (m.s-1)*stride + words
	}
	if len(choices) < need {
		return nil, fmt.Errorf("choices buffer len=%v too short for n=%v", len(choices), per)
	}
	if per == 0 {
		return nil, nil
	}
	u := make([]byte, m.s*UBytes(per))
	st := C.gc_iknp_multi_receive_bits(m.h, (*C.uint64_t)(unsafe.Pointer(&choices[0])), C.size_t(stride), C.size_t(per),
		(*C.uint8_t)(unsafe.Pointer(&u[0])), (*C.uint64_t)(unsafe.Pointer(&result[0])))
	if st != C.GC_OK {
		return nil, multiErr(st)
	}
	return u, nil
}

// SendBits runs (*IKNPSender).SendBits (iknp.go:259-310) for every session in one device call: u holds the u-matrices the
// sessions' peers sent (ReceiveU), session after session.
func (m *hipIKNPMulti) SendBits(u []byte, per int, result []uint64) error {
	if len(result) < m.s*((per+63)/64) {
		return fmt.Errorf("result buffer len=%v too short for n=%v", len(result), per)
	}
	if per == 0 {
		return nil
	}
	st := C.gc_iknp_multi_send_bits(m.h, (*C.uint8_t)(unsafe.Pointer(&u[0])), C.size_t(len(u)), C.size_t(per),
		(*C.uint64_t)(unsafe.Pointer(&result[0])))
	if st != C.GC_OK {
		return multiErr(st)
	}
	return nil
}

// SendU frames one session's u-matrix as ReceiveBits does (iknp.go:597, :615): a message per chunk, then Flush.
func SendU(io IO, u []byte) error {
	for ofs := 0; ofs < len(u); ofs += chunkSize {
		end := ofs + chunkSize
		if end > len(u) {
			end = len(u)
		}
		if err := io.SendData(u[ofs:end]); err != nil {
			return err
		}
	}
	return io.Flush()
}

// ReceiveU reads the chunk messages of one session's u-matrix at per OTs into dst (UBytes(per) bytes) as SendBits reads
// them (iknp.go:266-272).
func ReceiveU(io IO, dst []byte) error {
	for at := 0; at < len(dst); {
		chunk, err := io.ReceiveData()
		if err != nil {
			return err
		}
		if len(chunk)%K != 0 || at+len(chunk) > len(dst) {
			return fmt.Errorf("invalid chunk size: %v", len(chunk))
		}
		at += copy(dst[at:], chunk)
	}
	return nil
}

// device-resident forms of bit-COT: one kernel each, nothing allocated, asynchronous on the ctx stream
func (m *hipIKNPMulti) ReceiveBitsDev(dChoices unsafe.Pointer, stride, per int, dU, dResult unsafe.Pointer) error {
	if st := C.gc_iknp_multi_receive_bits_dev(m.h, dChoices, C.size_t(stride), C.size_t(per), dU, dResult); st != C.GC_OK {
		return multiErr(st)
	}
	return nil
}

func (m *hipIKNPMulti) SendBitsDev(dU unsafe.Pointer, per int, dResult unsafe.Pointer) error {
	if st := C.gc_iknp_multi_send_bits_dev(m.h, dU, C.size_t(per), dResult); st != C.GC_OK {
		return multiErr(st)
	}
	return nil
}

// pad loop of COT.Send (cot.go:155-182) for S sessions: seeds and deltas hold one label per session, data and wires
// S * per elements; out = the 2 * per labels every session puts on its wire, session after session
func cotMultiSendPads(ctx *C.gc_ctx, seeds, deltas []Label, data []Label, wires []Wire, per int) ([]Label, error) {
	out := make([]Label, 2*len(wires))
	if len(wires) == 0 {
		return out, nil
	}
	st := C.gc_cot_multi_send_pads(ctx, (*C.gc_label)(unsafe.Pointer(&seeds[0])), (*C.gc_label)(unsafe.Pointer(&deltas[0])),
		(*C.gc_label)(unsafe.Pointer(&data[0])), (*C.gc_wire)(unsafe.Pointer(&wires[0])), C.size_t(len(seeds)),
		C.size_t(per), (*C.gc_label)(unsafe.Pointer(&out[0])))
	if st != C.GC_OK {
		return nil, multiErr(st)
	}
	return out, nil
}

// unpad loop of COT.Receive (cot.go:200-232) for S sessions: result holds the receivers' IKNP labels in, the chosen wire
// labels out
func cotMultiReceiveUnpad(ctx *C.gc_ctx, seeds []Label, flags []bool, sent []Label, result []Label, per int) error {
	if len(flags) == 0 {
		return nil
	}
	st := C.gc_cot_multi_receive_unpad(ctx, (*C.gc_label)(unsafe.Pointer(&seeds[0])),
		(*C.uint8_t)(unsafe.Pointer(&flags[0])), (*C.gc_label)(unsafe.Pointer(&sent[0])),
		(*C.gc_label)(unsafe.Pointer(&result[0])), C.size_t(len(seeds)), C.size_t(per))
	if st != C.GC_OK {
		return multiErr(st)
	}
	return nil
}

func cotMultiSendPadsDev(ctx *C.gc_ctx, dSeeds, dDeltas, dData, dWires unsafe.Pointer, sessions, per int, dOut unsafe.Pointer) error {
	if st := C.gc_cot_multi_send_pads_dev(ctx, dSeeds, dDeltas, dData, dWires, C.size_t(sessions), C.size_t(per), dOut); st != C.GC_OK {
		return multiErr(st)
	}
	return nil
}

func cotMultiReceiveUnpadDev(ctx *C.gc_ctx, dSeeds, dFlags, dSent, dResult unsafe.Pointer, sessions, per int) error {
	if st := C.gc_cot_multi_receive_unpad_dev(ctx, dSeeds, dFlags, dSent, dResult, C.size_t(sessions), C.size_t(per)); st != C.GC_OK {
		return multiErr(st)
	}
	return nil
}

// receiveMalicious runs (*IKNPReceiver).Receive(b, result, true) (iknp.go:364-465) for every session.  Session s draws
// b0, b1 and seed2 from rands[s] in the reference's order (:374-381, :403), the 256 random choices of all sessions are
// extended in one call, seed2 goes out on ios[s], and x, t0, t1 of all sessions come from one device call.
func (m *hipIKNPMulti) receiveMalicious(ios []IO, rands []io.Reader, b []bool, per int, result []Label) error {
	if len(rands) != m.s {
		panic("len(rands) != sessions")
	}
	if err := m.receive(ios, b, per, result); err != nil {
		return err
	}
	bcv := make([]bool, m.s*256)
	for s := 0; s < m.s; s++ {
		b0, err := NewLabel(rands[s])
		if err != nil {
			return err
		}
		b1, err := NewLabel(rands[s])
		if err != nil {
			return err
		}
		for i := 0; i < 256; i++ { // iknp.go:382-389
			if i < 128 {
				bcv[s*256+i] = b0.Bit(i) == 1
			} else {
				bcv[s*256+i] = b1.Bit(i-128) == 1
			}
		}
	}
	choiceVector := make([]Label, m.s*256)
	if err := m.receive(ios, bcv, 256, choiceVector); err != nil {
		return err
	}
	seed2 := make([]Label, m.s)
	var ld LabelData
	for s, io := range ios {
		var err error
		if seed2[s], err = NewLabel(rands[s]); err != nil {
			return err
		}
		if err := io.SendLabel(seed2[s], &ld); err != nil {
			return err
		}
		if err := io.Flush(); err != nil {
			return err
		}
	}
	tags := make([]Label, 3*m.s) // x, t0, t1 of every session
	var resPtr *C.gc_label
	var bPtr *C.uint8_t
	if per > 0 {
		resPtr = (*C.gc_label)(unsafe.Pointer(&result[0]))
		bPtr = (*C.uint8_t)(unsafe.Pointer(&b[0]))
	}
	st := C.gc_kos_multi_receiver_tags(m.ctx, (*C.gc_label)(unsafe.Pointer(&seed2[0])), resPtr, bPtr,
		(*C.gc_label)(unsafe.Pointer(&choiceVector[0])), (*C.uint8_t)(unsafe.Pointer(&bcv[0])), C.size_t(m.s),
		C.size_t(per), (*C.gc_label)(unsafe.Pointer(&tags[0])))
	if st != C.GC_OK {
		return multiErr(st)
	}
	for s, io := range ios {
		for k := 0; k < 3; k++ { // iknp.go:456-464
			if err := io.SendLabel(tags[3*s+k], &ld); err != nil {
				return err
			}
		}
		if err := io.Flush(); err != nil {
			return err
		}
	}
	return nil
}

// sendMalicious runs (*IKNPSender).Send(per, true) (iknp.go:129-194) for every session: deltas are the S deltas the
// handle was created with.  A failing check is the reference's error, naming the lowest failing session.
func (m *hipIKNPMulti) sendMalicious(ios []IO, deltas []Label, per int) ([]Label, error) {
	if len(deltas) != m.s {
		panic("len(deltas) != sessions")
	}
	result, err := m.send(ios, per)
	if err != nil {
		return nil, err
	}
	choiceVector, err := m.send(ios, 256)
	if err != nil {
		return nil, err
	}
	seed2 := make([]Label, m.s)
	tags := make([]Label, 3*m.s)
	var ld LabelData
	for s, io := range ios { // a session's peer sends seed2 before it computes, and the tags behind (iknp.go:408, 456-464)
		if err := io.ReceiveLabel(&seed2[s], &ld); err != nil {
			return nil, err
		}
	}
	for s, io := range ios {
		for k := 0; k < 3; k++ {
			if err := io.ReceiveLabel(&tags[3*s+k], &ld); err != nil {
				return nil, err
			}
		}
	}
	var resPtr *C.gc_label
	if per > 0 {
		resPtr = (*C.gc_label)(unsafe.Pointer(&result[0]))
	}
	var bad C.size_t
	st := C.gc_kos_multi_sender_check(m.ctx, (*C.gc_label)(unsafe.Pointer(&seed2[0])), resPtr,
		(*C.gc_label)(unsafe.Pointer(&choiceVector[0])), (*C.gc_label)(unsafe.Pointer(&deltas[0])),
		(*C.gc_label)(unsafe.Pointer(&tags[0])), C.size_t(m.s), C.size_t(per), nil, &bad)
	if st != C.GC_OK {
		return nil, multiErr(st)
	}
	if bad != ^C.size_t(0) {
		return nil, fmt.Errorf("OT extension check failed (session %d)", uint64(bad))
	}
	return result, nil
}

// device-resident forms of the two KOS calls: every array in HBM, asynchronous on the ctx stream, no stream position (they
// may be captured).  dChoicePacked / dBcvPacked are the buffers receiveDev consumed at per and at 256, dResult /
// dChoiceVec the labels it (or sendDev) left; dTags holds x, t0, t1 of every session.
func kosMultiReceiverTagsDev(ctx *C.gc_ctx, dSeed2, dResult, dChoicePacked, dChoiceVec, dBcvPacked unsafe.Pointer, sessions, per int, dTags unsafe.Pointer) error {
	if st := C.gc_kos_multi_receiver_tags_dev(ctx, dSeed2, dResult, dChoicePacked, dChoiceVec, dBcvPacked, C.size_t(sessions), C.size_t(per), dTags); st != C.GC_OK {
		return multiErr(st)
	}
	return nil
}

func kosMultiSenderCheckDev(ctx *C.gc_ctx, dSeed2, dResult, dChoiceVec, dDelta, dTags unsafe.Pointer, sessions, per int, dOk, dStatus unsafe.Pointer) error {
	if st := C.gc_kos_multi_sender_check_dev(ctx, dSeed2, dResult, dChoiceVec, dDelta, dTags, C.size_t(sessions), C.size_t(per), dOk, dStatus); st != C.GC_OK {
		return multiErr(st)
	}
	return nil
}
