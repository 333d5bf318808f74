//go:build gchip

// Package rand — the random streams of S sessions expanded on the device (gc_rand_*; DESIGN.md §22).
// SOURCE ONLY here (no Go toolchain in the build image); see INTEGRATION.md.
//
// Every consumer of randomness in the reference takes an io.Reader, and env.Config.Rand is where a host injects one.  A
// host that gives session s the reader cipher.StreamReader{S: cipher.NewCTR(aes.NewCipher(seed[s]), iv[s]), R: zeros}
// reads an AES-CTR keystream; DeviceRand writes that same keystream for all S sessions where the device consumes it, so
// the host draws one seed of real entropy per session (crypto/rand) and nothing else crosses the link.  Session s stays
// byte for byte what the unchanged Go code computes from HostReader(s).
package rand

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../mpc_amd/csrc -lgcengine -Wl,-rpath,${SRCDIR}/../../mpc_amd/csrc
#include "gcengine.h"
*/
import "C"

import (
	"crypto/aes"
	"crypto/cipher"
	"fmt"
	"io"
	"math/big"
	"unsafe"
)

// DeviceRand holds the expanded seeds of S sessions and the one byte position their streams share; the cursor calls
// (SetCursors, FillAt, Ints) keep one position per session in an array of the caller's instead.
type DeviceRand struct {
	h      *C.gc_rand
	seeds  [][]byte
	ivs    [][]byte
	keylen int
}

func randErr(st C.int) error {
	return fmt.Errorf("gcengine: %s", C.GoString(C.gc_strerror(st)))
}

// zeros is the source a cipher.StreamReader XORs the keystream into.
type zeros struct{}

func (zeros) Read(p []byte) (int, error) {
	for i := range p {
		p[i] = 0
	}
	return len(p), nil
}

// NewDeviceRand expands the seeds (16, 24 or 32 bytes each, all of one length) on the device.  ivs is nil for all-zero
// IVs, or one 16-byte IV per seed.  ctx is the gc_ctx of the batches the draws feed, as an unsafe.Pointer.
func NewDeviceRand(ctx unsafe.Pointer, seeds [][]byte, ivs [][]byte) (*DeviceRand, error) {
	if len(seeds) == 0 || (ivs != nil && len(ivs) != len(seeds)) {
		return nil, fmt.Errorf("invalid seed count: %v seeds, %v ivs", len(seeds), len(ivs))
	}
	keylen := len(seeds[0])
	flat := make([]byte, 0, len(seeds)*keylen)
	for _, s := range seeds {
		if len(s) != keylen {
			return nil, aes.KeySizeError(len(s))
		}
		flat = append(flat, s...)
	}
	if keylen != 16 && keylen != 24 && keylen != 32 {
		return nil, aes.KeySizeError(keylen)
	}
	var ivp *C.uint8_t
	if ivs != nil {
		flatIV := make([]byte, 0, 16*len(ivs))
		for _, v := range ivs {
			if len(v) != aes.BlockSize {
				return nil, fmt.Errorf("invalid IV length: %v", len(v))
			}
			flatIV = append(flatIV, v...)
		}
		ivp = (*C.uint8_t)(unsafe.Pointer(&flatIV[0]))
	}
	var st C.int
	h := C.gc_rand_create((*C.gc_ctx)(ctx), (*C.uint8_t)(unsafe.Pointer(&flat[0])), C.size_t(keylen), ivp,
		C.size_t(len(seeds)), &st)
	if h == nil {
		return nil, randErr(st)
	}
	return &DeviceRand{h: h, seeds: seeds, ivs: ivs, keylen: keylen}, nil
}

// Free waits for the ctx stream and releases the handle.
func (d *DeviceRand) Free() {
	C.gc_rand_free(d.h)
	d.h = nil
}

// Sessions is S.
func (d *DeviceRand) Sessions() int { return len(d.seeds) }

// Pos reports the bytes every stream has given out.
func (d *DeviceRand) Pos() (uint64, error) {
	var sessions, keylen C.size_t
	var pos C.uint64_t
	if st := C.gc_rand_info(d.h, &sessions, &keylen, &pos); st != C.GC_OK {
		return 0, randErr(st)
	}
	return uint64(pos), nil
}

// Seek sets the byte position of every stream.
func (d *DeviceRand) Seek(pos uint64) error {
	if st := C.gc_rand_seek(d.h, C.uint64_t(pos)); st != C.GC_OK {
		return randErr(st)
	}
	return nil
}

// Fill writes the next nbytes of stream s to dOut + s*stride (device memory), one launch on the ctx stream.
func (d *DeviceRand) Fill(nbytes int, dOut unsafe.Pointer, stride int) error {
	if st := C.gc_rand_fill_dev(d.h, C.size_t(nbytes), dOut, C.size_t(stride)); st != C.GC_OK {
		return randErr(st)
	}
	return nil
}

// FillHost is Fill into host memory: out holds S*stride bytes, of which the first nbytes of every row are written.
func (d *DeviceRand) FillHost(nbytes int, out []byte, stride int) error {
	if stride < nbytes || len(out) < len(d.seeds)*stride {
		return fmt.Errorf("invalid output size: %v for %v sessions of %v", len(out), len(d.seeds), stride)
	}
	if nbytes == 0 {
		return nil
	}
	if st := C.gc_rand_fill(d.h, C.size_t(nbytes), (*C.uint8_t)(unsafe.Pointer(&out[0])), C.size_t(stride)); st != C.GC_OK {
		return randErr(st)
	}
	return nil
}

// DrawGarbler is what circuit.Garbler reads from its session's reader (circuit/garbler.go:47-53, circuit/garble.go:253,
// 272): a 32-byte key into dKeys [S][32], then R and one label per input wire into dRnd [S][1+ninputs][16] — the d_keys
// and d_rnd of gc_batch_garble_keyed (circuit/batch_hip.go).
func (d *DeviceRand) DrawGarbler(ninputs int, dKeys, dRnd unsafe.Pointer) error {
	if err := d.Fill(32, dKeys, 32); err != nil {
		return err
	}
	return d.Fill(16*(1+ninputs), dRnd, 16*(1+ninputs))
}

// GMWShares is tripleBatch's draw loop (gmw/triples.go:301-310) for every session: words draws of 16 bytes,
// a = BigEndian.Uint64(buf[0:8]), b = BigEndian.Uint64(buf[8:16]), stored as native uint64 in dA, dB [S][words], where
// gc_gmw_triples_local_dev and gc_gmw_set_triples_dev read them (gmw/triples_hip.go).
func (d *DeviceRand) GMWShares(words int, dA, dB unsafe.Pointer) error {
	if st := C.gc_rand_gmw_shares_dev(d.h, C.size_t(words), dA, dB); st != C.GC_OK {
		return randErr(st)
	}
	return nil
}

// Per-session cursors: dCur is uint64 [S] in device memory (8-byte aligned), dCur[s] the byte position of stream s; dStatus
// is uint64 [2] = {bad sessions, lowest bad session}.  The calls below read the positions from dCur and advance it on the
// device, leave Pos alone and may be recorded between gc_ctx_capture_begin and _end: a replayed graph continues every
// stream where the array stands.  A bad session (its range would pass 2^64-1, or Ints would need more than 4*count+256
// candidates) keeps its outputs and its cursor untouched and is counted in dStatus.

// SetCursors sets dCur[s] = pos for every session.
func (d *DeviceRand) SetCursors(dCur unsafe.Pointer, pos uint64) error {
	if st := C.gc_rand_cur_set_dev(d.h, dCur, C.uint64_t(pos)); st != C.GC_OK {
		return randErr(st)
	}
	return nil
}

// FillAt writes bytes [cur[s], cur[s]+nbytes) of stream s to dOut + s*stride and advances cur[s] by nbytes.
func (d *DeviceRand) FillAt(dCur unsafe.Pointer, nbytes int, dOut unsafe.Pointer, stride int, dStatus unsafe.Pointer) error {
	if st := C.gc_rand_fill_cur_dev(d.h, dCur, C.size_t(nbytes), dOut, C.size_t(stride), dStatus); st != C.GC_OK {
		return randErr(st)
	}
	return nil
}

func maxBytes(max *big.Int) ([]byte, error) {
	if max.Sign() <= 0 || max.BitLen() > 256 {
		return nil, fmt.Errorf("invalid modulus: %v bits", max.BitLen())
	}
	return max.FillBytes(make([]byte, 32)), nil
}

// Ints is count successive crand.Int(reader_s, max) draws for every session, exactly as crypto/rand makes them on
// HostReader(s) positioned at cur[s]: dOut [S][count][32] big-endian, zero-padded on the left (the d_a of
// gc_co_multi_sender_setup_dev with count = 1, the d_scalars of gc_co_multi_receiver_choices_dev).  cur[s] advances by
// the bytes the draws consumed, rejected candidates included.  2 <= max < 2^256.
func (d *DeviceRand) Ints(dCur unsafe.Pointer, max *big.Int, count int, dOut, dStatus unsafe.Pointer) error {
	m, err := maxBytes(max)
	if err != nil {
		return err
	}
	if st := C.gc_rand_scalars_cur_dev(d.h, dCur, (*C.uint8_t)(unsafe.Pointer(&m[0])), C.size_t(count), dOut, dStatus); st != C.GC_OK {
		return randErr(st)
	}
	return nil
}

// FillAtHost is FillAt on host memory: cur [S] is read and written back, out holds S*stride bytes.  With a bad session it
// returns an error that names the lowest one; every good session is written and advanced all the same.
func (d *DeviceRand) FillAtHost(cur []uint64, nbytes int, out []byte, stride int) error {
	if len(cur) != len(d.seeds) || stride < nbytes || len(out) < len(d.seeds)*stride {
		return fmt.Errorf("invalid sizes: %v cursors, %v bytes for %v sessions of %v", len(cur), len(out), len(d.seeds), stride)
	}
	if nbytes == 0 {
		return nil
	}
	bad := ^C.size_t(0)
	st := C.gc_rand_fill_cur(d.h, (*C.uint64_t)(unsafe.Pointer(&cur[0])), C.size_t(nbytes), (*C.uint8_t)(unsafe.Pointer(&out[0])),
		C.size_t(stride), &bad)
	return cursorErr(st, bad)
}

// IntsHost is Ints on host memory: out holds S*count*32 bytes.
func (d *DeviceRand) IntsHost(cur []uint64, max *big.Int, count int, out []byte) error {
	m, err := maxBytes(max)
	if err != nil {
		return err
	}
	if len(cur) != len(d.seeds) || len(out) < len(d.seeds)*count*32 {
		return fmt.Errorf("invalid sizes: %v cursors, %v bytes for %v sessions of %v scalars", len(cur), len(out), len(d.seeds), count)
	}
	if count == 0 {
		return nil
	}
	bad := ^C.size_t(0)
	st := C.gc_rand_scalars_cur(d.h, (*C.uint64_t)(unsafe.Pointer(&cur[0])), (*C.uint8_t)(unsafe.Pointer(&m[0])), C.size_t(count),
		(*C.uint8_t)(unsafe.Pointer(&out[0])), &bad)
	return cursorErr(st, bad)
}

func cursorErr(st C.int, bad C.size_t) error {
	if st == C.GC_E_ARG && bad != ^C.size_t(0) {
		return fmt.Errorf("session %v: the stream ends before the draw does", uint64(bad))
	}
	if st != C.GC_OK {
		return randErr(st)
	}
	return nil
}

// HostReader builds the stream of session s from its start with crypto/cipher: what code that stays in Go sets as
// env.Config.Rand to read the bytes the device draws.
func (d *DeviceRand) HostReader(s int) (io.Reader, error) {
	block, err := aes.NewCipher(d.seeds[s])
	if err != nil {
		return nil, err
	}
	iv := make([]byte, aes.BlockSize)
	if d.ivs != nil {
		copy(iv, d.ivs[s])
	}
	return cipher.StreamReader{S: cipher.NewCTR(block, iv), R: zeros{}}, nil
}

// HostReaderAt is HostReader(s) with the first pos bytes read and dropped: the reader whose crand.Int draws Ints makes
// for a session whose cursor stands at pos, and whose Reads FillAt makes.
func (d *DeviceRand) HostReaderAt(s int, pos uint64) (io.Reader, error) {
	r, err := d.HostReader(s)
	if err != nil {
		return nil, err
	}
	if _, err := io.CopyN(io.Discard, r, int64(pos)); err != nil {
		return nil, err
	}
	return r, nil
}
