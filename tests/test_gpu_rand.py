"""The device random streams (gc_rand_*; mpc_amd/csrc/rand_kernels.hip, rand_ctr.h) byte for byte against the Python
restatement of the Go reader (tests/py_rand_reference.py: cipher.NewCTR over zeros), which the CPU tests hold against NIST SP
800-38A and OpenSSL.  Whole slots are compared: every device output is filled with a canary first and lies between two
sentinel words, so a byte written behind `nbytes`, before the array or past its end fails the case.

The sizes are the smallest at which the named thing can go wrong: one lane, a ragged block, several units per stream (a unit
is a wave's run of 64 blocks), more streams than a workgroup has waves, positions in mid-block (the bytewise stores), counter
carries into every higher word, more blocks and more streams than one sweep of the capped grid (sized from the constants the
binding exports)."""
import ctypes as C

import numpy as np
import pytest

import oracle
from mpc_amd import engine
from tests import py_rand_reference as rr
from tests.test_gpu_ot_sweeps import Guarded, SENTINEL

pytestmark = pytest.mark.gpu

GRID, THREADS, RUN = engine.rand_kernel_shape()
FF64 = (1 << 64) - 1

# NIST SP 800-38A F.5.1 / F.5.3 / F.5.5: keys; the initial counter block is shared
NIST_CTR = bytes.fromhex("f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff")
NIST_KEYS = [bytes.fromhex(k) for k in ("2b7e151628aed2a6abf7158809cf4f3c",
                                        "8e73b0f7da0e6452c810f32b809079e562f8ead2522c6b7b",
                                        "603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4")]
# the keystream of F.5.5 = its plaintext XOR its ciphertext, written out so that this case stands without the reference
F55_STREAM = bytes(a ^ b for a, b in zip(
    bytes.fromhex("6bc1bee22e409f96e93d7e117393172aae2d8a571e03ac9c9eb76fac45af8e51"
                  "30c81c46a35ce411e5fbc1191a0a52eff69f2445df4f9b17ad2b417be66c3710"),
    bytes.fromhex("601ec313775789a5b7a7f504bbf3d228f443e3ca4d62b59aca84e990cacaf5c5"
                  "2b0930daa23de94ce87017ba2d84988ddfc9c58db67aada613c2dd08457941a6")))


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


def seeded(tag, S, keylen=32, ivs=True):
    rng = np.random.default_rng([S, keylen] + list(tag.encode()))
    seeds = rng.integers(0, 256, (S, keylen), dtype=np.uint8)
    return seeds, (rng.integers(0, 256, (S, 16), dtype=np.uint8) if ivs else None)


def slot_stride(n):
    return (n + 15) // 16 * 16 + 32


def fill_dev(ctx, h, n, stride=None):
    """one gc_rand_fill_dev into canary-filled slots -> u8 [S, stride]"""
    stride = slot_stride(n) if stride is None else stride
    g = Guarded(ctx, h.S * stride)
    h.fill(n, g.ptr, stride)
    ctx.sync()
    return g.read().reshape(h.S, stride)


def check_slots(got, want, n):
    assert (got[:, :n] == want).all(), "session %d differs" % int(np.argmax((got[:, :n] != want).any(axis=1)))
    assert (got[:, n:] == SENTINEL).all(), "bytes behind nbytes were written"


# ---- 1. SP 800-38A on the device ------------------------------------------------------------------------------------------


def test_sp800_38a_f55_on_the_device(ctx):
    h = engine.RandStreams(ctx, [list(NIST_KEYS[2])], [list(NIST_CTR)])
    got = fill_dev(ctx, h, 64)
    assert got[0, :64].tobytes() == F55_STREAM == rr.keystream(NIST_KEYS[2], NIST_CTR, 0, 64)
    check_slots(got, rr.Streams([list(NIST_KEYS[2])], [list(NIST_CTR)]).read(64), 64)
    h.close()


def test_sp800_38a_every_key_length_three_sessions_each(ctx):
    for key in NIST_KEYS:  # F.5.1, F.5.3, F.5.5 in handles of their own, S = 3: the vector and two neighbours of its counter
        ivs = [list(NIST_CTR), list(rr.ctr_add(NIST_CTR, 1)), list(rr.ctr_add(NIST_CTR, 2))]
        h = engine.RandStreams(ctx, [list(key)] * 3, ivs)
        assert h.info() == (3, len(key), 0)
        got = fill_dev(ctx, h, 64)
        for s in range(3):
            assert got[s, :64].tobytes() == rr.keystream(key, NIST_CTR, 16 * s, 64), (len(key), s)
        h.close()


# ---- 2. sizes ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("S", [1, 3, 65])
def test_sizes(ctx, S):
    seeds, ivs = seeded("sizes", S)
    for n in (1, 15, 16, 17, 4112, 65541):
        h = engine.RandStreams(ctx, seeds, ivs)
        check_slots(fill_dev(ctx, h, n), rr.Streams(seeds, ivs).read(n), n)
        assert h.pos == n
        h.close()


def test_key_lengths_and_default_ivs(ctx):
    for keylen in (16, 24, 32):
        seeds, _ = seeded("keylen", 5, keylen, ivs=False)
        d_seeds = ctx.to_device(seeds)
        for h in (engine.RandStreams(ctx, seeds), engine.RandStreams(ctx, d_seeds, None, S=5, keylen=keylen)):
            check_slots(fill_dev(ctx, h, 1000), rr.Streams(seeds).read(1000), 1000)
            h.close()


# ---- 3. positions -----------------------------------------------------------------------------------------------------


def test_successive_fills_continue_the_streams(ctx):
    S = 3
    seeds, ivs = seeded("positions", S)
    h, ref = engine.RandStreams(ctx, seeds, ivs), rr.Streams(seeds, ivs)
    want = ref.at(0, 4176)
    parts, pos = [], 0
    for n in (8, 24, 1, 4112, 31):  # starts and ends in mid-block
        got = fill_dev(ctx, h, n)
        check_slots(got, want[:, pos:pos + n], n)
        parts.append(got[:, :n])
        pos += n
        assert h.info() == (S, 32, pos)
    assert pos == 4176 and (np.concatenate(parts, axis=1) == want).all()
    h.seek(5)
    assert h.pos == 5
    check_slots(fill_dev(ctx, h, 100), ref.at(5, 100), 100)
    assert h.pos == 105
    # a stride that is no multiple of 16: every block of the slots off a 16-byte boundary goes out bytewise
    g = Guarded(ctx, 3 * 48)
    h.seek(16)
    h.fill(37, g.ptr, 41)
    ctx.sync()
    raw = g.read()
    for s in range(S):
        assert (raw[41 * s: 41 * s + 37] == want[s, 16:53]).all() and (raw[41 * s + 37: 41 * s + 41] == SENTINEL).all()
    assert (raw[41 * S:] == SENTINEL).all()
    h.close()


# ---- 4. counter carries -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("iv", [(0x0123456789abcdef << 64) | (FF64 - 1),  # the carry enters the high half inside the fill
                                (0x1122334455667788 << 64) | (0x99aabbcc << 32) | 0xffffffff,  # low 32 bits all ones
                                (1 << 128) - 1],  # wraps to zero at block 1
                         ids=["into-high-half", "low-32-ones", "wrap"])
def test_counter_carries(ctx, iv):
    seeds, _ = seeded("carry", 3)
    ivs = [list(iv.to_bytes(16, "big"))] * 3
    h = engine.RandStreams(ctx, seeds, ivs)
    check_slots(fill_dev(ctx, h, 64), rr.Streams(seeds, ivs).read(64), 64)
    h.close()


def test_block_index_past_2_to_32(ctx):
    seeds, ivs = seeded("far", 3)
    pos = ((1 << 32) + 5) * 16 + 3
    h = engine.RandStreams(ctx, seeds, ivs)
    h.seek(pos)
    check_slots(fill_dev(ctx, h, 200), rr.Streams(seeds, ivs).at(pos, 200), 200)
    assert h.pos == pos + 200
    h.close()


# ---- 5. past one sweep of the grid --------------------------------------------------------------------------------------


def test_one_stream_longer_than_a_sweep(ctx):
    sweep = GRID * THREADS  # blocks one sweep of the capped grid covers
    n = (sweep + 2 * THREADS + RUN + 3) * 16 + 5
    seeds, ivs = seeded("sweep", 1)
    h = engine.RandStreams(ctx, seeds, ivs)
    check_slots(fill_dev(ctx, h, n), rr.Streams(seeds, ivs).read(n), n)
    h.close()


def test_more_streams_than_a_sweep_of_waves(ctx):
    S = 70000
    assert S > GRID * THREADS // 64
    seeds, ivs = seeded("many", S)
    h = engine.RandStreams(ctx, seeds, ivs)
    check_slots(fill_dev(ctx, h, 16, stride=16), rr.Streams(seeds, ivs).read(16), 16)
    h.close()


# ---- 6. GMW shares ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("S", [1, 3])
def test_gmw_shares(ctx, S):
    seeds, ivs = seeded("gmw", S)
    h, ref = engine.RandStreams(ctx, seeds, ivs), rr.Streams(seeds, ivs)
    for words in (1, 63, 1025):
        nb = (S * words * 8 + 15) // 16 * 16
        ga, gb = Guarded(ctx, nb), Guarded(ctx, nb)
        pos = h.pos
        h.gmw_shares(words, ga.ptr, gb.ptr)
        ctx.sync()
        assert h.pos == pos + 16 * words
        a, b = ga.read(), gb.read()
        assert (a[S * words * 8:] == SENTINEL).all() and (b[S * words * 8:] == SENTINEL).all()
        a, b = a[:S * words * 8].view(np.uint64).reshape(S, words), b[:S * words * 8].view(np.uint64).reshape(S, words)
        buf = ref.read(16 * words)
        for s in range(S):
            wa, wb = rr.gmw_shares(buf[s].tobytes())
            assert a[s].tolist() == wa and b[s].tolist() == wb, (words, s)
    # a position that is no multiple of 16 is refused and stays
    h.seek(8)
    d = ctx.zeros(64)
    with pytest.raises(engine.EngineError) as e:
        h.gmw_shares(1, d, d + 32)
    assert e.value.code == engine.GC_E_ARG and h.pos == 8
    h.close()


# ---- 7. through the garbler -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("batch", [3, 65])
def test_the_two_fills_feed_the_keyed_garbler(ctx, add64_circ, batch):
    """d_keys and d_rnd of gc_batch_garble_keyed written by the two draws of circuit.Garbler's order; instance i must be the
    oracle's garble under key = bytes [0, 32) and randomness = bytes [32, 32 + 16 (1 + n)) of stream i"""
    c = add64_circ
    seeds, ivs = seeded("garbler", batch)
    h = engine.RandStreams(ctx, seeds, ivs)
    dc = engine.DeviceCircuit(ctx, c)
    gb = engine.Batch(dc, batch)
    assert gb.keyed_supported()
    nrnd = 16 * (1 + c.num_inputs)
    d_keys, d_rnd = ctx.empty((batch, 32)), ctx.empty((batch, nrnd))
    h.draw_garbler(c.num_inputs, d_keys, d_rnd)
    assert h.pos == 32 + nrnd
    gb.garble_keyed(d_keys, 32, d_rnd)
    ctx.sync()
    R, slab = gb.read_r(), gb.read_slab()
    stream = rr.Streams(seeds, ivs).at(0, 32 + nrnd)
    for i in range(batch):
        key, rnd = rr.garbler_draw(stream[i].tobytes(), c.num_inputs)
        ref = oracle.garble(c.Gates, c.NumWires, c.num_inputs, key, rnd)
        assert R[i] == ref["R"], "R of instance %d" % i
        assert (slab[i] == ref["slab"]).all(), "tables of instance %d" % i
    gb.close()
    dc.close()
    h.close()


# ---- 8. host form and errors ------------------------------------------------------------------------------------------


def test_the_host_form_is_the_dev_form(ctx):
    S = 5
    seeds, ivs = seeded("host", S)
    h, ref = engine.RandStreams(ctx, seeds, ivs), rr.Streams(seeds, ivs)
    assert (h.fill_host(100) == ref.read(100)).all()          # packed
    out = np.full((S, 64), SENTINEL, np.uint8)
    h.fill_host(37, out, 64)                                   # rows with gaps, from a position in mid-block
    check_slots(out, ref.read(37), 37)
    assert h.pos == 137
    check_slots(fill_dev(ctx, h, 50), ref.read(50), 50)       # the two forms share the position
    h.close()


def test_error_contract(ctx):
    L = engine.lib()
    seeds, ivs = seeded("errors", 3)
    st = C.c_int(0)
    p_seeds = seeds.ctypes.data_as(C.c_void_p)
    assert not L.gc_rand_create(ctx.h, p_seeds, 20, None, 3, C.byref(st)) and st.value == engine.GC_E_KEYSIZE
    assert not L.gc_rand_create(ctx.h, p_seeds, 32, None, 0, C.byref(st)) and st.value == engine.GC_E_ARG
    assert not L.gc_rand_create(ctx.h, None, 32, None, 3, C.byref(st)) and st.value == engine.GC_E_ARG
    assert not L.gc_rand_create_dev(ctx.h, None, 32, None, 3, C.byref(st)) and st.value == engine.GC_E_ARG
    h = engine.RandStreams(ctx, seeds, ivs)
    d = ctx.zeros(3 * 64)
    host = np.zeros((3, 64), np.uint8)

    def refused(call, pos):
        with pytest.raises(engine.EngineError) as e:
            call()
        assert e.value.code == engine.GC_E_ARG and h.pos == pos

    h.seek(32)
    refused(lambda: h.fill(33, d, 32), 32)                      # stride < nbytes
    refused(lambda: h.fill_host(33, host, 32), 32)
    refused(lambda: h.fill(16, None, 64), 32)                   # a NULL array
    refused(lambda: h.gmw_shares(1, None, d), 32)
    refused(lambda: h.gmw_shares(1, d, None), 32)
    refused(lambda: h.fill(16, d, 1 << 63), 32)                 # the last slot would end past size_t
    refused(lambda: h.gmw_shares((1 << 60) + 1, d, d), 32)      # 16 * words does not fit
    assert L.gc_rand_fill(h.h, 16, None, 16) == engine.GC_E_ARG and h.pos == 32
    h.seek(FF64 - 7)
    refused(lambda: h.fill(16, d, 64), FF64 - 7)                # the position would pass 2^64 - 1
    refused(lambda: h.fill_host(16, host, 64), FF64 - 7)
    h.seek(FF64 - 15)
    refused(lambda: h.gmw_shares(2, d, d + 64), FF64 - 15)
    # nothing to do is no error, whatever the other arguments
    h.seek(7)
    h.fill(0, None, 0)
    h.fill_host(0, host, 0)
    h.gmw_shares(0, None, None)
    assert h.pos == 7
    # between capture_begin and _end every draw is refused (the position is a kernel argument), and create too; the capture
    # ends cleanly and the handle goes on where it was
    h.seek(16)
    for call in (lambda: h.fill(16, d, 64), lambda: h.fill_host(16, host, 64), lambda: h.gmw_shares(1, d, d + 64),
                 lambda: engine.RandStreams(ctx, seeds, ivs)):
        with pytest.raises(engine.EngineError) as e:
            ctx.capture(call)  # (ends the capture and drops the empty graph before the error travels on)
        assert e.value.code == engine.GC_E_ARG and h.pos == 16
    check_slots(fill_dev(ctx, h, 48), rr.Streams(seeds, ivs).at(16, 48), 48)
    h.close()
