"""The IKNP extension and the COT pad loops for S sessions per call (gc_iknp_multi_*, gc_cot_multi_*;
mpc_amd/csrc/iknp_multi_kernels.hip, iknp_multi.h) byte for byte against the C oracle run on every session ALONE:
oracle.IKNPReceiver / IKNPSender, oracle.cot_send_pads / cot_receive_unpad.  Sessions have different seeded base labels,
deltas and seeds.  Whole buffers are compared, and every device output lies between two sentinel words.

The sizes are the smallest at which the named thing can go wrong: sessions shorter than a chunk, a block, a byte; a session
of several chunks with a ragged last one; a stream position off a block boundary; a second, ragged step of workgroup 0 of
the capped grid (derived from kernels.h); COT sessions across waves, workgroups and trips."""
import ctypes as C

import numpy as np
import pytest

import oracle
from mpc_amd import engine
from mpc_amd.circuit import LABEL, WIRE
from tests.test_gpu_ot_sweeps import Guarded, SENTINEL, chosen, label_u8, rand_labels, xor_where
from tests.util import kernel_constants

pytestmark = pytest.mark.gpu

MULTI_GRID, SEND_ITEMS, RECV_ITEMS = kernel_constants("kIknpMultiGrid", "kIknpSendChunks", "kIknpRecvChunks")
COT_THREADS, COT_GRID = kernel_constants("kCotThreads", "kCotGrid")
CHUNK = 512


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


def u_bytes(per):
    return (per // CHUNK) * 8192 + ((per % CHUNK + 7) // 8) * 128


def chunks(per):
    return -(-per // CHUNK)


def delta_bits(deltas):
    """[S, 128] bools: Delta.Bit(i) is bit i of D0 for i < 64, of D1 above (label.go:129-141)"""
    sh = np.arange(64, dtype=np.uint64)
    return np.concatenate([(deltas["d0"][:, None] >> sh) & np.uint64(1), (deltas["d1"][:, None] >> sh) & np.uint64(1)], axis=1).astype(bool)


def make_sessions(seed, S):
    """what S base-OT sessions leave: the receiver's label pairs [S, 128], the sender's deltas [S] and its labels [S, 128]"""
    rng = np.random.default_rng(seed)
    base = np.zeros((S, 128), WIRE)
    base["l0"], base["l1"] = rand_labels(rng, S * 128).reshape(S, 128), rand_labels(rng, S * 128).reshape(S, 128)
    deltas = rand_labels(rng, S)
    k0 = np.where(delta_bits(deltas), base["l1"], base["l0"])
    return rng, base, deltas, k0


def tup(l):
    return int(l["d0"]), int(l["d1"])


class OracleSessions:
    """one oracle receiver and one oracle sender per session, each run alone"""

    def __init__(self, base, deltas, k0):
        self.S = len(base)
        self.deltas = deltas
        self.rcv = [oracle.IKNPReceiver(base[s]) for s in range(self.S)]
        self.snd = [oracle.IKNPSender(tup(deltas[s]), k0[s]) for s in range(self.S)]

    def call(self, b, per):
        """b [S, per] -> u of all sessions (bytes), the receivers' labels, the senders' labels fed with that u"""
        us, got, sent = [], [], []
        for s in range(self.S):
            u, g = self.rcv[s].receive(b[s])
            assert len(u) == u_bytes(per)
            us.append(u)
            got.append(g.copy())
            sent.append(self.snd[s].send(u, per).copy())
        got, sent = np.concatenate(got), np.concatenate(sent)
        for s in range(self.S):  # rcvd = sent ^ b * delta_s (iknp_test.go:98-113), per session
            lo, hi = s * per, (s + 1) * per
            assert (got[lo:hi] == xor_where(sent[lo:hi], b[s], tup(self.deltas[s]))).all()
        return b"".join(us), got, sent

    def pos(self):
        """bytes every column stream has given out: blocks drawn * 16 less what is left of the last one (ot_oracle.c: prg)"""
        out = set()
        for p in (self.rcv[0].s.g0[0], self.rcv[0].s.g1[127], self.snd[-1].s.g0[64]):
            out.add(int.from_bytes(bytes(p.ctr), "big") * 16 - (16 - p.used))
        assert len(out) == 1
        return out.pop()


def oracle_once(base, deltas, k0, b, per):
    """one call from position 0, the oracle pair of a session dropped as soon as it has run (sizes past one trip)"""
    us, got, sent = [], [], []
    for s in range(len(base)):
        one = OracleSessions(base[s:s + 1], deltas[s:s + 1], k0[s:s + 1])
        u, g, t = one.call(b[s:s + 1], per)
        us.append(u), got.append(g), sent.append(t)
    return b"".join(us), np.concatenate(got), np.concatenate(sent)


def pack_choice(b, S, per):
    """the _dev form's choice bits: LSB first, every session zero-padded to whole chunks of 64 bytes"""
    bits = np.packbits(np.asarray(b, np.uint8).reshape(S, per), axis=1, bitorder="little")
    out = np.zeros((S, chunks(per) * 64), np.uint8)
    out[:, :bits.shape[1]] = bits
    return out


def receive_dev(ctx, rcv, b, S, per):
    d_choice = ctx.to_device(pack_choice(b, S, per))
    g_u, g_lab = Guarded(ctx, S * u_bytes(per)), Guarded(ctx, 16 * S * per)
    rcv.receive_dev(d_choice, per, g_u.ptr, g_lab.ptr)
    ctx.sync()
    return g_u.read().tobytes(), g_lab.read().tobytes()


def send_dev(ctx, snd, u, S, per):
    d_u = ctx.to_device(np.frombuffer(u, np.uint8))
    g_lab = Guarded(ctx, 16 * S * per)
    snd.send_dev(d_u, per, g_lab.ptr)
    ctx.sync()
    return g_lab.read().tobytes()


def check_calls(ctx, seed, S, pers, forms=("host", "dev")):
    """one pair of handles per form, the calls of `pers` one after the other, against one oracle pair per session"""
    rng, base, deltas, k0 = make_sessions(seed, S)
    want = []
    orc = OracleSessions(base, deltas, k0)
    for per in pers:
        b = rng.integers(0, 2, (S, per)).astype(np.uint8)
        want.append((per, b) + orc.call(b, per) + (orc.pos(),))
    for form in forms:
        rcv, snd = engine.IKNPMultiReceiver(ctx, base), engine.IKNPMultiSender(ctx, deltas, k0)
        assert rcv.info() == (S, True, 0) and snd.info() == (S, False, 0)
        for per, b, u, got, sent, pos in want:
            what = "%s form, S = %d, per = %d" % (form, S, per)
            if form == "host":
                have_u, have_got = rcv.receive(b.reshape(-1), per)
                have_got, have_sent = have_got.tobytes(), snd.send(u, per).tobytes()  # the sender is fed the ORACLE's u
            else:
                have_u, have_got = receive_dev(ctx, rcv, b, S, per)
                have_sent = send_dev(ctx, snd, u, S, per)
            assert have_u == u, "u differs from the oracle's (%s)" % what
            assert have_got == got.tobytes(), "the receiver's labels differ from the oracle's (%s)" % what
            assert have_sent == sent.tobytes(), "the sender's labels differ from the oracle's (%s)" % what
            assert rcv.pos == pos and snd.pos == pos, what
        rcv.close()
        snd.close()


# ---- 1, 2: short sessions, several chunks ------------------------------------------------------------------------------


@pytest.mark.parametrize("per", [128, 127, 37, 1])
def test_short_sessions(ctx, per):
    """a session of a whole block per column, of 16 bytes with 7 bits to spare, of 5 bytes (byte by byte), of one OT"""
    check_calls(ctx, 20241001 + per, 3, [per])


@pytest.mark.parametrize("per", [549, 1024])
def test_several_chunks(ctx, per):
    """a full chunk plus 37 rows: items of four blocks and of one in one step; two full chunks"""
    check_calls(ctx, 20241002 + per, 3, [per])


# ---- 3: the stream position ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("variant", ["default", "generic"])
def test_stream_position_across_calls(ctx, monkeypatch, variant):
    """40 OTs leave every column 5 bytes into a block: the 16-byte columns of the next call take two blocks, the full chunk
    of the third five.  generic: the general counter form (GC_IKNP_GENERIC=1)"""
    if variant == "generic":
        monkeypatch.setenv("GC_IKNP_GENERIC", "1")
    check_calls(ctx, 20241003, 3, [40, 128, 549])


def test_every_arm_of_the_misaligned_shift(ctx):
    """the calls start at byte 0, 12, 19, 24 and 93 of every column stream: off a block boundary by 12 (three dwords, no
    bytes), 3 (no dwords, three bytes), 8 (two dwords; a full chunk, five blocks) and 13 (three dwords and a byte) —
    with the 5 of the test above every dword selection of column_stream's shift, with and without a byte part"""
    pers = [96, 56, 40, 549, 128]
    starts = [0]
    for per in pers:
        starts.append(starts[-1] + (per // CHUNK) * 64 + (per % CHUNK + 7) // 8)
    assert [p % 16 for p in starts[:5]] == [0, 12, 3, 8, 13]
    check_calls(ctx, 20241010, 3, pers)


# ---- 4: past one trip of the capped grid ---------------------------------------------------------------------------------


def test_sender_past_one_trip(ctx):
    """per = 37 is one item per session and a sender step takes SEND_ITEMS: the smallest S at which workgroup 0 has a second
    step, and that step is ragged (one item, seven slices idle)"""
    per, S = 37, MULTI_GRID * SEND_ITEMS + 1
    items = S * chunks(per)
    steps = -(-items // SEND_ITEMS)
    assert steps == MULTI_GRID + 1 and items % SEND_ITEMS == 1 and (S - 1) * chunks(per) <= MULTI_GRID * SEND_ITEMS
    rng, base, deltas, k0 = make_sessions(20241004, S)
    b = rng.integers(0, 2, (S, per)).astype(np.uint8)
    u, _, sent = oracle_once(base, deltas, k0, b, per)
    snd = engine.IKNPMultiSender(ctx, deltas, k0)
    assert send_dev(ctx, snd, u, S, per) == sent.tobytes(), "the sender's labels differ from the oracle's"
    snd.close()


def test_receiver_past_one_trip(ctx):
    """per = 549 is a full chunk and one of 37 rows per session and a receiver step takes RECV_ITEMS: the smallest S at which
    workgroup 0 has a second step, and that step is ragged (the two items of the last session, two slices of each stream idle)"""
    per, S = 549, MULTI_GRID * RECV_ITEMS // 2 + 1
    items = S * chunks(per)
    steps = -(-items // RECV_ITEMS)
    assert chunks(per) == 2 and steps == MULTI_GRID + 1 and items % RECV_ITEMS == 2
    assert (S - 1) * chunks(per) <= MULTI_GRID * RECV_ITEMS
    rng, base, deltas, k0 = make_sessions(20241005, S)
    b = rng.integers(0, 2, (S, per)).astype(np.uint8)
    u, got, _ = oracle_once(base, deltas, k0, b, per)
    rcv = engine.IKNPMultiReceiver(ctx, base)
    have_u, have_got = receive_dev(ctx, rcv, b, S, per)
    assert have_u == u, "u differs from the oracle's"
    assert have_got == got.tobytes(), "the receiver's labels differ from the oracle's"
    rcv.close()


# ---- 5: COT multi ------------------------------------------------------------------------------------------------------


def cot_case(seed, S, per):
    """the labels IKNP would hand over are made in numpy with the IKNP correlation, per session; the oracle's bytes per
    session alone"""
    rng = np.random.default_rng(seed)
    seeds, deltas = rand_labels(rng, S), rand_labels(rng, S)
    n = S * per
    data = rand_labels(rng, n)
    flags = rng.integers(0, 2, n).astype(np.uint8)
    recv = data.copy()
    wires = np.zeros(n, WIRE)
    wires["l0"], wires["l1"] = rand_labels(rng, n), rand_labels(rng, n)
    sent, res = [], []
    for s in range(S):
        lo, hi = s * per, (s + 1) * per
        recv[lo:hi] = xor_where(data[lo:hi], flags[lo:hi], tup(deltas[s]))
        sent.append(oracle.cot_send_pads(tup(seeds[s]), tup(deltas[s]), data[lo:hi], wires[lo:hi]).copy())
        res.append(oracle.cot_receive_unpad(tup(seeds[s]), flags[lo:hi], sent[-1], recv[lo:hi]).copy())
    res = np.concatenate(res)
    assert (res == chosen(wires, flags)).all()
    return dict(S=S, per=per, n=n, seeds=seeds, deltas=deltas, data=data, flags=flags, recv=recv, wires=wires,
                sent=np.concatenate(sent), res=res)


def check_cot(ctx, c, host):
    S, per, n = c["S"], c["per"], c["n"]
    if host:
        sent = engine.cot_multi_send_pads(ctx, c["seeds"], c["deltas"], c["data"], c["wires"], S, per)
        assert sent.tobytes() == c["sent"].tobytes(), "COT.Send pads differ from the oracle's (host form)"
        res = engine.cot_multi_receive_unpad(ctx, c["seeds"], c["flags"], sent, c["recv"], S, per)
        assert res.tobytes() == c["res"].tobytes(), "COT.Receive labels differ from the oracle's (host form)"
        assert (res == chosen(c["wires"], c["flags"])).all(), "result[j] == wires[j].L{flag_j}"
    d_seeds, d_deltas = ctx.to_device(label_u8(c["seeds"])), ctx.to_device(label_u8(c["deltas"]))
    d_data, d_wires, d_flags = ctx.to_device(label_u8(c["data"])), ctx.to_device(label_u8(c["wires"])), ctx.to_device(c["flags"])
    g_sent, g_res = Guarded(ctx, 32 * n), Guarded(ctx, 16 * n, c["recv"])
    engine.cot_multi_send_pads_dev(ctx, d_seeds, d_deltas, d_data, d_wires, S, per, g_sent.ptr)
    engine.cot_multi_receive_unpad_dev(ctx, d_seeds, d_flags, g_sent.ptr, g_res.ptr, S, per)
    ctx.sync()
    assert g_sent.read().tobytes() == c["sent"].tobytes(), "COT.Send pads differ from the oracle's (device form)"
    res = g_res.read().tobytes()
    assert res == c["res"].tobytes(), "COT.Receive labels differ from the oracle's (device form)"
    assert res == chosen(c["wires"], c["flags"]).tobytes(), "result[j] == wires[j].L{flag_j}"


@pytest.mark.parametrize("per", [128, 37])
def test_cot_multi_short(ctx, per):
    check_cot(ctx, cot_case(20241006 + per, 3, per), host=True)


def test_cot_multi_past_one_sweep(ctx):
    """per = 127 puts session edges everywhere inside waves and workgroups; the smallest S past one trip of the capped grid
    plus a full workgroup, with a ragged last workgroup"""
    per = 127
    sweep = COT_GRID * COT_THREADS
    S = (sweep + COT_THREADS) // per + 1
    while (S * per) % COT_THREADS == 0:
        S += 1
    assert S * per > sweep + COT_THREADS and (S * per) % COT_THREADS != 0 and (S - 1) * per <= sweep + COT_THREADS
    check_cot(ctx, cot_case(20241007, S, per), host=False)


# ---- 6: the chain on the device ----------------------------------------------------------------------------------------


def test_base_ot_to_cot_on_the_device(ctx):
    """Chou-Orlandi for S sessions of 128 base OTs -> the multi handles created from the device arrays -> 128 OTs per
    session -> the COT pads, with nothing staged through the host in between.  The IKNP receiver is the base-OT sender (it
    holds the label pairs), the IKNP sender the base-OT receiver with the bits of delta_s as its choices."""
    from tests.test_gpu_co import scalars_array
    from tests.util import drbg
    S, per = 5, 128
    rng, base, deltas, k0 = make_sessions(20241008, S)
    a = scalars_array([int.from_bytes(drbg("iknp_multi/chain/a%d" % s, 32), "big") for s in range(S)])
    sc = scalars_array([int.from_bytes(drbg("iknp_multi/chain/b%d" % i, 32), "big") for i in range(S * 128)]).reshape(-1, 32)
    choice = delta_bits(deltas).astype(np.uint8).reshape(-1)
    d_a, d_sc, d_ch, d_base = ctx.to_device(a), ctx.to_device(sc), ctx.to_device(choice), ctx.to_device(label_u8(base))
    d_A, d_ainv, d_pts, d_ct = ctx.zeros((S, 64)), ctx.zeros((S, 64)), ctx.zeros((S * 128, 64)), ctx.zeros((S * 128, 32))
    g_k0 = Guarded(ctx, 16 * S * 128)
    d_st = [ctx.zeros(4, np.uint64) for _ in range(4)]
    engine.co_multi_sender_setup_dev(ctx, d_a, S, d_A, d_ainv, d_st[0])
    engine.co_multi_receiver_choices_dev(ctx, d_A, d_sc, d_ch, S, 128, d_pts, d_st[1])
    engine.co_multi_sender_encrypt_dev(ctx, d_a, d_ainv, d_pts, d_base, S, 128, 0, d_ct, d_st[2])
    engine.co_multi_receiver_decrypt_dev(ctx, d_A, d_sc, d_ch, d_ct, S, 128, 0, g_k0.ptr, d_st[3])
    # the handles copy behind the decrypt that is still queued
    d_deltas = ctx.to_device(label_u8(deltas))
    snd = engine.IKNPMultiSender(ctx, d_deltas, g_k0.ptr, S=S)
    rcv = engine.IKNPMultiReceiver(ctx, d_base, S=S)
    b = rng.integers(0, 2, (S, per)).astype(np.uint8)
    d_choice = ctx.to_device(pack_choice(b, S, per))
    g_u, g_got, g_sent = Guarded(ctx, S * u_bytes(per)), Guarded(ctx, 16 * S * per), Guarded(ctx, 16 * S * per)
    rcv.receive_dev(d_choice, per, g_u.ptr, g_got.ptr)
    snd.send_dev(g_u.ptr, per, g_sent.ptr)
    # COT over seeded wires: the IKNP sender pads with its labels, the IKNP receiver unpads its own in place
    seeds = rand_labels(rng, S)
    wires = np.zeros(S * per, WIRE)
    wires["l0"], wires["l1"] = rand_labels(rng, S * per), rand_labels(rng, S * per)
    d_seeds, d_wires, d_flags = ctx.to_device(label_u8(seeds)), ctx.to_device(label_u8(wires)), ctx.to_device(b.reshape(-1))
    g_pads = Guarded(ctx, 32 * S * per)
    engine.cot_multi_send_pads_dev(ctx, d_seeds, d_deltas, g_sent.ptr, d_wires, S, per, g_pads.ptr)
    ctx.sync()
    got_before = g_got.read().tobytes()
    engine.cot_multi_receive_unpad_dev(ctx, d_seeds, d_flags, g_pads.ptr, g_got.ptr, S, per)
    ctx.sync()
    assert all(int(v) == w for d in d_st for v, w in zip(d.numpy(), [0, (1 << 64) - 1, 0, (1 << 64) - 1])), "a bad base OT"
    assert g_k0.read().tobytes() == k0.tobytes(), "the base OTs did not select the oracle's labels"
    u, got, sent = OracleSessions(base, deltas, k0).call(b, per)
    assert g_u.read().tobytes() == u and got_before == got.tobytes() and g_sent.read().tobytes() == sent.tobytes()
    assert g_got.read().tobytes() == chosen(wires, b.reshape(-1)).tobytes(), "the receiver ends with wires[s][j].L{flag}"
    rcv.close()
    snd.close()


# ---- 7: argument errors --------------------------------------------------------------------------------------------------


def test_argument_errors(ctx):
    L, E_ARG, OK = engine.lib(), engine.GC_E_ARG, engine.GC_OK
    S, per = 3, 128
    rng, base, deltas, k0 = make_sessions(20241009, S)
    rcv, snd = engine.IKNPMultiReceiver(ctx, base), engine.IKNPMultiSender(ctx, deltas, k0)
    out = ctx.empty(S * u_bytes(per) + 16 * S * per + 64).zero(SENTINEL)
    q = C.c_void_p(out.ptr)
    host = np.zeros(S * u_bytes(per) + 16 * S * per, np.uint8)
    hp = host.ctypes.data_as(C.c_void_p)
    st = C.c_int(0)
    # S = 0 and NULLs at create
    for call in (lambda: L.gc_iknp_multi_receiver_create(ctx.h, hp, 0, C.byref(st)),
                 lambda: L.gc_iknp_multi_receiver_create(ctx.h, None, S, C.byref(st)),
                 lambda: L.gc_iknp_multi_receiver_create_dev(ctx.h, None, S, C.byref(st)),
                 lambda: L.gc_iknp_multi_sender_create(ctx.h, None, hp, S, C.byref(st)),
                 lambda: L.gc_iknp_multi_sender_create(ctx.h, hp, None, S, C.byref(st)),
                 lambda: L.gc_iknp_multi_sender_create_dev(ctx.h, q, q, 0, C.byref(st)),
                 lambda: L.gc_iknp_multi_sender_create(None, hp, hp, S, C.byref(st))):
        st.value = OK
        assert not call() and st.value == E_ARG
    assert not L.gc_iknp_multi_receiver_create(ctx.h, hp, 0, None)  # status may be NULL
    # the wrong role
    assert L.gc_iknp_multi_receive_dev(snd.h, q, per, q, q) == E_ARG
    assert L.gc_iknp_multi_receive(snd.h, hp, per, hp, hp) == E_ARG
    assert L.gc_iknp_multi_send_dev(rcv.h, q, per, q) == E_ARG
    assert L.gc_iknp_multi_send(rcv.h, hp, S * u_bytes(per), per, hp) == E_ARG
    # NULL handle and arrays
    assert L.gc_iknp_multi_receive_dev(None, q, per, q, q) == E_ARG
    for args in ((None, per, q, q), (q, per, None, q), (q, per, q, None)):
        assert L.gc_iknp_multi_receive_dev(rcv.h, *args) == E_ARG
        assert L.gc_iknp_multi_receive(rcv.h, *[hp if a is q else a for a in args]) == E_ARG
    assert L.gc_iknp_multi_send_dev(snd.h, None, per, q) == E_ARG and L.gc_iknp_multi_send_dev(snd.h, q, per, None) == E_ARG
    assert L.gc_iknp_multi_send(snd.h, None, S * u_bytes(per), per, hp) == E_ARG
    assert L.gc_iknp_multi_send(snd.h, hp, S * u_bytes(per), per, None) == E_ARG
    # u_len is S * gc_iknp_u_bytes(per), not one session's and not a byte more
    for bad in (u_bytes(per), S * u_bytes(per) + 1, S * u_bytes(per) - 1, 0):
        assert L.gc_iknp_multi_send(snd.h, hp, bad, per, hp) == E_ARG
    # sizes that do not fit size_t
    top = C.c_size_t(-1).value
    for big in (top // 2, top // S, top // 64):
        assert L.gc_iknp_multi_receive_dev(rcv.h, q, big, q, q) == E_ARG and L.gc_iknp_multi_send_dev(snd.h, q, big, q) == E_ARG
        assert L.gc_cot_multi_send_pads_dev(ctx.h, q, q, q, q, S, big, q) == E_ARG
        assert L.gc_cot_multi_receive_unpad_dev(ctx.h, q, q, q, q, S, big) == E_ARG
    # the COT calls: S = 0, NULL ctx, NULL arrays
    assert L.gc_cot_multi_send_pads_dev(ctx.h, q, q, q, q, 0, per, q) == E_ARG
    assert L.gc_cot_multi_receive_unpad_dev(ctx.h, q, q, q, q, 0, per) == E_ARG
    assert L.gc_cot_multi_send_pads(ctx.h, hp, hp, hp, hp, 0, per, hp) == E_ARG
    assert L.gc_cot_multi_receive_unpad(ctx.h, hp, hp, hp, hp, 0, per) == E_ARG
    assert L.gc_cot_multi_send_pads_dev(None, q, q, q, q, S, per, q) == E_ARG
    for k in range(5):
        args = [q] * 5
        args[k] = None
        assert L.gc_cot_multi_send_pads_dev(ctx.h, args[0], args[1], args[2], args[3], S, per, args[4]) == E_ARG
    for k in range(4):
        args = [q] * 4
        args[k] = None
        assert L.gc_cot_multi_receive_unpad_dev(ctx.h, *args, S, per) == E_ARG
    # inside a capture every call of the handle is refused: the position is a kernel argument
    for call in (lambda: rcv.receive_dev(out, per, out, out), lambda: snd.send_dev(out, per, out),
                 lambda: engine.IKNPMultiReceiver(ctx, base)):
        with pytest.raises(engine.EngineError) as e:
            ctx.capture(call)
        assert e.value.code == E_ARG
    # per = 0: GC_OK, nothing written, the position stays — with or without arrays
    assert L.gc_iknp_multi_receive_dev(rcv.h, q, 0, q, q) == OK and L.gc_iknp_multi_receive_dev(rcv.h, None, 0, None, None) == OK
    assert L.gc_iknp_multi_send_dev(snd.h, q, 0, q) == OK and L.gc_iknp_multi_send(snd.h, None, 0, 0, None) == OK
    assert L.gc_iknp_multi_receive(rcv.h, None, 0, None, None) == OK
    assert L.gc_cot_multi_send_pads_dev(ctx.h, q, q, q, q, S, 0, q) == OK
    assert L.gc_cot_multi_receive_unpad_dev(ctx.h, q, q, q, q, S, 0) == OK
    assert L.gc_cot_multi_send_pads(ctx.h, None, None, None, None, S, 0, None) == OK
    ctx.sync()
    assert (out.numpy() == SENTINEL).all() and not host.any(), "a refused or empty call wrote something"
    assert rcv.info() == (S, True, 0) and snd.info() == (S, False, 0), "a refused or empty call moved the position"
    # and the handles still serve: the bytes of a fresh pair
    b = rng.integers(0, 2, (S, per)).astype(np.uint8)
    u, got, sent = OracleSessions(base, deltas, k0).call(b, per)
    have_u, have_got = rcv.receive(b.reshape(-1), per)
    assert have_u == u and have_got.tobytes() == got.tobytes() and snd.send(u, per).tobytes() == sent.tobytes()
    rcv.close()
    snd.close()
