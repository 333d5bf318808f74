"""The persistent OT kernels past one trip of their capped grids, and MITCCRH at key indices other than zero, byte for byte
against the C oracle (and, at chosen indices, against tests/py_ot_reference.py).

k_cot_dual (MITCCRH, COT, ROT) and k_kos_accumulate launch at most kCotGrid workgroups of kCotThreads lanes and loop over the
rest; k_iknp_fused launches at most kIknpGrid workgroups that walk groups of 4 (receiver) or 8 (sender) chunks.  The sizes
here are the smallest that reach the second trip with a ragged tail, and they are derived from the constants of
mpc_amd/csrc/kernels.h, so that a changed cap moves the tests along:

  N_COT  = one sweep + one full workgroup + 37 lanes
  N_RECV = (kIknpGrid * 4 + 1) chunks + 37 rows: receiver group kIknpGrid is the first of workgroup 0's second trip and holds
           a full chunk, a chunk of 37 rows and two chunks that do not exist
  N_SEND = (kIknpGrid * 8 + 1) chunks + 37 rows: the same for the sender; the receiver's workgroup 0 makes three trips

The labels IKNP would hand to COT / ROT / KOS are made in numpy with the IKNP correlation (received = sent ^ choice * delta,
iknp_test.go:98-113): the pads and tags do not care where their labels came from."""
import numpy as np
import pytest

import oracle
from mpc_amd import engine
from mpc_amd.circuit import LABEL, WIRE
from tests import py_ot_reference as po
from tests.util import kernel_constants

pytestmark = pytest.mark.gpu

COT_THREADS, COT_GRID = kernel_constants("kCotThreads", "kCotGrid")
IKNP_GRID, IKNP_RECV_CHUNKS, IKNP_SEND_CHUNKS = kernel_constants("kIknpGrid", "kIknpRecvChunks", "kIknpSendChunks")
CHUNK = 512  # OTs per IKNP chunk (iknp.go:58)
COT_SWEEP = COT_GRID * COT_THREADS  # OTs of one trip of k_cot_dual / k_kos_accumulate
N_COT = COT_SWEEP + COT_THREADS + 37
N_RECV = (IKNP_GRID * IKNP_RECV_CHUNKS + 1) * CHUNK + 37
N_SEND = (IKNP_GRID * IKNP_SEND_CHUNKS + 1) * CHUNK + 37
M64 = (1 << 64) - 1
GUARD = 16  # bytes of sentinel either side of a device output (the kernels store 16-byte words)
SENTINEL = 0xC3


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


def assert_past_cot_sweep(n):
    """sweep two of k_cot_dual / k_kos_accumulate has a full workgroup and a ragged one"""
    assert n > COT_SWEEP + COT_THREADS and (n - COT_SWEEP) % COT_THREADS != 0


def iknp_groups(n, chunks_per_group):
    return -(-(-(-n // CHUNK)) // chunks_per_group)


def rand_labels(rng, n):
    out = np.zeros(n, LABEL)
    out["d0"] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    out["d1"] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    return out


def rand_label(rng):
    l = rand_labels(rng, 1)[0]
    return int(l["d0"]), int(l["d1"])


def tup(l):
    return int(l["d0"]), int(l["d1"])


def xor_where(labels, flags, delta):
    """labels ^ flags * delta"""
    out = labels.copy()
    f = np.asarray(flags).astype(bool)
    out["d0"][f] ^= np.uint64(delta[0])
    out["d1"][f] ^= np.uint64(delta[1])
    return out


def label_u8(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class Guarded:
    """a device buffer between two sentinel words; read() checks that the kernel left them alone"""

    def __init__(self, ctx, nbytes, data=None):
        assert nbytes % 16 == 0
        self.buf = ctx.empty(nbytes + 2 * GUARD).zero(SENTINEL)
        if data is not None:
            self.buf.upload(label_u8(data), GUARD)
        self.ptr = self.buf + GUARD

    def read(self):
        raw = self.buf.numpy()
        assert (raw[:GUARD] == SENTINEL).all(), "the word before the output was written"
        assert (raw[-GUARD:] == SENTINEL).all(), "the word behind the output was written"
        return raw[GUARD:-GUARD]


# ---- MITCCRH -------------------------------------------------------------------------------------------------------


def oracle_mitccrh(seed, gid0, blks, h):
    """the C oracle's MITCCRH object with its key counter preset, driven 8 keys per call as cot.go:160-171 drives it"""
    m = oracle.MITCCRH(seed, 8)
    m.s.gid = gid0
    want = np.ascontiguousarray(blks, dtype=LABEL).copy()
    n = len(want) // h
    full = n - n % 8
    for i in range(0, full, 8):
        m.hash(want[i * h:(i + 8) * h], 8, h)  # a slice of a contiguous array: hashed in place
    if n > full:
        pad = np.zeros(8 * h, LABEL)
        pad[:(n - full) * h] = want[full * h:]
        m.hash(pad, 8, h)
        want[full * h:] = pad[:(n - full) * h]
    return want


def py_mitccrh(seed, gid, blocks):
    """H(x) = AES_key(gid)(x) ^ x for the blocks of one OT, key = BE(Label{gid, 0} ^ seed) (mitccrh.go:70-128), through the
    Python restatement: a one-key batch whose counter starts at gid"""
    m = po.Mitccrh(seed, batch=1)
    m.gid = gid & M64
    return m.hash(list(blocks), 1, len(blocks))


def spot_indices(n, special, rng_seed, count=64):
    """the first 8, the 8 each side of every index in `special`, the last 8, and seeded ones up to `count`"""
    idx = set(range(8)) | set(range(n - 8, n))
    for s in special:
        idx |= set(range(s - 8, s + 8))
    idx = {i for i in idx if 0 <= i < n}
    rng = np.random.default_rng(rng_seed)
    while len(idx) < count:
        idx.add(int(rng.integers(0, n)))
    return sorted(idx)


@pytest.fixture(scope="module")
def mitccrh_inputs():
    rng = np.random.default_rng(20240601)
    return rand_label(rng), rand_labels(rng, 2 * N_COT)


GID0S = [0, (1 << 32) - 1000, (1 << 64) - 1000]


@pytest.mark.parametrize("h", [1, 2])
@pytest.mark.parametrize("gid0", GID0S)
def test_mitccrh_past_one_sweep_and_across_the_key_carry(ctx, mitccrh_inputs, gid0, h):
    """gc_mitccrh_hash at N_COT: the key index gid0 + j carries into the high key word (gid0 = 2^32 - 1000) or wraps at 2^64
    (2^64 - 1000) at j = 1000, inside sweep one, and sweep two runs past it"""
    n = N_COT
    assert_past_cot_sweep(n)
    seed, pool = mitccrh_inputs
    blks = pool[:n * h]
    got = engine.mitccrh_hash(ctx, seed, gid0, blks, h)
    want = oracle_mitccrh(seed, gid0, blks, h)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "first differing block %d (OT %d) of %d" % (bad[0], bad[0] // h, bad.size)
    carry = [1000] if gid0 else []
    assert all((gid0 + c) & 0xFFFFFFFF == 0 for c in carry)
    for j in spot_indices(n, carry + [COT_SWEEP], gid0 % 1009 + h):
        x = [tup(blks[j * h + t]) for t in range(h)]
        assert [tup(got[j * h + t]) for t in range(h)] == py_mitccrh(seed, gid0 + j, x), j


@pytest.mark.parametrize("gid0", [0, (1 << 32) - 5])
@pytest.mark.parametrize("n", [13, 1000])
@pytest.mark.parametrize("h", [3, 4])
def test_mitccrh_more_than_two_blocks_per_key(ctx, h, n, gid0):
    """h > 2 goes to the one-OT-per-thread kernel (k_mitccrh) whatever GC_COT_CLASSIC says"""
    rng = np.random.default_rng(7 * h + n)
    seed, blks = rand_label(rng), rand_labels(rng, n * h)
    got = engine.mitccrh_hash(ctx, seed, gid0, blks, h)
    assert (got == oracle_mitccrh(seed, gid0, blks, h)).all()
    for j in (0, 4, 5, n - 1):  # 5: the first index past the carry of gid0 = 2^32 - 5
        x = [tup(blks[j * h + t]) for t in range(h)]
        assert [tup(got[j * h + t]) for t in range(h)] == py_mitccrh(seed, gid0 + j, x), j


# ---- COT / ROT -----------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def cot_case():
    """inputs at N_COT and the oracle's bytes of the four pad loops, computed once"""
    n = N_COT
    rng = np.random.default_rng(20240602)
    seed, delta = rand_label(rng), rand_label(rng)
    data = rand_labels(rng, n)  # the sender's IKNP labels
    flags = rng.integers(0, 2, n).astype(np.uint8)
    recv = xor_where(data, flags, delta)  # the receiver's
    wires = np.zeros(n, WIRE)
    wires["l0"], wires["l1"] = rand_labels(rng, n), rand_labels(rng, n)
    sent = oracle.cot_send_pads(seed, delta, data, wires)
    return dict(n=n, seed=seed, delta=delta, data=data, flags=flags, recv=recv, wires=wires, sent=sent,
                res=oracle.cot_receive_unpad(seed, flags, sent, recv), rot_wires=oracle.rot_send(seed, delta, data),
                rot_res=oracle.rot_receive(seed, recv))


def chosen(wires, flags):
    return np.where(np.asarray(flags).astype(bool), wires["l1"], wires["l0"])


def test_cot_pads_past_one_sweep(ctx, cot_case):
    c = cot_case
    assert_past_cot_sweep(c["n"])
    sent = engine.cot_send_pads(ctx, c["seed"], c["delta"], c["data"], c["wires"])
    assert sent.tobytes() == c["sent"].tobytes(), "COT.Send pads differ from the oracle"
    res = engine.cot_receive_unpad(ctx, c["seed"], c["flags"], sent, c["recv"])
    assert res.tobytes() == c["res"].tobytes(), "COT.Receive labels differ from the oracle"
    assert (res == chosen(c["wires"], c["flags"])).all(), "result[j] == wires[j].L{flag_j}"


def test_rot_pads_past_one_sweep(ctx, cot_case):
    c = cot_case
    assert_past_cot_sweep(c["n"])
    wires = engine.rot_send(ctx, c["seed"], c["delta"], c["data"])
    assert wires.tobytes() == c["rot_wires"].tobytes(), "ROT.Send wires differ from the oracle"
    res = engine.rot_receive(ctx, c["seed"], c["recv"])
    assert res.tobytes() == c["rot_res"].tobytes(), "ROT.Receive pads differ from the oracle"
    assert (res == chosen(wires, c["flags"])).all(), "result[j] == wires[j].L{flag_j}"


def test_cot_rot_device_chain_past_one_sweep(ctx, cot_case):
    """the device-pointer forms, every output between two sentinel words: the bytes of the host forms, which are the oracle's"""
    c = cot_case
    n, seed, delta = c["n"], c["seed"], c["delta"]
    assert_past_cot_sweep(n)
    d_data, d_flags, d_wires = ctx.to_device(label_u8(c["data"])), ctx.to_device(c["flags"]), ctx.to_device(label_u8(c["wires"]))
    g_rot_w = Guarded(ctx, 32 * n)
    g_rot_r = Guarded(ctx, 16 * n, c["recv"])
    g_sent = Guarded(ctx, 32 * n)
    g_res = Guarded(ctx, 16 * n, c["recv"])
    engine.rot_send_dev(ctx, seed, delta, d_data, n, g_rot_w.ptr)
    engine.rot_receive_dev(ctx, seed, g_rot_r.ptr, n)
    engine.cot_send_pads_dev(ctx, seed, delta, d_data, d_wires, n, g_sent.ptr)
    engine.cot_receive_unpad_dev(ctx, seed, d_flags, g_sent.ptr, g_res.ptr, n)
    ctx.sync()
    host = dict(rot_wires=engine.rot_send(ctx, seed, delta, c["data"]), rot_res=engine.rot_receive(ctx, seed, c["recv"]),
                sent=engine.cot_send_pads(ctx, seed, delta, c["data"], c["wires"]))
    host["res"] = engine.cot_receive_unpad(ctx, seed, c["flags"], host["sent"], c["recv"])
    for name, g in (("rot_wires", g_rot_w), ("rot_res", g_rot_r), ("sent", g_sent), ("res", g_res)):
        raw = g.read().tobytes()
        assert raw == c[name].tobytes(), "%s: the device form differs from the oracle" % name
        assert raw == host[name].tobytes(), "%s: the device form differs from the host form" % name


# ---- KOS -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("past", [0, 1, N_COT - COT_SWEEP])
def test_kos_check_with_more_than_one_ot_per_lane(ctx, past):
    """k_kos_accumulate keeps XOR-ing a lane's OTs into the lane's own 256-bit accumulator.  One sweep exactly: every lane of
    the full grid has one OT; + 1: lane 0 of workgroup 0 is the first with two; N_COT: a full workgroup and a ragged one have
    two.  A bit flipped in a lane's SECOND OT must fail the sender's check."""
    n = COT_SWEEP + past
    if past > 1:
        assert_past_cot_sweep(n)
    rng = np.random.default_rng(20240603 + n % 1000)
    seed2, delta = rand_label(rng), rand_label(rng)
    sent = rand_labels(rng, n)
    b = rng.integers(0, 2, n).astype(np.uint8)
    got = xor_where(sent, b, delta)
    cvs = rand_labels(rng, 256)
    bcv = rng.integers(0, 2, 256).astype(np.uint8)
    cvr = xor_where(cvs, bcv, delta)
    want = oracle.kos_receiver_tags(seed2, got, b, cvr, bcv)
    have = engine.kos_receiver_tags(ctx, seed2, got, b, cvr, bcv)
    assert have == want, "the receiver's tags differ from the oracle"
    x, t0, t1 = want
    assert oracle.kos_sender_check(seed2, sent, cvs, delta, x, t0, t1)  # the inputs are a consistent IKNP run
    assert engine.kos_sender_check(ctx, seed2, sent, cvs, delta, x, t0, t1)
    flip = COT_SWEEP + 5 if n > COT_SWEEP + 5 else n - 1  # n - 1: the last single-OT lane, or lane 0's second OT
    assert (flip >= COT_SWEEP) == (n > COT_SWEEP)
    bad = sent.copy()
    bad[flip]["d1"] ^= np.uint64(1 << 40)
    assert not oracle.kos_sender_check(seed2, bad, cvs, delta, x, t0, t1)
    assert not engine.kos_sender_check(ctx, seed2, bad, cvs, delta, x, t0, t1)
    d_got, d_sent, d_bad, d_b = (ctx.to_device(label_u8(got)), ctx.to_device(label_u8(sent)), ctx.to_device(label_u8(bad)),
                                 ctx.to_device(b))
    assert engine.kos_receiver_tags_dev(ctx, seed2, d_got, d_b, n, cvr, bcv) == want
    assert engine.kos_sender_check_dev(ctx, seed2, d_sent, n, cvs, delta, x, t0, t1)
    assert not engine.kos_sender_check_dev(ctx, seed2, d_bad, n, cvs, delta, x, t0, t1)


# ---- IKNP ----------------------------------------------------------------------------------------------------------


def base_setup(rng):
    """what the base OTs leave: the receiver's 128 label pairs, the sender's delta and its label of every pair"""
    base = np.zeros(128, WIRE)
    base["l0"], base["l1"] = rand_labels(rng, 128), rand_labels(rng, 128)
    delta = rand_label(rng)
    bits = np.array([po.bit(delta, i) for i in range(128)], bool)
    return base, delta, np.where(bits, base["l1"], base["l0"])


def assert_correlated(got, sent, b, delta):
    assert (got == xor_where(sent, b, delta)).all(), "rcvd = sent ^ b * delta (iknp_test.go:98-113)"


@pytest.mark.parametrize("variant", ["position_0", "mid_block_generic"])
def test_iknp_receive_past_one_sweep(ctx, monkeypatch, variant):
    """the receiver's workgroup 0 takes a second group, a ragged one: it reuses its LDS chunk buffers behind the barrier of
    the loop, with two of its four chunk slices idle.  mid_block_generic: a first call of 40 OTs leaves every column stream
    5 bytes into a block (the MISALIGNED instantiation), with the general first AES round (GC_IKNP_GENERIC=1)."""
    n = N_RECV
    chunks = -(-n // CHUNK)
    assert iknp_groups(n, IKNP_RECV_CHUNKS) > IKNP_GRID and chunks % IKNP_RECV_CHUNKS != 0 and n % CHUNK != 0
    rng = np.random.default_rng(20240604)
    base, delta, k0 = base_setup(rng)
    rcv, snd = engine.IKNPReceiver(ctx, base), engine.IKNPSender(ctx, delta, k0)
    orcv, osnd = oracle.IKNPReceiver(base), oracle.IKNPSender(delta, k0)
    sizes = [n]
    if variant == "mid_block_generic":
        monkeypatch.setenv("GC_IKNP_GENERIC", "1")
        sizes = [40, n]
    for m in sizes:
        b = rng.integers(0, 2, m).astype(np.uint8)
        u, got = rcv.receive(b)
        ou, ogot = orcv.receive(b)
        assert u == ou, "u-matrix bytes differ from the oracle (%d OTs)" % m
        assert got.tobytes() == ogot.tobytes(), "receiver labels differ from the oracle (%d OTs)" % m
        sent = snd.send(u, m)
        assert sent.tobytes() == osnd.send(ou, m).tobytes(), "sender labels differ from the oracle (%d OTs)" % m
        assert_correlated(got, sent, b, delta)
    rcv.close(); snd.close()


def test_iknp_bits_past_one_sweep(ctx):
    """ReceiveBits / SendBits at the same n: not a multiple of 64, so the fold of whole choice words only is live (the last
    chunk, 37 rows, folds none)"""
    n = N_RECV
    assert iknp_groups(n, IKNP_RECV_CHUNKS) > IKNP_GRID and n % 64 != 0
    rng = np.random.default_rng(20240605)
    base, delta, k0 = base_setup(rng)
    choices = rng.integers(0, 1 << 64, (n + 63) // 64, dtype=np.uint64)
    rcv, snd = engine.IKNPReceiver(ctx, base), engine.IKNPSender(ctx, delta, k0)
    orcv, osnd = oracle.IKNPReceiver(base), oracle.IKNPSender(delta, k0)
    u, r = rcv.receive_bits(choices, n)
    ou, orr = oracle.iknp_receive_bits(orcv, choices, n)
    assert u == ou, "u-matrix bytes differ from the oracle"
    assert (r == orr).all(), "the receiver's bit words differ from the oracle"
    s = snd.send_bits(u, n)
    assert (s == oracle.iknp_send_bits(osnd, ou, n)).all(), "the sender's bit words differ from the oracle"
    rcv.close(); snd.close()


@pytest.fixture(scope="module")
def send_case():
    """one oracle run at N_SEND from stream position 0, shared by the sender's and the receiver's test"""
    n = N_SEND
    rng = np.random.default_rng(20240606)
    base, delta, k0 = base_setup(rng)
    b = rng.integers(0, 2, n).astype(np.uint8)
    u, got = oracle.IKNPReceiver(base).receive(b)
    sent = oracle.IKNPSender(delta, k0).send(u, n)
    assert_correlated(got, sent, b, delta)
    return dict(n=n, base=base, delta=delta, k0=k0, b=b, u=u, got=got, sent=sent)


def test_iknp_send_past_one_sweep(ctx, send_case):
    """the sender's workgroup 0 takes a second group of eight chunk slots of which two exist; host and device-pointer form,
    fed with the ORACLE receiver's u"""
    c = send_case
    n = c["n"]
    chunks = -(-n // CHUNK)
    assert iknp_groups(n, IKNP_SEND_CHUNKS) > IKNP_GRID and chunks % IKNP_SEND_CHUNKS != 0 and n % CHUNK != 0
    snd = engine.IKNPSender(ctx, c["delta"], c["k0"])
    sent = snd.send(c["u"], n)
    assert sent.tobytes() == c["sent"].tobytes(), "sender labels differ from the oracle"
    snd.close()
    snd = engine.IKNPSender(ctx, c["delta"], c["k0"])
    d_u = ctx.zeros(chunks * 8192)
    d_u.upload(np.frombuffer(c["u"], np.uint8))
    g_lab = Guarded(ctx, 16 * n)
    snd.send_dev(d_u, n, g_lab.ptr)
    ctx.sync()
    assert g_lab.read().tobytes() == c["sent"].tobytes(), "send_dev labels differ from the oracle"
    snd.close()


def test_iknp_receive_three_trips(ctx, send_case):
    c = send_case
    n = c["n"]
    assert iknp_groups(n, IKNP_RECV_CHUNKS) > 2 * IKNP_GRID
    rcv = engine.IKNPReceiver(ctx, c["base"])
    u, got = rcv.receive(c["b"])
    assert u == c["u"], "u-matrix bytes differ from the oracle"
    assert got.tobytes() == c["got"].tobytes(), "receiver labels differ from the oracle"
    rcv.close()
