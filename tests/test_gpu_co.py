"""The Chou-Orlandi base OT on the device (gc_co_*, mpc_amd/csrc/co_kernels.hip) against the restated reference
(tests/py_co_reference.py, checked on the CPU by tests/test_py_co_reference.py): byte parity of the three kernels in host
and device-pointer form, coordinates with leading zero bytes, hostile points, Go's round constants, the hand-over to IKNP,
and misuse.  The restatement costs about 4 ms per scalar multiplication, so every expected value is computed once per
module, on a pool of 257 OTs that every size takes its first n from (the id of OT i is id0 + i for every n)."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import oracle
from mpc_amd import engine
from mpc_amd.circuit import LABEL, WIRE
from tests import go_transcript as gt
from tests import py_co_reference as co
from tests.test_py_co_reference import go_session, round2_hash
from tests.util import drbg, kernel_constants

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 257]  # wave and workgroup edges, a second, ragged workgroup (the grid-stride loops make one trip)
CO_THREADS, CO_GRID = kernel_constants("kCoThreads", "kCoGrid")
CO_SWEEP = CO_GRID * CO_THREADS  # OTs of one trip of the capped grid
N_CO = CO_SWEEP + CO_THREADS + 37  # the second trip has a full workgroup and one with 37 live lanes
ID0S = [0, (1 << 32) + 5]
POOL = 257
TOP = 1 << 256


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


def labels_from_bytes(raws):
    be = np.frombuffer(b"".join(raws), ">u8").reshape(-1, 2)
    out = np.zeros(len(be), LABEL)
    out["d0"], out["d1"] = be[:, 0], be[:, 1]
    return out


def wires_of(pairs):
    w = np.zeros(len(pairs), WIRE)
    if len(pairs):
        w["l0"] = labels_from_bytes([p[0] for p in pairs])
        w["l1"] = labels_from_bytes([p[1] for p in pairs])
    return w


def points_array(points):
    return np.frombuffer(b"".join(co.point_bytes(p) for p in points), np.uint8).reshape(-1, 64).copy()


def scalars_array(scalars):
    return np.frombuffer(b"".join(s.to_bytes(32, "big") for s in scalars), np.uint8).reshape(-1, 32).copy()


def ct_bytes(ct):
    return [bytes(c) for c in np.asarray(ct).reshape(-1, 32)]


def label_raw(labels):
    raw = gt.label_bytes(labels)
    return [raw[16 * i:16 * i + 16] for i in range(len(labels))]


def pick(wires, choice):
    """L_choice of every wire"""
    out = wires["l0"].copy()
    out[choice == 1] = wires["l1"][choice == 1]
    return out


def masks_xor(pt, idx, label):
    return bytes(x ^ y for x, y in zip(co.mask(pt, idx), label))


@pytest.fixture(scope="module")
def pool():
    """one session and 257 OTs: the curve results of the restatement (S, T, B, b * A), from which the bytes for any id0
    follow by hashing alone"""
    a = int.from_bytes(drbg("co/gpu/a", 32), "big")
    A, AaInv = co.sender_setup(a)
    edge = [0, 1, co.N - 1, co.N, TOP - 1, co.N + 1, 2]
    scalars = [int.from_bytes(drbg("co/gpu/b%d" % i, 32), "big") for i in range(POOL)]
    # the edge scalars among the first 63, so that every size but 1 meets them; OT 0 is a plain one
    for k, e in enumerate(edge):
        scalars[3 + 7 * k] = e
    choice = (np.frombuffer(drbg("co/gpu/choice", POOL), np.uint8) & 1).astype(np.uint8)
    choice[3], choice[24] = 1, 1  # b = 0 and b = N with the choice set: B = A exactly ...
    scalars[52], choice[52] = 0, 0  # ... and without it B is the point at infinity, which the sender then refuses
    pairs = [(drbg("co/gpu/l0/%d" % i, 16), drbg("co/gpu/l1/%d" % i, 16)) for i in range(POOL)]
    B = co.receiver_choices(A, scalars, list(choice))
    D = [co.mul(A, b) for b in scalars]
    infinite = [i for i, p in enumerate(B) if p == co.INF]
    assert infinite == [i for i in range(POOL) if scalars[i] % co.N == 0 and not choice[i]]
    S = [co.INF if i in infinite else co.mul(p, a) for i, p in enumerate(B)]
    T = [co.add(s, AaInv) for s in S]
    return dict(a=a, A=A, AaInv=AaInv, scalars=scalars, choice=choice, pairs=pairs, wires=wires_of(pairs), B=B, D=D, S=S, T=T,
                infinite=infinite)


def expected_ct(pool, n, id0):
    out = []
    for i in range(n):
        if i in pool["infinite"]:
            out.append(bytes(32))
        else:
            out.append(masks_xor(pool["S"][i], id0 + i, pool["pairs"][i][0]) + masks_xor(pool["T"][i], id0 + i, pool["pairs"][i][1]))
    return out


def expected_labels(pool, n, id0, cts):
    return [masks_xor(pool["D"][i], id0 + i, cts[i][16:] if pool["choice"][i] else cts[i][:16]) for i in range(n)]


def run_host(ctx, pool, n, id0):
    A, AaInv = co.point_bytes(pool["A"]), co.point_bytes(pool["AaInv"])
    sc, ch = scalars_array(pool["scalars"][:n]), pool["choice"][:n]
    pts = engine.co_receiver_choices(ctx, A, sc, ch)
    bad = None
    try:
        ct = engine.co_sender_encrypt(ctx, pool["a"], AaInv, pts, pool["wires"][:n], id0)
    except engine.CoPointError as e:
        ct, bad = e.ct, e.bad_index
    labels = engine.co_receiver_decrypt(ctx, A, sc, ch, ct, id0)
    return pts, ct, labels, bad


def run_dev(ctx, pool, n, id0):
    A, AaInv = co.point_bytes(pool["A"]), co.point_bytes(pool["AaInv"])
    m = max(n, 1)
    d_sc = ctx.to_device(scalars_array(pool["scalars"][:m]))
    d_ch = ctx.to_device(pool["choice"][:m].copy())
    d_w = ctx.to_device(pool["wires"][:m].copy())
    sentinel = 0xA5
    d_pts, d_ct, d_lab = ctx.empty((m, 64)).zero(sentinel), ctx.empty((m, 32)).zero(sentinel), ctx.empty((m, 16)).zero(sentinel)
    d_status = ctx.empty(2, np.uint64).zero(sentinel)
    engine.co_receiver_choices_dev(ctx, A, d_sc, d_ch, n, d_pts)
    engine.co_sender_encrypt_dev(ctx, pool["a"], AaInv, d_pts, d_w, n, id0, d_ct, d_status)
    engine.co_receiver_decrypt_dev(ctx, A, d_sc, d_ch, d_ct, n, id0, d_lab)
    ctx.sync()
    pts, ct, lab, status = d_pts.numpy(), d_ct.numpy(), d_lab.numpy(), d_status.numpy()
    if n == 0:  # nothing written, the status block included
        assert (pts == sentinel).all() and (ct == sentinel).all() and (lab == sentinel).all()
        assert (status.view(np.uint8) == sentinel).all()
        return pts[:0], ct[:0], np.zeros(0, LABEL), None
    labels = np.frombuffer(lab.tobytes(), LABEL)
    count, lowest = int(status[0]), int(status[1])
    assert (count == 0) == (lowest == (1 << 64) - 1)
    return pts, ct, labels, (lowest if count else None, count)


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("id0", ID0S)
@pytest.mark.parametrize("n", SIZES)
def test_byte_parity(ctx, pool, n, id0, form):
    pts, ct, labels, bad = (run_host if form == "host" else run_dev)(ctx, pool, n, id0)
    assert [bytes(p) for p in pts] == [co.point_bytes(p) for p in pool["B"][:n]], "choice points differ"
    want_ct = expected_ct(pool, n, id0)
    assert ct_bytes(ct) == want_ct, "ciphertexts differ"
    want_bad = [i for i in pool["infinite"] if i < n]  # b = 0 mod N without the choice: the receiver sent infinity
    if form == "host":
        assert bad == (want_bad[0] if want_bad else None)
    elif n:
        assert bad == ((want_bad[0], len(want_bad)) if want_bad else (None, 0))
    assert label_raw(labels) == expected_labels(pool, n, id0, want_ct), "decrypted labels differ"
    for i in range(n):  # decrypt(encrypt) = L_choice
        if i not in want_bad:
            assert label_raw(labels[i:i + 1])[0] == pool["pairs"][i][pool["choice"][i]], i


def test_past_one_grid_sweep(ctx):
    """N_CO OTs through the device-pointer forms: every lane of the first CO_THREADS + 37 makes a second trip of its
    grid-stride loop.  decrypt(encrypt(choices)) = L_choice for every OT, and point, ciphertext and label equal the
    restatement's bytes at 24 indices (both sides of the sweep edge among them).  Then the sender meets two hostile points,
    one in each trip."""
    n, id0 = N_CO, (1 << 32) - 7  # the id carries into its high word at OT 7
    assert n > CO_SWEEP + CO_THREADS and (n - CO_SWEEP) % CO_THREADS != 0
    rng = np.random.default_rng(20240607)
    a = int.from_bytes(drbg("co/sweep/a", 32), "big")
    A, AaInv = co.sender_setup(a)
    Ab, AaInvb = co.point_bytes(A), co.point_bytes(AaInv)
    scalars = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    choice = rng.integers(0, 2, n).astype(np.uint8)
    wires = np.zeros(n, WIRE)
    for half in ("l0", "l1"):
        wires[half]["d0"] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        wires[half]["d1"] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    d_sc, d_ch, d_w = ctx.to_device(scalars), ctx.to_device(choice), ctx.to_device(wires)
    sentinel = 0xA5
    d_pts, d_ct, d_lab = ctx.empty((n, 64)).zero(sentinel), ctx.empty((n, 32)).zero(sentinel), ctx.empty((n, 16)).zero(sentinel)
    d_status = ctx.empty(2, np.uint64).zero(sentinel)
    engine.co_receiver_choices_dev(ctx, Ab, d_sc, d_ch, n, d_pts)
    engine.co_sender_encrypt_dev(ctx, a, AaInvb, d_pts, d_w, n, id0, d_ct, d_status)
    engine.co_receiver_decrypt_dev(ctx, Ab, d_sc, d_ch, d_ct, n, id0, d_lab)
    ctx.sync()
    pts, ct = d_pts.numpy(), d_ct.numpy()
    labels = np.frombuffer(d_lab.numpy().tobytes(), LABEL)
    assert [int(v) for v in d_status.numpy()] == [0, (1 << 64) - 1]
    want = pick(wires, choice)
    bad = np.flatnonzero(labels != want)
    assert bad.size == 0, "decrypt(encrypt) != L_choice at %d OTs, the first %d" % (bad.size, bad[0])
    idx = {0, 1, n - 2, n - 1} | set(range(CO_SWEEP - 4, CO_SWEEP + 4))
    while len(idx) < 24:
        idx.add(int(rng.integers(0, n)))
    for i in sorted(idx):
        b, c = int.from_bytes(bytes(scalars[i]), "big"), int(choice[i])
        pair = (label_raw(wires["l0"][i:i + 1])[0], label_raw(wires["l1"][i:i + 1])[0])
        B = co.receiver_choices(A, [b], [c])
        assert bytes(pts[i]) == co.point_bytes(B[0]), "choice point %d" % i
        cts, none_bad = co.sender_encrypt(a, AaInv, B, [pair], id0 + i)
        assert not none_bad and bytes(ct[i]) == cts[0], "ciphertext %d" % i
        assert label_raw(labels[i:i + 1]) == co.receiver_decrypt(A, [b], [c], cts, id0 + i) == [pair[c]], "label %d" % i
    # a second encrypt of the same points, two of them hostile: one off the curve in the second trip, x = p in the first
    off, xp = CO_SWEEP + 12, 700
    assert xp < CO_SWEEP < off < n
    x, y = co.point_from_bytes(bytes(pts[off]))
    hostile = {off: (x, (y + 1) % co.P), xp: HOSTILE["x_equals_p"]}
    for at, p in hostile.items():
        assert not co.valid_point(p)
        d_pts.upload(np.frombuffer(co.point_bytes(p), np.uint8), 64 * at)
    d_ct2 = ctx.empty((n, 32)).zero(sentinel)
    engine.co_sender_encrypt_dev(ctx, a, AaInvb, d_pts, d_w, n, id0, d_ct2, d_status)
    ctx.sync()
    assert [int(v) for v in d_status.numpy()] == [2, xp]
    ct2 = d_ct2.numpy()
    for at in hostile:
        assert not ct2[at].any(), "the ciphertexts of a refused point are zero"
        assert (ct2[at + 1:at + 3] == ct[at + 1:at + 3]).all(), "the OTs behind a refused point are untouched by it"
    rest = np.ones(n, bool)
    rest[list(hostile)] = False
    assert (ct2[rest] == ct[rest]).all()


def test_short_coordinates(ctx):
    """S, T and b * A whose coordinates have leading zero bytes: deriveMask hashes x.Bytes() and y.Bytes(), not 32 bytes each"""
    a = co.SHORT_A_SCALAR
    A, AaInv = co.sender_setup(a)
    ks = sorted(co.SHORT_MULTIPLES)
    short = {k: co.mul(A, k) for k in ks}
    for k in ks:
        assert co.coord_lengths(short[k]) == co.SHORT_MULTIPLES[k]
    id0 = 1000
    # decrypt with b = k: the mask is that of k * A
    cts = [drbg("co/short/ct%d" % k, 32) for k in ks]
    choice = np.array([i & 1 for i in range(len(ks))], np.uint8)
    labels = engine.co_receiver_decrypt(ctx, co.point_bytes(A), ks, choice, np.frombuffer(b"".join(cts), np.uint8), id0)
    want = [masks_xor(short[k], id0 + i, cts[i][16:] if choice[i] else cts[i][:16]) for i, k in enumerate(ks)]
    assert label_raw(labels) == want
    # encrypt: B = k * G gives S = k * A;  B = k * G + A (the receiver's point for b = k with the choice set) gives
    # S = k * A + a * A and T = S + AaInv = k * A
    points = [co.mul(co.G, k) for k in ks] + [co.add(co.mul(co.G, k), A) for k in ks]
    pairs = [(drbg("co/short/l0/%d" % i, 16), drbg("co/short/l1/%d" % i, 16)) for i in range(len(points))]
    S = [short[k] for k in ks] + [co.mul(p, a) for p in points[len(ks):]]
    T = [co.add(s, AaInv) for s in S]
    assert T[len(ks):] == [short[k] for k in ks]
    ct = engine.co_sender_encrypt(ctx, a, co.point_bytes(AaInv), points_array(points), wires_of(pairs), id0)
    want = [masks_xor(S[i], id0 + i, pairs[i][0]) + masks_xor(T[i], id0 + i, pairs[i][1]) for i in range(len(points))]
    assert ct_bytes(ct) == want


HOSTILE = {
    "off_curve": (co.G[0], co.G[1] + 1),
    "x_equals_p": (co.P, co.SQRT_B),
    "infinity": co.INF,
}


@pytest.fixture(scope="module")
def hostile_base(pool):
    """65 good points of the pool's session with the accepted edge cases placed among them:
    20: (0, sqrt b);  40: B = A (T = infinity, ct1 = SHA-256 of the bare id);  50: B = -A (S = AaInv: T = 2 * AaInv)"""
    n = 65
    a, A, AaInv = pool["a"], pool["A"], pool["AaInv"]
    good = [i for i in range(POOL) if i not in pool["infinite"] and pool["B"][i] != A][:n]
    points = [pool["B"][i] for i in good]
    S = [pool["S"][i] for i in good]
    pairs = [pool["pairs"][i] for i in good]
    for at, p in ((20, (0, co.SQRT_B)), (40, A), (50, co.neg(A))):
        points[at], S[at] = p, co.mul(p, a)
    T = [co.add(s, AaInv) for s in S]
    assert T[40] == co.INF and S[50] == AaInv and T[50] == co.mul(AaInv, 2)
    return dict(n=n, points=points, S=S, T=T, pairs=pairs)


@pytest.mark.parametrize("case", ["none"] + sorted(HOSTILE) + ["mixed"])
def test_hostile_points(ctx, pool, hostile_base, case):
    hb = hostile_base
    n, id0 = hb["n"], 77
    points = list(hb["points"])
    if case == "mixed":
        bad_at = {3: "off_curve", 10: "x_equals_p", 30: "infinity", 64: "off_curve"}
    elif case == "none":
        bad_at = {}
    else:
        bad_at = {37: case}
    for at, kind in bad_at.items():
        points[at] = HOSTILE[kind]
        assert not co.valid_point(points[at])
    want = [bytes(32) if i in bad_at else
            masks_xor(hb["S"][i], id0 + i, hb["pairs"][i][0]) + masks_xor(hb["T"][i], id0 + i, hb["pairs"][i][1]) for i in range(n)]
    assert want[40][16:] == bytes(x ^ y for x, y in zip(hashlib.sha256((id0 + 40).to_bytes(8, "big")).digest(), hb["pairs"][40][1]))
    AaInv, wires, pts = co.point_bytes(pool["AaInv"]), wires_of(hb["pairs"]), points_array(points)
    # host form: GC_E_POINT and the lowest bad index, the ciphertexts all the same
    if bad_at:
        with pytest.raises(engine.CoPointError) as e:
            engine.co_sender_encrypt(ctx, pool["a"], AaInv, pts, wires, id0)
        assert e.value.code == engine.GC_E_POINT and e.value.bad_index == min(bad_at)
        assert "ot: point not on curve" in str(e.value)
        ct = e.value.ct
    else:
        ct = engine.co_sender_encrypt(ctx, pool["a"], AaInv, pts, wires, id0)
    assert ct_bytes(ct) == want
    # device form: the status block
    d_ct, d_status = ctx.empty((n, 32)).zero(0x5A), ctx.empty(2, np.uint64).zero(0x5A)
    engine.co_sender_encrypt_dev(ctx, pool["a"], AaInv, ctx.to_device(pts), ctx.to_device(wires), n, id0, d_ct, d_status)
    ctx.sync()
    status = d_status.numpy()
    assert int(status[0]) == len(bad_at) and int(status[1]) == (min(bad_at) if bad_at else (1 << 64) - 1)
    assert ct_bytes(d_ct.numpy()) == want


def test_go_pinned_rounds(ctx, sha_circ):
    """sha2pc's TestDeterministicTranscript with the device as ot.CO: the choice points hash to Go's `expRound2`, the
    ciphertexts are the bytes under `expRound3`, the decrypted labels are the evaluator's"""
    dc = engine.DeviceCircuit(ctx, sha_circ)
    seen = {}

    def garble(key, rnd):
        g = dc.garble(key, rnd, batch=1)
        io = g["io"][0]
        seen["in"] = io[:512].copy()
        return {"in": io[:512], "out": io[512:]}, g["slab"][0]

    t = gt.transcript(sha_circ, garble, "transcript")
    dc.close()
    want = gt.CASES["transcript"][1]
    assert (t["round1"], t["round2"], t["round3"]) == want
    session, bits = go_session()
    A, AaInv = engine.co_sender_setup(session["a"])
    assert bytes(A) == co.point_bytes(session["A"]) and bytes(AaInv) == co.point_bytes(session["AaInv"])
    choice = np.array(bits, np.uint8)
    pts = engine.co_receiver_choices(ctx, A, t["scalars"], choice)
    assert round2_hash(session, [co.point_from_bytes(bytes(p)) for p in pts]) == want[1]
    wires = np.ascontiguousarray(seen["in"][256:], dtype=WIRE)
    ct = engine.co_sender_encrypt(ctx, session["a"], AaInv, pts, wires)
    assert ct_bytes(ct) == t["ciphertexts"]
    r3 = t["round3_bytes"]
    assert r3[len(r3) - 32 * 256:] == b"".join(ct_bytes(ct))  # the tail of the payload that `expRound3` hashes
    labels = engine.co_receiver_decrypt(ctx, A, t["scalars"], choice, ct)
    assert (labels == pick(wires, choice)).all()


def test_base_ots_feed_iknp(ctx):
    """128 base OTs through the device-pointer calls; their outputs are the base of gc_iknp_receiver_create and the k0 of
    gc_iknp_sender_create as they are, and a 1 000-OT extension pairs up (as tests/test_gpu_ot.py)"""
    n = 128
    base = np.zeros(n, WIRE)
    base["l0"] = labels_from_bytes([drbg("co/iknp/l0/%d" % i, 16) for i in range(n)])
    base["l1"] = labels_from_bytes([drbg("co/iknp/l1/%d" % i, 16) for i in range(n)])
    delta = oracle.label_from_bytes(drbg("co/iknp/delta", 16))
    choice = np.array([oracle.label_bit(delta, i) for i in range(n)], np.uint8)
    a = int.from_bytes(drbg("co/iknp/a", 32), "big")
    A, AaInv = engine.co_sender_setup(a)
    d_sc = ctx.to_device(np.frombuffer(drbg("co/iknp/scalars", 32 * n), np.uint8).reshape(n, 32))
    d_ch, d_base = ctx.to_device(choice), ctx.to_device(base)
    d_pts, d_ct, d_k0, d_status = ctx.zeros((n, 64)), ctx.zeros((n, 32)), ctx.zeros((n, 16)), ctx.zeros(2, np.uint64)
    engine.co_receiver_choices_dev(ctx, A, d_sc, d_ch, n, d_pts)
    engine.co_sender_encrypt_dev(ctx, a, AaInv, d_pts, d_base, n, 0, d_ct, d_status)
    engine.co_receiver_decrypt_dev(ctx, A, d_sc, d_ch, d_ct, n, 0, d_k0)
    ctx.sync()
    assert int(d_status.numpy()[0]) == 0
    k0 = np.frombuffer(d_k0.numpy().tobytes(), LABEL)
    assert (k0 == pick(base, choice)).all()
    m = 1000
    b = (np.frombuffer(drbg("co/iknp/b", m), np.uint8) & 1).astype(np.uint8)
    rcv, snd = engine.IKNPReceiver(ctx, base), engine.IKNPSender(ctx, delta, k0)
    u, got = rcv.receive(b)
    sent = snd.send(u, m)
    x0 = sent["d0"] ^ np.where(b == 1, np.uint64(delta[0]), np.uint64(0))
    x1 = sent["d1"] ^ np.where(b == 1, np.uint64(delta[1]), np.uint64(0))
    assert (got["d0"] == x0).all() and (got["d1"] == x1).all()  # rcvd = sent ^ b * delta
    rcv.close(); snd.close()


def test_misuse(ctx, pool):
    L, p = engine.lib(), engine._p
    E_ARG, E_POINT, OK = engine.GC_E_ARG, engine.GC_E_POINT, engine.GC_OK
    n = 4
    a = engine._b32(pool["a"])
    A, AaInv = engine.co_point(pool["A"]), engine.co_point(pool["AaInv"])
    sc, ch = scalars_array(pool["scalars"][:n]), pool["choice"][:n].copy()
    pts, wires = points_array(pool["B"][:n]), pool["wires"][:n].copy()
    ct, out_pts, out_lab = np.zeros((n, 32), np.uint8), np.zeros((n, 64), np.uint8), np.zeros(n, LABEL)
    bad = C.c_size_t(99)
    good_enc = [ctx.h, p(a), p(AaInv), p(pts), p(wires), n, 0, p(ct), C.byref(bad)]
    for k in (0, 1, 2, 3, 4, 7):  # every pointer but bad_index, which may be NULL
        args = list(good_enc)
        args[k] = None
        assert L.gc_co_sender_encrypt(*args) == E_ARG, k
    args = list(good_enc)
    args[8] = None
    assert L.gc_co_sender_encrypt(*args) == OK and bad.value == 99
    good_ch = [ctx.h, p(A), p(sc), p(ch), n, p(out_pts)]
    for k in (0, 1, 2, 3, 5):
        args = list(good_ch)
        args[k] = None
        assert L.gc_co_receiver_choices(*args) == E_ARG, k
    good_dec = [ctx.h, p(A), p(sc), p(ch), p(ct), n, 0, p(out_lab)]
    for k in (0, 1, 2, 3, 4, 7):
        args = list(good_dec)
        args[k] = None
        assert L.gc_co_receiver_decrypt(*args) == E_ARG, k
    d = ctx.zeros(64 * n)
    vp = C.c_void_p
    assert L.gc_co_sender_encrypt_dev(ctx.h, p(a), p(AaInv), vp(d.ptr), vp(d.ptr), n, 0, vp(d.ptr), None) == E_ARG
    assert L.gc_co_sender_encrypt_dev(ctx.h, p(a), p(AaInv), None, vp(d.ptr), n, 0, vp(d.ptr), vp(d.ptr)) == E_ARG
    assert L.gc_co_receiver_choices_dev(ctx.h, p(A), vp(d.ptr), vp(d.ptr), n, None) == E_ARG
    assert L.gc_co_receiver_decrypt_dev(ctx.h, p(A), vp(d.ptr), None, vp(d.ptr), n, 0, vp(d.ptr)) == E_ARG
    # a = 0 mod N
    for zero in (0, co.N):
        z = engine._b32(zero)
        assert L.gc_co_sender_encrypt(ctx.h, p(z), p(AaInv), p(pts), p(wires), n, 0, p(ct), C.byref(bad)) == E_ARG
        assert L.gc_co_sender_encrypt_dev(ctx.h, p(z), p(AaInv), vp(d.ptr), vp(d.ptr), n, 0, vp(d.ptr), vp(d.ptr)) == E_ARG
        assert L.gc_co_sender_encrypt(ctx.h, p(z), p(AaInv), None, None, 0, 0, None, None) == E_ARG  # checked before n = 0 returns
        assert L.gc_co_sender_encrypt_dev(ctx.h, p(z), p(AaInv), None, None, 0, 0, None, None) == E_ARG
    # a bad A: off the curve, an encoding >= p, infinity
    for badA in (HOSTILE["off_curve"], HOSTILE["x_equals_p"], co.INF):
        q = engine.co_point(badA)
        assert L.gc_co_receiver_choices(ctx.h, p(q), p(sc), p(ch), n, p(out_pts)) == E_POINT
        assert L.gc_co_receiver_decrypt(ctx.h, p(q), p(sc), p(ch), p(ct), n, 0, p(out_lab)) == E_POINT
        assert L.gc_co_receiver_choices_dev(ctx.h, p(q), vp(d.ptr), vp(d.ptr), n, vp(d.ptr)) == E_POINT
        assert L.gc_co_receiver_decrypt_dev(ctx.h, p(q), vp(d.ptr), vp(d.ptr), vp(d.ptr), n, 0, vp(d.ptr)) == E_POINT
        assert L.gc_co_receiver_choices(ctx.h, p(q), None, None, 0, None) == E_POINT  # checked before n = 0 returns
        assert L.gc_co_receiver_decrypt(ctx.h, p(q), None, None, None, 0, 0, None) == E_POINT
        assert L.gc_co_receiver_choices_dev(ctx.h, p(q), None, None, 0, None) == E_POINT
        assert L.gc_co_receiver_decrypt_dev(ctx.h, p(q), None, None, None, 0, 0, None) == E_POINT
        # ... and behind the pointers and the count: a NULL or an n whose bytes do not fit is GC_E_ARG whatever A is
        assert L.gc_co_receiver_choices(ctx.h, p(q), None, p(ch), n, p(out_pts)) == E_ARG
        assert L.gc_co_receiver_decrypt_dev(ctx.h, p(q), vp(d.ptr), vp(d.ptr), None, n, 0, vp(d.ptr)) == E_ARG
        assert L.gc_co_receiver_decrypt(ctx.h, p(q), p(sc), p(ch), p(ct), (1 << 58) + 1, 0, p(out_lab)) == E_ARG
        assert L.gc_co_receiver_choices_dev(ctx.h, p(q), vp(d.ptr), vp(d.ptr), (1 << 58) + 1, vp(d.ptr)) == E_ARG
        assert L.gc_co_sender_encrypt(ctx.h, p(a), p(q), p(pts), p(wires), n, 0, p(ct), None) == E_ARG  # the caller's own constant
    # n = 0: GC_OK with no other pointer, nothing written
    out_pts[:], ct[:] = 0x77, 0x77
    assert L.gc_co_receiver_choices(ctx.h, p(A), None, None, 0, None) == OK
    assert L.gc_co_receiver_decrypt(ctx.h, p(A), None, None, None, 0, 5, None) == OK
    assert L.gc_co_sender_encrypt(ctx.h, p(a), p(AaInv), None, None, 0, 5, None, None) == OK
    assert L.gc_co_sender_encrypt_dev(ctx.h, p(a), p(AaInv), None, None, 0, 5, None, None) == OK
    assert L.gc_co_receiver_choices(ctx.h, p(A), p(sc), p(ch), 0, p(out_pts)) == OK and (out_pts == 0x77).all()
    assert L.gc_co_sender_encrypt(ctx.h, p(a), p(AaInv), p(pts), p(wires), 0, 0, p(ct), C.byref(bad)) == OK and (ct == 0x77).all()
    assert (d.numpy() == 0).all()
