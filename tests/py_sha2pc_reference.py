"""The four rounds and three encodings of the reference's sha2pc package restated on Python integers for a general 2-party
circuit — TEST INFRASTRUCTURE, the reference of tests/test_gpu_sha2pc.py, tests/test_gpu_sha2pc_hostile.py and
tests/test_py_sha2pc_reference.py.

Restated from sha2pc/garbler.go:37-136 (GarblerRound1, GarblerRound3), evaluator.go:27-113 (EvaluatorRound2,
EvaluatorRound4), encoding.go (EncodeRound1 :35, DecodeRound1 :52, EncodeRound2 :84, DecodeRound2 :103, EncodeRound3 :149,
DecodeRound3 :177, encodePoints :481, decodePoints :505, packPointSigns :546) with the constants 256 / 256 / 256 / 42 914 of
params.go replaced by (ng, ne, nout, rows).  P-256, deriveMask and the label bytes are those of tests/go_transcript.py and
tests/py_co_reference.py, which the Go tests' round hashes pin; at sha256xor's numbers the functions here reproduce those
hashes (tests/test_py_sha2pc_reference.py).

Every function works on ONE session and returns its outputs and a verdict: 0, or code | index << 8 for the first check the
reference would fail, in the reference's order.  A bad session's outputs are zero bytes of the right lengths, which is
what the engine writes for it (the reference returns an error and nothing)."""
from collections import namedtuple

import numpy as np

from tests import go_transcript as gt
from tests import py_co_reference as co

MAGIC, CURVE, SESSION, SETUP, POINT, LABEL = 1, 2, 3, 4, 5, 6
P, N, B = gt.P, gt.N, gt.B
CHUNK = gt.CURVE_CHUNK

Geometry = namedtuple("Geometry", "ng ne nout rows")


def len1(g):
    return 16 + 64


def len2(g):
    return 16 + 32 * g.ne + (g.ne + 7) // 8


def len3(g):
    return 42 + 16 * g.rows + 16 * g.ng + 32 * g.nout + 32 * g.ne


def digest_bytes(g):
    return (g.nout + 7) // 8


def verdict(code, index=0):
    return code | index << 8


def decompress(x, odd):
    """elliptic.UnmarshalCompressed of 0x02 / 0x03 || X: None when X >= p or x^3 - 3x + b is no square"""
    if x >= P:
        return None
    t = (x * x * x - 3 * x + B) % P
    y = pow(t, (P + 1) // 4, P)
    if y * y % P != t:
        return None
    if (y & 1) != odd:
        y = (-y) % P
    return (x, y)


def garbler_round1(g, a, sid):
    """a: 32 bytes (the scalar crand.Int drew; any value, taken mod N), sid: 8 bytes -> (r1, A, AaInv, verdict)"""
    k = int.from_bytes(a, "big")
    if k % N == 0:
        return bytes(len1(g)), bytes(64), bytes(64), verdict(SETUP)
    A, ainv = co.sender_setup(k)
    A, ainv = co.point_bytes(A), co.point_bytes(ainv)
    return b"R1" + sid + CHUNK + A, A, ainv, 0


def evaluator_round2(g, r1, scalars, bits):
    """DecodeRound1 + EvaluatorRound2 + EncodeRound2 -> (r2, A, sid, verdict); scalars: ne x 32 bytes, bits: ne"""
    bad = lambda code: (bytes(len2(g)), bytes(64), bytes(8), verdict(code))
    assert len(r1) == len1(g)
    if r1[:2] != b"R1":
        return bad(MAGIC)
    if r1[10:16] != CHUNK:
        return bad(CURVE)
    sid, A = r1[2:10], co.point_from_bytes(r1[16:80])
    if not co.valid_point(A):
        return bad(SETUP)
    pts = co.receiver_choices(A, [int.from_bytes(s, "big") for s in scalars], bits)
    signs = bytearray((g.ne + 7) // 8)
    for i, pt in enumerate(pts):
        if pt[1] & 1:
            signs[i // 8] |= 1 << (i % 8)
    r2 = b"R2" + sid + CHUNK + b"".join(pt[0].to_bytes(32, "big") for pt in pts) + bytes(signs)
    return r2, r1[16:80], sid, 0


def decode_round2(g, r2):
    """DecodeRound2 -> (sid, points, verdict)"""
    assert len(r2) == len2(g)
    if r2[:2] != b"R2":
        return None, None, verdict(MAGIC)
    if r2[10:16] != CHUNK:
        return None, None, verdict(CURVE)
    signs = r2[16 + 32 * g.ne:]
    pts = []
    for i in range(g.ne):
        pt = decompress(int.from_bytes(r2[16 + 32 * i:48 + 32 * i], "big"), (signs[i // 8] >> (i % 8)) & 1)
        if pt is None:
            return None, None, verdict(POINT, i)
        pts.append(pt)
    return r2[2:10], pts, 0


def garbler_round3(g, a, AaInv, sid, r2, key, rnd, bits, garble):
    """DecodeRound2 + GarblerRound3 + EncodeRound3 -> (r3, verdict).  garble(key, rnd) -> (input wires WIRE [ng + ne],
    output wires WIRE [nout], slab LABEL [rows]); bits: ng"""
    bad = lambda v: (bytes(len3(g)), v)
    got, pts, v = decode_round2(g, r2)
    if v:
        return bad(v)
    if got != sid:
        return bad(verdict(SESSION))
    k, ainv = int.from_bytes(a, "big") % N, co.point_from_bytes(AaInv)
    if k == 0 or not co.valid_point(ainv):
        return bad(verdict(SETUP))
    win, wout, slab = garble(key, rnd)
    assert len(win) == g.ng + g.ne and len(wout) == g.nout and len(slab) == g.rows
    lb = gt.label_bytes
    ginputs = b"".join(lb(win[i]["l1" if bits[i] else "l0"]) for i in range(g.ng))
    hints = b"".join(lb(w["l0"]) + lb(w["l1"]) for w in wout)
    cts, none_bad = co.sender_encrypt(k, ainv, pts, [(lb(w["l0"]), lb(w["l1"])) for w in win[g.ng:]])
    assert not none_bad
    r3 = b"R3" + sid + key + lb(slab) + ginputs + hints + b"".join(cts)
    assert len(r3) == len3(g)
    return r3, 0


def labels_from_bytes(raw):
    be = np.frombuffer(raw, ">u8").reshape(-1, 2)
    out = np.zeros(len(be), np.dtype([("d0", "<u8"), ("d1", "<u8")]))
    out["d0"], out["d1"] = be[:, 0], be[:, 1]
    return out


def evaluator_round4(g, A, sid, scalars, bits, r3, evaluate):
    """DecodeRound3 + EvaluatorRound4 -> (digest, verdict).  evaluate(key, slab LABEL [rows], inputs LABEL [ng + ne]) ->
    output labels LABEL [nout]"""
    bad = lambda v: (bytes(digest_bytes(g)), v)
    assert len(r3) == len3(g)
    if r3[:2] != b"R3":
        return bad(verdict(MAGIC))
    if r3[2:10] != sid:
        return bad(verdict(SESSION))
    Apt = co.point_from_bytes(A)
    if not co.valid_point(Apt):
        return bad(verdict(SETUP))
    key, off = r3[10:42], 42
    slab = labels_from_bytes(r3[off:off + 16 * g.rows])
    off += 16 * g.rows
    inputs = np.zeros(g.ng + g.ne, slab.dtype)
    inputs[:g.ng] = labels_from_bytes(r3[off:off + 16 * g.ng])
    off += 16 * g.ng
    hints = r3[off:off + 32 * g.nout]
    off += 32 * g.nout
    cts = [r3[off + 32 * i:off + 32 * i + 32] for i in range(g.ne)]
    got = co.receiver_decrypt(Apt, [int.from_bytes(s, "big") for s in scalars], bits, cts)
    inputs[g.ng:] = labels_from_bytes(b"".join(got))
    out = gt.label_bytes(evaluate(key, slab, inputs))
    digest = bytearray(digest_bytes(g))
    for j in range(g.nout):  # BitFromLabel: L0 is asked first
        l, l0, l1 = out[16 * j:16 * j + 16], hints[32 * j:32 * j + 16], hints[32 * j + 16:32 * j + 32]
        if l == l0:
            continue
        if l != l1:
            return bad(verdict(LABEL, j))
        digest[j // 8] |= 1 << (j % 8)
    return bytes(digest), 0
