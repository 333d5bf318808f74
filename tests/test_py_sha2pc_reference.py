"""tests/py_sha2pc_reference.py at sha256xor's numbers reproduces Go's own round hashes (tests/go_transcript.py: CASES,
EXP_FINAL), with the CPU oracle as Circuit.Garble / Circuit.Eval; and its verdicts on tampered payloads are the checks the
reference fails, in its order.  CPU only."""
import hashlib

import pytest

from tests import go_transcript as gt
from tests import py_sha2pc_reference as ref
from tests.sha2pc_cases import SHA256XOR, go_session, oracle_evaluate, oracle_garble, reference_rounds

G = SHA256XOR


@pytest.fixture(scope="module")
def transcript(sha_circ):
    s = go_session("transcript")
    return s, reference_rounds(G, s, oracle_garble(sha_circ, G), oracle_evaluate(sha_circ, G))


def test_lengths():
    assert (ref.len1(G), ref.len2(G), ref.len3(G), ref.digest_bytes(G)) == (80, 8240, gt.ROUND3_LEN, 32)
    g = ref.Geometry(3, 67, 11, 40)
    assert (ref.len2(g), ref.len3(g), ref.digest_bytes(g)) == (16 + 32 * 67 + 9, 42 + 640 + 48 + 352 + 2144, 2)


def test_reference_reproduces_gos_hashes(transcript):
    _, t = transcript
    h = lambda x: hashlib.sha256(x).hexdigest()
    assert t["verdicts"] == (0, 0, 0, 0)
    assert (h(t["r1"]), h(t["r2"]), h(t["r3"])) == gt.CASES["transcript"][1]
    assert t["digest"].hex() == gt.EXP_FINAL


def test_decompress():
    assert ref.decompress(gt.G[0], gt.G[1] & 1) == gt.G
    assert ref.decompress(gt.G[0], 1 - (gt.G[1] & 1)) == (gt.G[0], gt.P - gt.G[1])
    assert ref.decompress(gt.P, 0) is None and ref.decompress(2 ** 256 - 1, 0) is None
    assert ref.decompress(0, 0) is not None  # b is a square
    non = next(x for x in range(1, 50) if pow((x ** 3 - 3 * x + gt.B) % gt.P, (gt.P - 1) // 2, gt.P) != 1)
    assert ref.decompress(non, 0) is None


def test_verdicts_follow_the_references_order(transcript, sha_circ):
    s, t = transcript
    garble, evaluate = oracle_garble(sha_circ, G), oracle_evaluate(sha_circ, G)
    V = ref.verdict
    zero = bytes(32)
    assert ref.garbler_round1(G, zero, s["sid"]) == (bytes(80), bytes(64), bytes(64), V(ref.SETUP))
    assert ref.garbler_round1(G, gt.N.to_bytes(32, "big"), s["sid"])[3] == V(ref.SETUP)
    # round 2: magic before curve before A
    r1 = bytearray(t["r1"])
    r1[0] ^= 1
    r1[12] ^= 1
    r1[79] ^= 1
    assert ref.evaluator_round2(G, bytes(r1), s["scalars"], s["ebits"])[3] == V(ref.MAGIC)
    r1[0] ^= 1
    assert ref.evaluator_round2(G, bytes(r1), s["scalars"], s["ebits"])[3] == V(ref.CURVE)
    r1[12] ^= 1
    out = ref.evaluator_round2(G, bytes(r1), s["scalars"], s["ebits"])
    assert out == (bytes(8240), bytes(64), bytes(8), V(ref.SETUP))

    # round 3: magic, curve, point (lowest), sid, setup
    def r3(r2, a=s["a"], ainv=t["AaInv"], sid=s["sid"]):
        return ref.garbler_round3(G, a, ainv, sid, bytes(r2), s["key"], s["rnd"], s["gbits"], garble)[1]
    r2 = bytearray(t["r2"])
    r2[16 + 32 * 5:16 + 32 * 6] = gt.P.to_bytes(32, "big")
    r2[16 + 32 * 200:16 + 32 * 201] = (2 ** 256 - 1).to_bytes(32, "big")
    other = bytes(8)
    assert r3(r2, sid=other) == V(ref.POINT, 5)
    r2[1] = ord("3")
    r2[10] = 4
    assert r3(r2) == V(ref.MAGIC)
    r2[1] = ord("2")
    assert r3(r2) == V(ref.CURVE)
    r2 = bytearray(t["r2"])
    assert r3(r2, a=zero, sid=other) == V(ref.SESSION)
    assert r3(r2, a=zero) == V(ref.SETUP) and r3(r2, ainv=bytes(64)) == V(ref.SETUP)
    # a flipped sign bit is a valid point: the session stays good
    r2[16 + 32 * 256] ^= 1
    got, v = ref.garbler_round3(G, s["a"], t["AaInv"], s["sid"], bytes(r2), s["key"], s["rnd"], s["gbits"], garble)
    assert v == 0 and got[:-32 * 256] == t["r3"][:-32 * 256] and got[-32 * 256:-32 * 255] != t["r3"][-32 * 256:-32 * 255]
    assert got[-32 * 255:] == t["r3"][-32 * 255:]

    # round 4: magic, sid, A, label (lowest)
    def r4(r3b, A=t["A"], sid=s["sid"]):
        return ref.evaluator_round4(G, A, sid, s["scalars"], s["ebits"], bytes(r3b), evaluate)
    p3 = bytearray(t["r3"])
    hints = 42 + 16 * 42914 + 16 * 256
    p3[hints + 32 * 7] ^= 1       # L0 of output 7 (its label is one of the two)
    p3[hints + 32 * 7 + 16] ^= 1  # ... and L1
    p3[hints + 32 * 90] ^= 1
    p3[hints + 32 * 90 + 16] ^= 1
    assert r4(p3) == (bytes(32), V(ref.LABEL, 7))
    assert r4(p3, A=bytes(64))[1] == V(ref.SETUP)
    assert r4(p3, A=bytes(64), sid=other)[1] == V(ref.SESSION)
    p3[0] = 0
    assert r4(p3, A=bytes(64), sid=other)[1] == V(ref.MAGIC)
