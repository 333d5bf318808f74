"""The Chou-Orlandi base OT of the reference (ot/co_helpers.go) restated on Python integers — TEST INFRASTRUCTURE, the
reference of tests/test_gpu_co.py and tests/test_py_co_reference.py.  P-256, crypto/rand.Int and deriveMask are the ones of
tests/go_transcript.py, whose output the Go tests' round hashes pin.

Points are (x, y) integer pairs, (0, 0) the point at infinity (crypto/elliptic's encoding); labels and ciphertext halves are
16 bytes (ot.LabelData: BE(D0) || BE(D1)); scalars are integers below 2^256, taken mod N by the curve code."""
from tests import go_transcript as gt

P, N, B, G = gt.P, gt.N, gt.B, gt.G
INF = (0, 0)
SQRT_B = pow(B, (P + 1) // 4, P)  # (0, SQRT_B) is on the curve


def valid_point(pt):
    """curve.IsOnCurve (co_helpers.go:179-188): coordinates in [0, p) — an encoding >= p is refused, not reduced — and on
    the curve; (0, 0) is not"""
    x, y = pt
    return 0 <= x < P and 0 <= y < P and gt.on_curve(pt)


def add(p, q):
    """curve.Add: complete, with (0, 0) as the neutral element"""
    if p == INF:
        return q
    if q == INF:
        return p
    return gt.point_add(p, q)


def neg(p):
    return p if p == INF else (p[0], P - p[1])


def mul(pt, k):
    """curve.ScalarMult(x, y, k.Bytes())"""
    if pt == INF or k % N == 0:
        return INF
    return gt.scalar_mult(pt, k)


def coord_lengths(pt):
    """(len(x.Bytes()), len(y.Bytes())): what deriveMask hashes of each coordinate"""
    return tuple((v.bit_length() + 7) // 8 for v in pt)


def mask(pt, idx):
    return gt.derive_mask(pt, idx)[:16]


def _xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


def sender_setup(a):
    """GenerateCOSenderSetup (:77-101) for the scalar crand.Int drew -> (A, AaInv)"""
    if a % N == 0:
        raise ValueError("a = 0 mod N")
    A = mul(G, a)
    Aa = mul(A, a)
    return A, (Aa[0], P - Aa[1])


def sender_encrypt(a, AaInv, points, wires, id0=0):
    """EncryptCOCiphertexts (:104-137).  wires: [(l0, l1)] of 16 bytes each -> ([ct0 || ct1], indices of the bad points);
    the reference fails the whole call on the first bad point, the engine reports them and zeroes their ciphertexts"""
    cts, bad = [], []
    for i, (pt, (l0, l1)) in enumerate(zip(points, wires)):
        if not valid_point(pt):
            bad.append(i)
            cts.append(bytes(32))
            continue
        S = mul(pt, a)
        T = add(S, AaInv)
        cts.append(_xor(mask(S, id0 + i), l0) + _xor(mask(T, id0 + i), l1))
    return cts, bad


def receiver_choices(A, scalars, choices):
    """BuildCOChoices (:140-177) for the scalars crand.Int drew"""
    if not valid_point(A):
        raise ValueError("ot: point not on curve")
    return [add(mul(G, b), A) if c else mul(G, b) for b, c in zip(scalars, choices)]


def receiver_decrypt(A, scalars, choices, cts, id0=0):
    """DecryptCOCiphertexts (:191-219) -> [16 label bytes]"""
    out = []
    for i, (b, c, ct) in enumerate(zip(scalars, choices, cts)):
        out.append(_xor(mask(mul(A, b), id0 + i), ct[16:32] if c else ct[:16]))
    return out


def point_bytes(pt):
    """gc_p256_point: x and y as 32 big-endian bytes each; values of 2^256 and more do not exist at this boundary"""
    return pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big")


def point_from_bytes(b):
    return int.from_bytes(b[:32], "big"), int.from_bytes(b[32:64], "big")


# the session of the issue's short-coordinate cases: a = BE(01 02 .. 20) mod N, and the multiples k * A whose coordinates
# have leading zero bytes: k -> (len x, len y)
SHORT_A_SCALAR = int.from_bytes(bytes(range(1, 33)), "big") % N
SHORT_MULTIPLES = {180: (32, 31), 242: (31, 32), 22777: (31, 31), 26462: (30, 32), 40312: (32, 30)}
