"""Self-test of the plain-Python GMW restatement (tests/py_gmw_reference.py): the parties' output shares XOR to the plaintext
result, and the triples of tripleBatch's arithmetic are Beaver triples.  Needs neither the engine nor a GPU."""
import numpy as np
import pytest

from tests import py_gmw_reference as R


def _check_online(c, P, n, seed, plain):
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, (n, c.num_inputs)).astype(np.uint8)
    shares = R.share_inputs(rng, c, bits, P)
    _, _, tw = R.triple_words(c)
    msgs, outs = R.run_parties(c, shares, R.beaver_triples(rng, P, tw, n))
    ob = R.unpack(np.bitwise_xor.reduce(np.stack(outs), axis=0), c.num_outputs)
    for i in range(n):
        assert (ob[:, i] == plain(bits[i])).all()
    ands, _ = R.buckets(c)
    assert [lv for lv, _ in msgs[0]] == [i for i, a in enumerate(ands) if a]  # a level without ANDs sends nothing


@pytest.mark.parametrize("P", [2, 3])
def test_restatement_computes_the_circuit(aes_circ, add64_circ, P):
    for c in (aes_circ, add64_circ):
        _check_online(c, P, 5, 1 + P, lambda b, c=c: c.compute_bits(b)[c.NumWires - c.num_outputs:])


@pytest.mark.parametrize("P", [2, 3])
def test_restatement_fuzz_with_wire_reuse(P):
    rng = np.random.default_rng(100 + P)
    for k in range(12):
        reuse = [0.0, 0.1, 0.3][k % 3]
        c = R.fuzz_circuit(rng, int(rng.integers(3, 90)), int(rng.integers(1, 400)), reuse, nargs=3)
        # the reference evaluates in the bucketed order; without reuse that is circuit order
        _check_online(c, P, 4, k, lambda b, c=c: R.plain_bucketed(c, b))
        if reuse == 0.0:
            _check_online(c, P, 4, k, lambda b, c=c: c.compute_bits(b)[c.NumWires - c.num_outputs:])


def test_bucketed_order_differs_from_circuit_order_with_reuse():
    """w2 = w0 & w1 (level 0 -> w2 at level 1); w3 = w2 ^ w0 (level 1); w2 = w0 ^ w1 (level 0): the reference runs the XOR
    of level 0 first, then the AND, so w3 reads the AND's value; circuit order reads the same here, but the final w2 is
    the AND in bucketed order and the XOR in circuit order"""
    from mpc_amd.circuit import AND, GATE, XOR, Circuit
    g = np.zeros(3, GATE)
    g[0] = (0, 1, 2, AND, 0)
    g[1] = (2, 0, 3, XOR, 0)
    g[2] = (0, 1, 2, XOR, 0)
    c = Circuit(4, [1, 1], [2], g)
    for a in (0, 1):
        for b in (0, 1):
            assert R.plain_bucketed(c, [a, b]).tolist() == [a & b, (a & b) ^ a]
            assert c.compute_bits([a, b])[2:].tolist() == [a ^ b, (a & b) ^ a]
    _check_online(c, 2, 8, 3, lambda bits: R.plain_bucketed(c, bits))


def test_levels_of_the_shipped_circuits(aes_circ, add64_circ):
    for c, (nl, nand, tw) in ((aes_circ, (61, 60, 130)), (add64_circ, (64, 63, 63))):
        ands, _ = R.buckets(c)
        assert (len(ands), sum(1 for a in ands if a), R.triple_words(c)[2]) == (nl, nand, tw)


@pytest.mark.parametrize("P", [2, 3])
def test_triple_batch_gives_beaver_triples(P):
    rng = np.random.default_rng(7 + P)
    words = 64
    a = [rng.integers(0, 2 ** 62, words, dtype=np.int64).astype(np.uint64) * np.uint64(3) for _ in range(P)]
    b = [rng.integers(0, 2 ** 62, words, dtype=np.int64).astype(np.uint64) * np.uint64(5) for _ in range(P)]
    cot = R.ideal_cot(rng, b, P, words)
    c, sent = R.triple_batch(a, b, cot)
    xa = np.bitwise_xor.reduce(np.stack(a), axis=0)
    xb = np.bitwise_xor.reduce(np.stack(b), axis=0)
    xc = np.bitwise_xor.reduce(np.stack(c), axis=0)
    assert (xc == (xa & xb)).all()
    for (s, r), (u, v) in sent.items():
        d = np.uint64(0xFFFFFFFFFFFFFFFF) if cot[(s, r)][0] else np.uint64(0)
        assert (u == (a[s] ^ d)).all() and (v == b[r]).all()
