"""GPU parity of the device AES core alone (mpc_amd/csrc/aes_device.h: aes_encrypt_dual, the wide form, and
hash_col_whitened, the column-sliced form), through the entry that exposes the fixed-key hash most directly: one level of
independent AND gates.  Every table row and output label of such a circuit is an XOR of hashes H(x, j) = AES_k(K) ^ K with
K = 2x ^ j of the INPUT labels, which the caller sets (they are the random stream), so the AES input blocks are chosen here:
random ones, and blocks whose state after the first AddRoundKey — the bytes the first round's look-ups are addressed
with — is 0x00 or 0xff in every byte position (all sixteen at once, and one position at a time among random bytes), and the
same for the block before whitening.  Random 16-, 24- and 32-byte keys; a level small enough to run column-sliced as a whole,
the same level with one OR gate added (a unit with an OR gate stays in the wide form), and a level wide enough to run wide.
Compared byte for byte with the C oracle (oracle/aes_oracle.c, oracle/gc_oracle.c)."""
import numpy as np
import pytest

import oracle
from mpc_amd import engine
from mpc_amd.circuit import AND, GATE, LABEL, OR, Circuit, bitwise
from tests.util import drbg

pytestmark = pytest.mark.gpu

M128 = (1 << 128) - 1


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


def targets(seed):
    """(state, whitened?) pairs: the wanted 128-bit state, either after the first AddRoundKey or before it"""
    out = [(0, True), (M128, True), (0, False), (M128, False)]
    rnd = drbg(seed + "/targets", 16 * 32)
    for p in range(16):
        for i, v in enumerate((0x00, 0xff)):
            b = bytearray(rnd[16 * (2 * p + i):16 * (2 * p + i + 1)])
            b[p] = v
            out.append((int.from_bytes(b, "big"), True))
    return out


def crafted_rnd(c, key, seed, batch):
    """the random stream of `batch` instances; in instance 0 the zero labels of gate i's operands are set so that the block
    of H(a0, 2i) or of H(b0, 2i + 1) is target i (the one whose parity allows it: K = 2x ^ j has the low bit of j)"""
    nin = c.num_inputs
    bits = nin // 2
    assert (c.Gates["op"][:bits] == AND).all() and (c.Gates["in1"][:bits] == bits + np.arange(bits)).all()
    stride = 16 * (nin + 1)
    rnd = bytearray(drbg(seed, stride * batch))
    rk0 = int.from_bytes(key[:16], "big")
    tg = targets(seed)
    assert len(tg) <= bits
    hit = 0
    for i, (t, whitened) in enumerate(tg):
        for wire, j in ((i, 2 * i), (bits + i, 2 * i + 1)):
            k = t ^ (rk0 if whitened else 0)  # the block K wanted
            x = ((k ^ j) & M128) >> 1
            rnd[16 * (1 + wire):16 * (2 + wire)] = x.to_bytes(16, "big")
            got = ((x << 1) & M128) ^ j
            hit += got == k
            assert got | 1 == k | 1
    assert hit == len(tg)  # exactly one operand of every crafted gate meets its target in all 128 bits
    return bytes(rnd)


def check_level(ctx, c, key, seed, batch):
    nin, nout, nw = c.num_inputs, c.num_outputs, c.NumWires
    stride = 16 * (nin + 1)
    rnd = crafted_rnd(c, key, seed, batch)
    dc = engine.DeviceCircuit(ctx, c)
    b = engine.Batch(dc, batch)
    assert b.lds_wires, "expected the flat kernels with LDS-resident labels"
    b.close()
    g = dc.garble(key, rnd, batch=batch)  # without Garbled.Wires: the flat kernels
    bits = (np.frombuffer(drbg(seed + "/bits", batch * nin), np.uint8) & 1).reshape(batch, nin).astype(bool)
    bits[0] = False  # the evaluator of instance 0 holds the crafted zero labels
    inputs = np.where(bits, g["io"]["l1"][:, :nin], g["io"]["l0"][:, :nin])
    out = dc.eval(key, g["slab"], inputs=inputs, batch=batch)
    dc.close()
    for i in range(batch):
        ref = oracle.garble(c.Gates, nw, nin, key, rnd[i * stride:(i + 1) * stride])
        assert g["R"][i] == ref["R"]
        assert (g["slab"][i] == ref["slab"]).all(), "garbled tables of instance %d differ from the oracle" % i
        assert (g["io"][i][:nin] == ref["wires"][:nin]).all()
        assert (g["io"][i][nin:] == ref["wires"][nw - nout:]).all(), "output labels of instance %d" % i
        w = np.zeros(nw, LABEL)
        w[:nin] = inputs[i]
        oracle.eval_(c.Gates, nw, key, w, ref["slab"])
        assert (out[i] == w[nw - nout:]).all(), "evaluated labels of instance %d differ from the oracle" % i


def and_level(bits, with_or=False):
    """gate i = AND(a_i, b_i), hash indices 2i and 2i + 1; with_or: one OR gate more, after the ANDs"""
    c = bitwise(bits, AND)
    if not with_or:
        return c
    g = np.zeros(bits + 1, GATE)
    g[:bits] = c.Gates
    g[bits] = (0, bits, 3 * bits, OR, 0)
    return Circuit(3 * bits + 1, [bits, bits], [bits + 1], g, "and%d_or" % bits)


@pytest.mark.parametrize("keylen", [16, 24, 32])
@pytest.mark.parametrize("form", ["column", "wide-lone-wave", "wide"])
def test_fixed_key_hash_matches_oracle(ctx, keylen, form):
    """column: 40 ANDs of one instance = 160 hash lanes in the garbler, 80 in the evaluator (at most 256 and no OR gate: the
    unit runs column-sliced as a whole); wide-lone-wave: the same ANDs and one OR gate, which keeps the unit in the wide
    form; wide: 600 ANDs x 5 instances, the crafted gates in the first, full passes of the wide form"""
    for rep in range(2):
        seed = "aescore/%s/%d/%d" % (form, keylen, rep)
        key = drbg(seed + "/key", keylen)
        if form == "wide":
            check_level(ctx, and_level(600), key, seed, 5)
        else:
            check_level(ctx, and_level(40, with_or=(form == "wide-lone-wave")), key, seed, 1)
