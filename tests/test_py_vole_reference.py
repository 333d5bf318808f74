"""CPU checks of the plain-Python VOLE restatement (tests/py_vole_reference.py): the worked vector of the VOLE issue on both
AES implementations (the Python FIPS-197 AES and the C oracle's, portable and AES-NI), the pads of 256 seeded labels on
both, the reference's own test (TestVOLEBasic, vole_test.go:24-95) over the Python IKNP, and the property the packed
design rests on: with all-false choices the receiver's IKNP labels are the sender's (iknp.go:127-128)."""
import pytest

import oracle
from tests import py_vole_reference as vole
from tests.py_reference import label_bytes, label_from_bytes
from tests.util import drbg

P256 = vole.P256
KEY = bytes(range(16))
PAD = bytes.fromhex("c6a13b37878f5b826f4f8162a1c8d8797346139595c0b41e497bbde365f42d0a")
X = int.from_bytes(bytes(range(0x20, 0x40)), "big")
Y = (1 << 256) - 1
U = bytes.fromhex("8a63fcf8c3ce9dc79b7db194d5ff10b38f6331b4598273dbe5145375f580b691")


def oracle_pad(key, portable):
    return oracle.aes_encrypt(key, bytes(16), portable=portable) + oracle.aes_encrypt(key, bytes(15) + b"\x01",
                                                                                      portable=portable)


def test_worked_example():
    label = (0x0001020304050607, 0x08090a0b0c0d0e0f)
    assert label_bytes(label) == KEY
    assert vole.label_pad(label) == PAD
    for portable in (False, True):
        assert oracle_pad(KEY, portable) == PAD
    assert int.from_bytes(PAD, "big") < P256
    rs, u_msg = vole.sender_mul([PAD], [X], vole.bytes32(Y), P256)
    assert rs == [int.from_bytes(PAD, "big")]
    assert u_msg == U
    assert vole.receiver_reduce(u_msg, 1, P256) == [int.from_bytes(U, "big")]


@pytest.mark.parametrize("portable", [False, True])
def test_pads_match_the_oracle_aes(portable):
    raw = drbg("vole/pads", 16 * 256)
    for i in range(256):
        key = raw[16 * i:16 * i + 16]
        assert vole.prg_expand_label(key) == oracle_pad(key, portable), i


def test_bytes32_is_gos():
    assert vole.bytes32(None) == bytes(32)
    assert vole.bytes32(0) == bytes(32)
    assert vole.bytes32(1) == bytes(31) + b"\x01"
    assert vole.bytes32(-5) == bytes(31) + b"\x05"  # v.Bytes() is |v|
    assert vole.bytes32((1 << 256) - 1) == b"\xff" * 32
    with pytest.raises(ValueError):
        vole.bytes32(1 << 256)


def base_setup(seed):
    """128 seeded base-OT wires, a seeded Delta and the labels the sender's base OT delivers (k0[i] = wire i's l_{Delta_i})"""
    raw = drbg(seed, 128 * 32 + 16)
    base = [(label_from_bytes(raw[32 * i:32 * i + 16]), label_from_bytes(raw[32 * i + 16:32 * i + 32])) for i in range(128)]
    delta = label_from_bytes(raw[128 * 32:])
    k0 = [base[i][vole.ot.bit(delta, i)] for i in range(128)]
    return base, delta, k0


def field_elements(seed, m, p):
    """randomFieldElementFromCrypto (vole.go:207-216) on a seeded stream: 32 bytes, SetBytes, Mod p"""
    raw = drbg(seed, 32 * m)
    return [int.from_bytes(raw[32 * i:32 * i + 32], "big") % p for i in range(m)]


def test_vole_basic():
    """TestVOLEBasic (vole_test.go:24-95): m = 20, P-256, u_i - r_i == x_i * y_i mod p"""
    m = 20
    xs, ys = field_elements("vole/basic/x", m, P256), field_elements("vole/basic/y", m, P256)
    base, delta, k0 = base_setup("vole/basic")
    out = vole.mul(xs, ys, P256, base, delta, k0)
    assert len(out["rs"]) == m and len(out["us"]) == m
    for i in range(m):
        assert (out["us"][i] - out["rs"][i]) % P256 == xs[i] * ys[i] % P256, i


def test_receiver_labels_equal_the_senders():
    """all-false choices: the receiver's labels are the sender's (iknp.go:127-128), so the receiver could recompute every r"""
    base, delta, k0 = base_setup("vole/labels")
    out = vole.mul([1] * 9, [2] * 9, P256, base, delta, k0)
    assert out["labels_r"] == out["labels_s"]
