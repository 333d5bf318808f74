"""A plain-Python restatement of the reference's packed-IKNP VOLE, written from the Go text alone — vole/vole.go,
vole/prg.go — on the project's own Python AES (tests/py_reference.AES, FIPS-197 checked) and Python IKNP
(tests/py_ot_reference).  Test infrastructure (tests/test_py_vole_reference.py, tests/test_gpu_vole.py): integers and byte
strings, slow on purpose."""
from tests import py_ot_reference as ot
from tests.py_reference import AES, label_bytes

# P-256's field prime (vole_test.go:18-22)
P256 = int("ffffffff00000001000000000000000000000000ffffffffffffffffffffffff", 16)


def prg_expand_label(key):
    """prgExpandLabel (prg.go:16-27): AES-128-CTR under `key` (16 bytes), zero IV, over 32 zero bytes — the key stream of
    counter blocks 0 and 1 (crypto/cipher.NewCTR: the IV is one big-endian 128-bit counter)"""
    a = AES(bytes(key))
    return a.encrypt((0).to_bytes(16, "big")) + a.encrypt((1).to_bytes(16, "big"))


def label_pad(label):
    """pad of one IKNP label: prgExpandLabel(GetData(label)) (vole.go:63-68; GetData = BE64(D0) || BE64(D1), label.go:105-108)"""
    return prg_expand_label(label_bytes(label))


def bytes32(v):
    """bytes32 (vole.go:219-227): v.Bytes() — the big-endian bytes of |v| — right-aligned in 32 bytes.  A value of more
    than 32 bytes makes Go's copy(out[32-len(b):], b) index below zero: a run-time panic (raised here as ValueError)."""
    if v is None:
        return bytes(32)
    b = abs(v).to_bytes((abs(v).bit_length() + 7) // 8, "big")
    if len(b) > 32:
        raise ValueError("panic: slice bounds out of range [%d:]" % (32 - len(b)))
    return bytes(32 - len(b)) + b


def sender_mul(pads, xs, y_msg, p):
    """the per-label work of (*Sender).Mul (vole.go:58-107) from the labels' pads: (rs, u_msg)"""
    m = len(xs)
    assert len(pads) == m
    rs = [int.from_bytes(pad, "big") % p for pad in pads]  # SetBytes, Mod (vole.go:70-73)
    if len(y_msg) != m * 32:
        raise ValueError("vole: MulSender expected %d bytes for y-vector, got %d" % (m * 32, len(y_msg)))
    ys = [int.from_bytes(y_msg[32 * i:32 * i + 32], "big") % p for i in range(m)]
    out = b""
    for i in range(m):  # Mul, Mod, Add, Mod (vole.go:89-96); big.Int.Mod is Euclidean, as Python's %
        tmp = (xs[i] * ys[i]) % p
        out += bytes32((rs[i] + tmp) % p)
    return rs, out


def receiver_reduce(u_msg, m, p):
    """the tail of (*Receiver).Mul (vole.go:177-188): us_i = BE256(u_msg_i) mod p"""
    if len(u_msg) != m * 32:
        raise ValueError("vole: MulReceiver expected %d bytes for u-vector, got %d" % (m * 32, len(u_msg)))
    return [int.from_bytes(u_msg[32 * i:32 * i + 32], "big") % p for i in range(m)]


def mul(xs, ys, p, base_wires, delta, k0):
    """a whole Mul of both sides on the Python IKNP: the receiver runs iknp.Receive with all-false flags (vole.go:150-159),
    the sender iknp.Send(m, false) (vole.go:52); then the y- and u-messages.  base_wires / delta / k0: the base OTs'
    outcome (128 wires, the sender's Delta and the labels it received for Delta's bits)."""
    m = len(xs)
    assert len(ys) == m
    rcv, snd = ot.Receiver(base_wires), ot.Sender(delta, k0)
    u, labels_r = rcv.receive([False] * m)
    labels_s = snd.send(u, m)
    y_msg = b"".join(bytes32(y) for y in ys)  # the raw y, not reduced (vole.go:164-167)
    rs, u_msg = sender_mul([label_pad(l) for l in labels_s], xs, y_msg, p)
    us = receiver_reduce(u_msg, m, p)
    return {"u": u, "labels_r": labels_r, "labels_s": labels_s, "y_msg": y_msg, "rs": rs, "u_msg": u_msg, "us": us}
