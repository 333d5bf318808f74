"""The random streams of gc_rand_* restated from the Go sources, for the tests only.

A Go host that sets env.Config.Rand to cipher.StreamReader{S: cipher.NewCTR(aes.NewCipher(seed), iv), R: zeros} reads the
AES-CTR keystream: crypto/cipher/ctr.go encrypts the 16-byte counter, XORs the result into the (zero) source and then
increments the counter as a big-endian number, byte 15 first, the carry running up through byte 0 and falling off the end.
Successive Reads continue where the last one stopped, block boundaries or not.

`keystream` is that definition on the FIPS-197 AES class of tests/py_reference.py, one block at a time.  `Streams` is the same
for S (seed, iv) pairs at once with the rounds done on numpy arrays, because the GPU tests compare megabytes; the CPU tests
hold it against `keystream`, NIST SP 800-38A and OpenSSL.  The two draw orders served on top: circuit.Garbler's (garbler.go:
47-53: a 32-byte key, then garble.go:253,272: R and one label per input wire, 16 bytes each) and tripleBatch's (gmw/
triples.go:301-310: 16 bytes per triple word, a = BigEndian.Uint64(buf[0:8]), b = BigEndian.Uint64(buf[8:16]))."""
import numpy as np

from tests.py_reference import AES, SBOX, _gmul

MASK128 = (1 << 128) - 1


def ctr_add(iv, j):
    """the counter block after j increments of ctr.go: (iv + j) mod 2^128, big-endian"""
    return ((int.from_bytes(bytes(iv), "big") + j) & MASK128).to_bytes(16, "big")


def keystream(seed, iv, pos, n):
    """bytes [pos, pos + n) of the stream of (seed, iv), block by block on the AES class"""
    alg = AES(bytes(seed))
    iv = bytes(16) if iv is None else bytes(iv)
    first, last = pos // 16, (pos + n + 15) // 16
    blocks = b"".join(alg.encrypt(ctr_add(iv, j)) for j in range(first, last))
    return blocks[pos - 16 * first: pos - 16 * first + n]


class Reader:
    """the io.Reader of one session: successive read(n) continue the stream"""

    def __init__(self, seed, iv=None):
        self.seed, self.iv, self.pos = bytes(seed), iv, 0

    def read(self, n):
        out = keystream(self.seed, self.iv, self.pos, n)
        self.pos += n
        return out


# ---- the same rounds on arrays -------------------------------------------------------------------------------------------
_SB = np.array(SBOX, np.uint8)
_X2 = np.array([_gmul(x, 2) for x in range(256)], np.uint8)
_X3 = np.array([_gmul(x, 3) for x in range(256)], np.uint8)
_SHIFT = np.array([(4 * c + 5 * i) % 16 for c in range(4) for i in range(4)])  # ShiftRows on the column-major state
_ROT = [np.array([4 * c + (i + d) % 4 for c in range(4) for i in range(4)]) for d in range(4)]


def expand_keys(seeds):
    """u8 [S, keylen] -> round keys u8 [S, nr + 1, 16] (FIPS-197 5.2, every seed at once)"""
    seeds = np.ascontiguousarray(seeds, np.uint8)
    S, keylen = seeds.shape
    if keylen not in (16, 24, 32):
        raise ValueError("crypto/aes: invalid key size %d" % keylen)
    nk = keylen // 4
    nr = nk + 6
    w = np.zeros((S, 4 * (nr + 1), 4), np.uint8)
    w[:, :nk] = seeds.reshape(S, nk, 4)
    rcon = 1
    for i in range(nk, 4 * (nr + 1)):
        t = w[:, i - 1]
        if i % nk == 0:
            t = _SB[np.roll(t, -1, axis=1)]
            t[:, 0] ^= rcon
            rcon = _gmul(rcon, 2)
        elif nk > 6 and i % nk == 4:
            t = _SB[t]
        w[:, i] = w[:, i - nk] ^ t
    return w.reshape(S, nr + 1, 16)


def encrypt_blocks(rk, blocks):
    """rk u8 [S, nr + 1, 16], blocks u8 [S, B, 16] -> AES of every block under its row's key"""
    nr = rk.shape[1] - 1
    s = blocks ^ rk[:, None, 0]
    for r in range(1, nr + 1):
        s = _SB[s][..., _SHIFT]
        if r != nr:
            s = _X2[s] ^ _X3[s[..., _ROT[1]]] ^ s[..., _ROT[2]] ^ s[..., _ROT[3]]
        s = s ^ rk[:, None, r]
    return s


class Streams:
    """S sessions in lock step: one byte position, as the gc_rand handle keeps it"""

    def __init__(self, seeds, ivs=None):
        self.rk = expand_keys(seeds)
        self.S = len(self.rk)
        ivs = np.zeros((self.S, 16), np.uint8) if ivs is None else np.ascontiguousarray(ivs, np.uint8).reshape(self.S, 16)
        self.iv = [int.from_bytes(bytes(v), "big") for v in ivs]
        self.pos = 0

    def at(self, pos, n):
        """u8 [S, n]: bytes [pos, pos + n) of every stream"""
        first, last = pos // 16, (pos + n + 15) // 16
        ctr = b"".join(((iv + j) & MASK128).to_bytes(16, "big") for iv in self.iv for j in range(first, last))
        ctr = np.frombuffer(ctr, np.uint8).reshape(self.S, last - first, 16)
        ks = encrypt_blocks(self.rk, ctr).reshape(self.S, -1)
        return np.ascontiguousarray(ks[:, pos - 16 * first: pos - 16 * first + n])

    def read(self, n):
        out = self.at(self.pos, n)
        self.pos += n
        return out

    def seek(self, pos):
        self.pos = pos


def garbler_draw(stream, ninputs):
    """what circuit.Garbler takes from the head of a session's stream: (key [32], rnd [16 (1 + ninputs)])"""
    stream = bytes(stream)
    return stream[:32], stream[32: 32 + 16 * (1 + ninputs)]


def gmw_shares(buf):
    """tripleBatch's loop over 16-byte draws: (a, b) as lists of ints"""
    buf = bytes(buf)
    assert len(buf) % 16 == 0
    a = [int.from_bytes(buf[i: i + 8], "big") for i in range(0, len(buf), 16)]
    b = [int.from_bytes(buf[i + 8: i + 16], "big") for i in range(0, len(buf), 16)]
    return a, b
