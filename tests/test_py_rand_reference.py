"""The Python restatement of the random streams (tests/py_rand_reference.py), which the GPU tests of gc_rand_* take their
expected bytes from, reproduces NIST SP 800-38A's CTR vectors (F.5.1 / F.5.3 / F.5.5: the four blocks each, as plaintext XOR
keystream), agrees with OpenSSL's EVP_aes_{128,192,256}_ctr on seeded keys, IVs and positions, and its array form agrees
with its block-by-block form, carries and wrap-around included.  No GPU needed."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

from tests import py_rand_reference as rr
from tests.util import drbg

# NIST SP 800-38A, F.5: the counter block and the plaintext are shared by the three key sizes
CTR0 = bytes.fromhex("f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff")
PLAIN = bytes.fromhex("6bc1bee22e409f96e93d7e117393172a" "ae2d8a571e03ac9c9eb76fac45af8e51"
                      "30c81c46a35ce411e5fbc1191a0a52ef" "f69f2445df4f9b17ad2b417be66c3710")
NIST = {
    "F.5.1": ("2b7e151628aed2a6abf7158809cf4f3c",
              "874d6191b620e3261bef6864990db6ce" "9806f66b7970fdff8617187bb9fffdff"
              "5ae4df3edbd5d35e5b4f09020db03eab" "1e031dda2fbe03d1792170a0f3009cee"),
    "F.5.3": ("8e73b0f7da0e6452c810f32b809079e562f8ead2522c6b7b",
              "1abc932417521ca24f2b0459fe7e6e0b" "090339ec0aa6faefd5ccc2c6f4ce8e94"
              "1e36b26bd1ebc670d1bd1d665620abf7" "4f78a7f6d29809585a97daec58c6b050"),
    "F.5.5": ("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4",
              "601ec313775789a5b7a7f504bbf3d228" "f443e3ca4d62b59aca84e990cacaf5c5"
              "2b0930daa23de94ce87017ba2d84988d" "dfc9c58db67aada613c2dd08457941a6"),
}


def xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


def test_nist_sp800_38a_ctr_vectors():
    for name, (key, cipher) in NIST.items():
        key, cipher = bytes.fromhex(key), bytes.fromhex(cipher)
        assert xor(PLAIN, rr.keystream(key, CTR0, 0, 64)) == cipher, name
        assert xor(PLAIN, rr.Streams([list(key)], [list(CTR0)]).read(64)[0].tobytes()) == cipher, name
        # block by block through a reader, and the fourth block alone by position
        rd = rr.Reader(key, CTR0)
        assert b"".join(xor(PLAIN[i:i + 16], rd.read(16)) for i in range(0, 64, 16)) == cipher, name
        assert xor(PLAIN[48:], rr.keystream(key, CTR0, 48, 16)) == cipher[48:], name


def test_counter_addition_carries_and_wraps():
    assert rr.ctr_add(bytes(16), 1) == bytes(15) + b"\x01"
    assert rr.ctr_add(bytes(8) + b"\xff" * 8, 1) == bytes(7) + b"\x01" + bytes(8)
    assert rr.ctr_add(b"\xff" * 16, 1) == bytes(16)
    assert rr.ctr_add(b"\xff" * 16, 1 << 33) == ((1 << 33) - 1).to_bytes(16, "big")


def test_the_array_form_is_the_block_form():
    rng = np.random.default_rng(11)
    ivs = [bytes(rng.integers(0, 256, 16, dtype=np.uint8)), bytes(8) + b"\xff" * 7 + b"\xfe", b"\xff" * 16,
           bytes(12) + b"\xff" * 4]
    for keylen in (16, 24, 32):
        seeds = rng.integers(0, 256, (len(ivs), keylen), dtype=np.uint8)
        st = rr.Streams(seeds, [list(v) for v in ivs])
        for pos, n in ((0, 64), (5, 1), (15, 2), (8, 24), (31, 4112), ((1 << 36) + 3, 40)):
            got = st.at(pos, n)
            for s in range(len(ivs)):
                assert got[s].tobytes() == rr.keystream(seeds[s].tobytes(), ivs[s], pos, n), (keylen, s, pos, n)
    # successive reads continue the stream
    st = rr.Streams(seeds)
    parts = [st.read(n) for n in (8, 24, 1, 100, 31)]
    assert st.pos == 164 and (np.concatenate(parts, axis=1) == rr.Streams(seeds).at(0, 164)).all()
    assert (np.concatenate(parts, axis=1)[2].tobytes() == rr.keystream(seeds[2].tobytes(), None, 0, 164))


def test_the_draw_orders():
    buf = bytes(range(32)) + bytes(range(100, 148)) + b"rest"
    key, rnd = rr.garbler_draw(buf, 2)
    assert key == bytes(range(32)) and rnd == bytes(range(100, 148))
    a, b = rr.gmw_shares(bytes(range(32)))
    assert a == [0x0001020304050607, 0x1011121314151617] and b == [0x08090a0b0c0d0e0f, 0x18191a1b1c1d1e1f]


def _openssl():
    name = ctypes.util.find_library("crypto")
    if not name:
        return None
    try:
        lib = C.CDLL(name)
        lib.EVP_CIPHER_CTX_new.restype = C.c_void_p
        for f in ("EVP_aes_128_ctr", "EVP_aes_192_ctr", "EVP_aes_256_ctr"):
            getattr(lib, f).restype = C.c_void_p
        return lib
    except (OSError, AttributeError):
        return None


def test_against_openssl_ctr():
    lib = _openssl()
    if lib is None:
        pytest.skip("libcrypto not loadable")
    for i in range(24):
        klen = (16, 24, 32)[i % 3]
        key, iv = drbg("rk%d" % i, klen), drbg("ri%d" % i, 16)
        if i % 4 == 3:
            iv = iv[:8] + b"\xff" * 7 + b"\xfd"  # the carry crosses into the high half inside the read
        n = 16 * 9 + i
        ctx = C.c_void_p(lib.EVP_CIPHER_CTX_new())
        assert lib.EVP_EncryptInit_ex(ctx, C.c_void_p(getattr(lib, "EVP_aes_%d_ctr" % (8 * klen))()), None, key, iv) == 1
        out, m = C.create_string_buffer(n + 32), C.c_int(0)
        assert lib.EVP_EncryptUpdate(ctx, out, C.byref(m), bytes(n), n) == 1 and m.value == n
        lib.EVP_CIPHER_CTX_free(ctx)
        assert rr.keystream(key, iv, 0, n) == out.raw[:n], i
        assert rr.Streams([list(key)], [list(iv)]).at(3, n - 3)[0].tobytes() == out.raw[3:n], i
