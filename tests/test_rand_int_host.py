"""CPU check of crand.Int on the random streams (mpc_amd/csrc/rand_int.h), the arithmetic the engine's argument checks and the
kernel of gc_rand_scalars_cur* share: the header is compiled into a small stand-alone C++ program with the host compiler and
the address and undefined-behaviour sanitizers, and its walk is held against tests/go_transcript.py::crand_int (pinned by Go's
own transcript hashes) on 200 seeded cases over the moduli of the GPU test, and on synthetic streams that real AES cannot
supply: nothing but rejections (the walk must end bad at exactly the bound with nothing emitted), the last accepted candidate
on the last one the bound allows, and cursors at the edge of the range test."""
import os
import subprocess

import numpy as np
import pytest

from tests.go_transcript import crand_int

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpc_amd", "csrc")

P256_N = 0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551
# max -> (k, mask): the table of the GPU test
MODULI = {P256_N: (32, 0xff), (1 << 255) - 19: (32, 0x7f), (1 << 255) + 1: (32, 0xff), 1 << 128: (16, 0xff),
          (1 << 64) + 1: (9, 0x01), 257: (2, 0x01), 3: (1, 0x03), 2: (1, 0x01)}
FF64 = (1 << 64) - 1

PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "rand_int.h"

using namespace gc;

static std::vector<uint8_t> unhex(const std::string &h) {
    std::vector<uint8_t> b(h.size() / 2);
    for (size_t i = 0; i < b.size(); i++) b[i] = (uint8_t)std::stoul(h.substr(2 * i, 2), nullptr, 16);
    return b;
}

// "<stream bytes behind the cursor, hex, or -> <max, 64 hex digits> <count> <cursor>"
//   -> "noshape" | "<k> <mask> <cap> range" | "<k> <mask> <cap> bad <consumed> <emitted>"
//    | "<k> <mask> <cap> ok <consumed> <new cursor> <scalar, 64 hex digits> ..."
int main() {
    std::string hex, maxhex;
    uint64_t count, cursor;
    while (std::cin >> hex >> maxhex >> count >> cursor) {
        const std::vector<uint8_t> bytes = hex == "-" ? std::vector<uint8_t>() : unhex(hex), max = unhex(maxhex);
        if (max.size() != 32) return 1;
        RandIntShape sh;
        if (!rand_int_shape(max.data(), sh)) {
            std::printf("noshape\n");
            continue;
        }
        std::printf("%u %u %" PRIu64, sh.k, sh.mask, rand_int_cap(count));
        if (!rand_int_range_ok(sh, cursor, count)) {
            std::printf(" range\n");
            continue;
        }
        std::vector<std::string> scalars(count);
        size_t emitted = 0;
        bool past = false;
        uint64_t consumed = 0;
        const bool ok = rand_int_walk(
            sh, count,
            [&](uint64_t p) {
                if (p >= bytes.size()) {
                    past = true;
                    return (uint8_t)0;
                }
                return bytes[p];
            },
            [&](uint64_t i, const uint32_t(&v)[8]) {
                char buf[65];
                for (int l = 0; l < 8; l++) std::snprintf(buf + 8 * l, 9, "%08x", v[l]);
                scalars.at(i) = buf;
                emitted++;
            },
            consumed);
        if (past) return 2;  // the test gave too few bytes
        if (!ok) {
            std::printf(" bad %" PRIu64 " %zu\n", consumed, emitted);
            continue;
        }
        std::printf(" ok %" PRIu64 " %" PRIu64, consumed, cursor + consumed * sh.k);
        for (const std::string &s : scalars) std::printf(" %s", s.c_str());
        std::printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("rand_int")
    src, exe = d / "rand_int_host.cpp", d / "rand_int_host"
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def run(prog, cases):
    """cases: (bytes, max, count, cursor) -> one list of fields per case"""
    lines = ["%s %064x %d %d" % (b.hex() or "-", mx, count, cur) for b, mx, count, cur in cases]
    r = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-4000:])
    out = r.stdout.strip().split("\n")
    assert len(out) == len(cases)
    return [o.split() for o in out]


def cap(count):
    return 4 * count + 256


class BytesReader:
    def __init__(self, data):
        self.data, self.pos = data, 0

    def read(self, n):
        assert self.pos + n <= len(self.data)
        self.pos += n
        return self.data[self.pos - n: self.pos]


def test_shapes_and_the_moduli_without_one(prog):
    out = run(prog, [(b"", mx, 1, 0) for mx in (0, 1)] + [(bytes(32 * cap(1)), mx, 1, 0) for mx in MODULI])
    assert out[0] == out[1] == ["noshape"]
    for (mx, (k, mask)), f in zip(MODULI.items(), out[2:]):
        assert f[:4] == [str(k), str(mask), str(cap(1)), "ok"], (hex(mx), f)
        assert f[4:] == ["1", str(k), "0" * 64]  # zero bytes: the first candidate is 0 and is accepted


def test_against_crand_int(prog):
    rng = np.random.default_rng(2027)
    moduli = list(MODULI)
    cases, want = [], []
    rejected = {mx: 0 for mx in moduli}
    for i in range(200):
        mx = moduli[i % len(moduli)]
        k = MODULI[mx][0]
        count = int(rng.choice([1, 2, 5, 63, 64, 65, 130]))
        cursor = int(rng.integers(0, 1 << 62)) >> int(rng.integers(0, 62))
        data = rng.bytes(k * cap(count))
        reader = BytesReader(data)
        scalars = [crand_int(reader, mx) for _ in range(count)]
        assert reader.pos % k == 0 and reader.pos // k <= cap(count)
        rejected[mx] += reader.pos // k - count
        cases.append((data, mx, count, cursor))
        want.append(["ok", str(reader.pos // k), str(cursor + reader.pos)] + ["%064x" % v for v in scalars])
    for mx in ((1 << 255) + 1, (1 << 64) + 1, 257, 3):  # the cases do reject
        assert rejected[mx] > 0, hex(mx)
    for (data, mx, count, cursor), w, f in zip(cases, want, run(prog, cases)):
        assert f[:3] == [str(MODULI[mx][0]), str(MODULI[mx][1]), str(cap(count))]
        assert f[3:] == w, (hex(mx), count, cursor)


@pytest.mark.parametrize("count", [1, 5, 64, 65])
def test_nothing_but_rejections_ends_bad_at_the_bound(prog, count):
    mx = (1 << 255) + 1
    ones = b"\xff" * (32 * cap(count))
    (f,) = run(prog, [(ones, mx, count, 0)])
    assert f == ["32", "255", str(cap(count)), "bad", str(cap(count)), "0"]  # every candidate looked at, nothing emitted
    # count - 1 accepted candidates are not enough either, wherever they lie, and still nothing is emitted
    if count > 1:
        some = bytearray(ones)
        for j in range(count - 1):
            some[32 * 3 * j: 32 * 3 * j + 32] = bytes(32)
        (f,) = run(prog, [(bytes(some), mx, count, 0)])
        assert f[3:] == ["bad", str(cap(count)), "0"]


@pytest.mark.parametrize("count", [1, 5, 64, 65])
def test_the_last_accept_on_the_last_candidate_of_the_bound(prog, count):
    mx = (1 << 255) + 1
    stream = b"\xff" * (32 * (cap(count) - count)) + b"".join((j + 1).to_bytes(32, "big") for j in range(count))
    (f,) = run(prog, [(stream, mx, count, 7)])
    assert f[3:6] == ["ok", str(cap(count)), str(7 + 32 * cap(count))]
    assert f[6:] == ["%064x" % (j + 1) for j in range(count)]
    # accepted candidates spread out, the count-th still the last one: the walk must not stop a chunk early
    spread = bytearray(b"\xff" * (32 * cap(count)))
    at = sorted(set(range(0, 3 * (count - 1), 3)) | {cap(count) - 1})
    assert len(at) == count
    for j, c in enumerate(at):
        spread[32 * c: 32 * c + 32] = (j + 1).to_bytes(32, "big")
    (f,) = run(prog, [(bytes(spread), mx, count, 0)])
    assert f[3:5] == ["ok", str(cap(count))] and f[6:] == ["%064x" % (j + 1) for j in range(count)]


def test_the_range_test_of_a_cursor(prog):
    cases, want = [], []
    for mx, (k, _) in MODULI.items():
        for count in (1, 5):
            edge = FF64 - k * cap(count)
            cases += [(bytes(k * cap(count)), mx, count, edge), (bytes(k * cap(count)), mx, count, edge + 1)]
            want += [["ok", str(count), str(edge + count * k)], ["range"]]
    for f, w in zip(run(prog, cases), want):
        assert f[3:3 + len(w)] == w, (f, w)
    # a count whose bound times k does not fit 64 bits has no good cursor at all
    (f,) = run(prog, [(b"", P256_N, 1 << 58, 0)])
    assert f[3] == "range"
