"""What the sha2pc tests share — TEST INFRASTRUCTURE: the CPU oracle as Circuit.Garble / Circuit.Eval of the Python reference
(tests/py_sha2pc_reference.py), the random bytes of a session in the reference's consumption order (Go's deterministic runs
and seeded ones), the four reference rounds of a list of sessions, and the four engine rounds on device slots."""
import numpy as np

import oracle
from oracle import LABEL
from tests import go_transcript as gt
from tests import py_sha2pc_reference as ref
from tests.util import drbg

SHA256XOR = ref.Geometry(256, 256, 256, 42914)
FILL = 0xA5  # what the slots hold before a round writes them: the padding must still hold it afterwards


def small_circuit(ng, ne):
    """a 2-party circuit with AND, OR and INV gates and 11 outputs (not a multiple of 8)"""
    from mpc_amd.circuit import synthetic_levelised
    c = synthetic_levelised(4, 11, 0.3, 7, ninputs=ng + ne, or_frac=0.2, inv_frac=0.15)
    st = c.stats()
    assert st["AND"] and st["OR"] and st["INV"] and c.num_outputs == 11
    return c, ref.Geometry(ng, ne, c.num_outputs, c.slab_rows())


def oracle_garble(circ, g):
    def garble(key, rnd):
        o = oracle.garble(circ.Gates, circ.NumWires, circ.num_inputs, key, rnd)
        w = o["wires"]
        return w[:g.ng + g.ne], w[circ.NumWires - g.nout:], o["slab"]
    return garble


def oracle_evaluate(circ, g):
    def evaluate(key, slab, inputs):
        wires = np.zeros(circ.NumWires, LABEL)
        wires[:g.ng + g.ne] = inputs
        oracle.eval_(circ.Gates, circ.NumWires, key, wires, slab)
        return wires[circ.NumWires - g.nout:]
    return evaluate


def go_session(case, cooked=None):
    """the random bytes of one of Go's deterministic runs (tests/go_transcript.py: CASES), in the order the rounds consume
    them, and the two inputs of sha2pc_test.go:79-84"""
    cooked = cooked or gt.cooked_table()
    n1, n2, n3 = gt.CASES[case][0]
    r = gt.DeterministicReader(n1, cooked)
    a = gt.crand_int(r, gt.N).to_bytes(32, "big")
    sid = r.read(8)
    r = gt.DeterministicReader(n2, cooked)
    scalars = [gt.crand_int(r, gt.N).to_bytes(32, "big") for _ in range(256)]
    r = gt.DeterministicReader(n3, cooked)
    key = r.read(32)
    rnd = r.read(16 * 513)
    return {"a": a, "sid": sid, "scalars": scalars, "key": key, "rnd": rnd,
            "gbits": gt.bits_little(bytes(range(32))), "ebits": gt.bits_little(bytes(32 - i for i in range(32)))}


def seeded_session(g, seed):
    """any 32 bytes serve as a scalar (taken mod N)"""
    rnd = lambda what, n: drbg("sha2pc/%s/%s" % (seed, what), n)
    sc = rnd("scalars", 32 * g.ne)
    return {"a": rnd("a", 32), "sid": rnd("sid", 8), "scalars": [sc[32 * i:32 * i + 32] for i in range(g.ne)],
            "key": rnd("key", 32), "rnd": rnd("rnd", 16 * (1 + g.ng + g.ne)),
            "gbits": [b & 1 for b in rnd("gbits", g.ng)], "ebits": [b & 1 for b in rnd("ebits", g.ne)]}


def reference_rounds(g, s, garble, evaluate):
    r1, A, ainv, v1 = ref.garbler_round1(g, s["a"], s["sid"])
    r2, A2, sid2, v2 = ref.evaluator_round2(g, r1, s["scalars"], s["ebits"])
    r3, v3 = ref.garbler_round3(g, s["a"], ainv, s["sid"], r2, s["key"], s["rnd"], s["gbits"], garble)
    digest, v4 = ref.evaluator_round4(g, A2, sid2, s["scalars"], s["ebits"], r3, evaluate)
    return {"r1": r1, "r2": r2, "r3": r3, "digest": digest, "A": A, "AaInv": ainv, "verdicts": (v1, v2, v3, v4)}


def rows_of(sessions, what):
    """one field of every session as u8 [S, bytes]: bytes, a list of bits, or a list of 32-byte scalars"""
    flat = lambda v: b"".join(v) if isinstance(v, list) and isinstance(v[0], bytes) else bytes(v)
    return np.stack([np.frombuffer(flat(s[what]), np.uint8) for s in sessions])


class DeviceRounds:
    """the four _dev rounds of S sessions on device slots; every output comes back as a host array [S, ...] with the
    payloads cut out of their slots, and the slots' padding is checked to hold what it held"""

    def __init__(self, dc, g, S):
        from mpc_amd import engine
        self.engine, self.ctx, self.g, self.S = engine, dc.ctx, g, S
        self.gb = engine.Sha2pcGarbler(dc, g.ng, g.ne, S)
        self.ev = engine.Sha2pcEvaluator(dc, g.ng, g.ne, S)
        assert self.gb.len == [ref.len1(g), ref.len2(g), ref.len3(g)] and self.gb.lead == [0, 0, 6]
        assert self.ev.len == self.gb.len and self.ev.digest_bytes == ref.digest_bytes(g)
        self.len, self.lead, self.stride = self.gb.len, self.gb.lead, self.gb.stride
        z = lambda n: self.ctx.zeros(max(n, 16))
        self.d_slots = [z(S * st) for st in self.stride]
        self.d_v = z(4 * S)
        self.d_A, self.d_ainv, self.d_A2, self.d_sid2 = z(64 * S), z(64 * S), z(64 * S), z(8 * S)
        self.d_digest = z(S * ref.digest_bytes(g))

    def load(self, sessions):
        up = self.ctx.to_device
        self.d_a, self.d_sid = up(rows_of(sessions, "a")), up(rows_of(sessions, "sid"))
        self.d_scalars, self.d_ebits = up(rows_of(sessions, "scalars")), up(rows_of(sessions, "ebits"))
        self.d_keys, self.d_rnd = up(rows_of(sessions, "key")), up(rows_of(sessions, "rnd"))
        self.d_gbits = up(rows_of(sessions, "gbits")) if self.g.ng else self.ctx.zeros(16)

    def fill(self, k):
        self.d_slots[k].zero(FILL)

    def payloads(self, k):
        """[S, len] of round k + 1, and a check of the padding around them"""
        raw = self.d_slots[k].download(np.uint8, (self.S, self.stride[k]))
        lead, ln = self.lead[k], self.len[k]
        assert (raw[:, :lead] == FILL).all() and (raw[:, lead + ln:] == FILL).all(), "a round wrote a slot's padding"
        return raw[:, lead:lead + ln].copy()

    def set_payloads(self, k, rows):
        raw = np.full((self.S, self.stride[k]), FILL, np.uint8)
        raw[:, self.lead[k]:self.lead[k] + self.len[k]] = rows
        self.d_slots[k].upload(raw)

    def verdicts(self):
        return self.d_v.download(np.uint32, (self.S,))

    def round1(self):
        self.fill(0)
        self.gb.round1_dev(self.d_a, self.d_sid, self.d_A, self.d_ainv, self.d_slots[0], self.stride[0], self.d_v)
        return self.payloads(0), self.d_A.download(np.uint8, (self.S, 64)), self.d_ainv.download(np.uint8, (self.S, 64)), self.verdicts()

    def round2(self):
        self.fill(1)
        self.ev.round2_dev(self.d_slots[0], self.stride[0], self.d_scalars, self.d_ebits, self.d_A2, self.d_sid2,
                           self.d_slots[1], self.stride[1], self.d_v)
        return self.payloads(1), self.d_A2.download(np.uint8, (self.S, 64)), self.d_sid2.download(np.uint8, (self.S, 8)), self.verdicts()

    def round3(self):
        self.fill(2)
        self.gb.round3_dev(self.d_a, self.d_ainv, self.d_sid, self.d_slots[1], self.stride[1], self.d_keys, self.d_rnd,
                           self.d_gbits, self.d_slots[2], self.stride[2], self.d_v)
        return self.payloads(2), self.verdicts()

    def round4(self):
        self.d_digest.zero(FILL)
        self.ev.round4_dev(self.d_A2, self.d_sid2, self.d_scalars, self.d_ebits, self.d_slots[2], self.stride[2],
                           self.d_digest, self.d_v)
        return self.d_digest.download(np.uint8, (self.S, ref.digest_bytes(self.g))), self.verdicts()

    def run(self, sessions):
        self.load(sessions)
        r1, A, ainv, v1 = self.round1()
        r2, A2, sid2, v2 = self.round2()
        r3, v3 = self.round3()
        digest, v4 = self.round4()
        return {"r1": r1, "r2": r2, "r3": r3, "digest": digest, "A": A, "AaInv": ainv, "A2": A2, "sid2": sid2,
                "verdicts": np.stack([v1, v2, v3, v4], 1)}

    def close(self):
        self.gb.close()
        self.ev.close()


def assert_equal_to_reference(got, want, s):
    """session s of a DeviceRounds.run against reference_rounds of that session"""
    b = lambda a: bytes(np.asarray(a[s]).tobytes())
    assert tuple(int(v) for v in got["verdicts"][s]) == want["verdicts"], (s, got["verdicts"][s], want["verdicts"])
    for k in ("r1", "r2", "r3", "digest", "A", "AaInv"):
        if b(got[k]) != want[k]:
            g_, w_ = np.frombuffer(b(got[k]), np.uint8), np.frombuffer(want[k], np.uint8)
            first = int(np.flatnonzero(g_ != w_)[0]) if len(g_) == len(w_) else -1
            raise AssertionError("session %d: %s differs from the reference, first at byte %d of %d / %d" % (s, k, first, len(g_), len(w_)))
