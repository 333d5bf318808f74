"""What the gc_yao_* tests share — TEST INFRASTRUCTURE: the random bytes of a session, the reference messages of a list of
sessions (tests/py_yao_reference.py over the CPU oracle), and the six engine calls on device slots."""
import numpy as np

from oracle import LABEL
from tests import py_yao_reference as ref
from tests import sha2pc_cases
from tests.util import drbg

FILL = 0xA5  # what the slots hold before a call writes them: the padding must still hold it afterwards


def session(g, seed):
    rnd = lambda what, n: drbg("yao/%s/%s" % (seed, what), n)
    return {"key": rnd("key", g.keylen), "rnd": rnd("rnd", 16 * (1 + g.ng + g.ne)),
            "gbits": [b & 1 for b in rnd("gbits", g.ng)], "ebits": [b & 1 for b in rnd("ebits", g.ne)]}


def ot_labels(wires, ebits):
    """what any OT delivers: the label of the evaluator's bit, LABEL [ne]"""
    w = np.asarray(wires)
    return np.where(np.asarray(ebits, bool), w["l1"], w["l0"]).astype(LABEL)


def reference(circ, g, s):
    """one session through the restatement: every message, the bits both sides end with, the four verdicts"""
    rg = sha2pc_cases.ref.Geometry(g.ng, g.ne, g.nout, sum(g.rows))
    garble, evaluate = sha2pc_cases.oracle_garble(circ, rg), sha2pc_cases.oracle_evaluate(circ, rg)
    m1, gst = ref.garbler_send(g, s["key"], s["rnd"], s["gbits"], garble)
    est, v1 = ref.evaluator_accept(g, m1)
    m2, v2 = ref.evaluator_eval(g, est, v1, ot_labels(gst["ot_wires"], s["ebits"]), evaluate)
    m3, len3, bits, v3 = ref.garbler_result(g, gst, m2)
    ebits, v4 = ref.evaluator_result(g, m3 + bytes(ref.slot3(g) - len(m3)), ref.slot3(g))
    plain = circ.compute_bits(np.array(list(s["gbits"]) + list(s["ebits"]), np.uint8))[circ.NumWires - g.nout:]
    assert bits == np.packbits(plain, bitorder="little").tobytes() == ebits
    return {"m1": m1, "m2": m2, "m3": m3, "len3": len3, "bits": bits, "ot_wires": gst["ot_wires"], "verdicts": (v1, v2, v3, v4)}


def rows_of(sessions, what):
    return np.stack([np.frombuffer(bytes(s[what]), np.uint8) for s in sessions]) if len(bytes(sessions[0][what])) else \
        np.zeros((len(sessions), 0), np.uint8)


class DeviceYao:
    """the six _dev calls of S sessions on device slots; every output comes back as a host array with the messages cut out of
    their slots, and the slots' padding is checked to hold what it held"""

    def __init__(self, dc, g, S, extra_stride=0):
        from mpc_amd import engine
        self.engine, self.ctx, self.g, self.S = engine, dc.ctx, g, S
        self.gb = engine.YaoGarbler(dc, g.ng, g.ne, g.keylen, S)
        self.ev = engine.YaoEvaluator(dc, g.ng, g.ne, g.keylen, S)
        assert self.gb.len == self.ev.len == [ref.len1(g), ref.len2(g), ref.slot3(g)]
        self.len = self.gb.len
        self.stride = [st + extra_stride for st in self.gb.stride]
        z = lambda n: self.ctx.zeros(max(n, 16))
        self.d_slots = [z(S * st) for st in self.stride]
        self.d_v, self.d_len3 = z(4 * S), z(4 * S)
        self.d_gbits_out, self.d_ebits_out = z(S * ref.bits_bytes(g)), z(S * ref.bits_bytes(g))
        self.d_wires, self.d_labels = z(32 * S * g.ne), z(16 * S * g.ne)

    def load(self, sessions):
        up = self.ctx.to_device
        self.d_keys, self.d_rnd = up(rows_of(sessions, "key")), up(rows_of(sessions, "rnd"))
        self.d_gbits = up(rows_of(sessions, "gbits")) if self.g.ng else self.ctx.zeros(16)
        self.ebits = rows_of(sessions, "ebits")

    def slots(self, k, ln=None):
        """[S, len] of message k + 1 (ln: u32 [S] lengths, else the layout's), and a check of the padding behind them"""
        raw = self.d_slots[k].download(np.uint8, (self.S, self.stride[k]))
        if ln is None:
            assert (raw[:, self.len[k]:] == FILL).all(), "a call wrote a slot's padding"
            return raw[:, :self.len[k]].copy()
        for s in range(self.S):
            assert (raw[s, int(ln[s]):] == FILL).all(), "a call wrote behind session %d's message" % s
        return raw[:, :self.len[k]].copy()

    def set_slots(self, k, rows):
        raw = np.full((self.S, self.stride[k]), FILL, np.uint8)
        rows = np.asarray(rows)
        raw[:, :rows.shape[1]] = rows
        self.d_slots[k].upload(raw)

    def verdicts(self):
        return self.d_v.download(np.uint32, (self.S,))

    def send(self):
        self.d_slots[0].zero(FILL)
        self.gb.send_dev(self.d_keys, self.d_rnd, self.d_gbits, self.d_slots[0], self.stride[0])
        return self.slots(0)

    def plain_ot(self):
        """ot_wires_dev, then the OT in the clear on the host: the evaluator's labels go back to the device"""
        self.gb.ot_wires_dev(self.d_wires)
        wires = self.d_wires.download(self.engine.WIRE, (self.S, self.g.ne))
        self.d_labels.upload(np.stack([ot_labels(wires[s], self.ebits[s]) for s in range(self.S)]))
        return wires

    def accept(self):
        self.d_v.zero(FILL)
        self.ev.accept_dev(self.d_slots[0], self.stride[0], self.d_v)
        return self.verdicts()

    def eval(self):
        self.d_slots[1].zero(FILL)
        self.d_v.zero(FILL)
        self.ev.eval_dev(self.d_labels, self.d_slots[1], self.stride[1], self.d_v)
        return self.slots(1), self.verdicts()

    def garbler_result(self):
        for d in (self.d_slots[2], self.d_v, self.d_len3, self.d_gbits_out):
            d.zero(FILL)
        self.gb.result_dev(self.d_slots[1], self.stride[1], self.d_slots[2], self.stride[2], self.d_len3, self.d_gbits_out, self.d_v)
        len3, v = self.d_len3.download(np.uint32, (self.S,)), self.verdicts()
        # a bad session's message is zero over its slot bytes
        written = np.where(v != 0, self.len[2], len3)
        return self.slots(2, written), len3, self.d_gbits_out.download(np.uint8, (self.S, ref.bits_bytes(self.g))), v

    def evaluator_result(self):
        self.d_v.zero(FILL)
        self.d_ebits_out.zero(FILL)
        self.ev.result_dev(self.d_slots[2], self.stride[2], self.d_ebits_out, self.d_v)
        return self.d_ebits_out.download(np.uint8, (self.S, ref.bits_bytes(self.g))), self.verdicts()

    def run(self, sessions):
        self.load(sessions)
        m1 = self.send()
        wires = self.plain_ot()
        v1 = self.accept()
        m2, v2 = self.eval()
        m3, len3, gbits, v3 = self.garbler_result()
        ebits, v4 = self.evaluator_result()
        return {"m1": m1, "m2": m2, "m3": m3, "len3": len3, "bits": gbits, "ebits": ebits, "ot_wires": wires,
                "verdicts": np.stack([v1, v2, v3, v4], 1)}

    def close(self):
        self.gb.close()
        self.ev.close()


def assert_equal_to_reference(got, want, s):
    """session s of a DeviceYao.run against reference() of that session: every byte of every message, len3, the bits"""
    assert tuple(int(v) for v in got["verdicts"][s]) == want["verdicts"], (s, got["verdicts"][s], want["verdicts"])
    for k in ("m1", "m2"):
        g_, w_ = np.asarray(got[k][s]), np.frombuffer(want[k], np.uint8)
        if g_.tobytes() != want[k]:
            first = int(np.flatnonzero(g_ != w_)[0]) if len(g_) == len(w_) else -1
            raise AssertionError("session %d: %s differs from the reference, first at byte %d of %d / %d" % (s, k, first, len(g_), len(w_)))
    assert int(got["len3"][s]) == want["len3"] == len(want["m3"]), (s, got["len3"][s], want["len3"])
    assert got["m3"][s, :want["len3"]].tobytes() == want["m3"], "session %d: M3 differs" % s
    assert got["bits"][s].tobytes() == want["bits"] == got["ebits"][s].tobytes(), "session %d: bits differ" % s
    assert got["ot_wires"][s].tobytes() == np.asarray(want["ot_wires"]).astype(got["ot_wires"].dtype).tobytes(), "session %d: ot wires" % s
