"""Hostile peers of the gc_yao_* calls beyond three sessions: 1 027 sessions (a layout tile of four instances, a last session
tile of three) with pieces of 64 bytes, several bad sessions in one call — two in one session tile with different codes, one
on each side of a tile boundary, bad gates in several pieces of one session, bad sessions in the ragged last tile and in a
decode block with a dead wave — and the evaluator's and the results' calls replayed from captured graphs around a bad
message.  Exact verdict words from the Python restatement, zero outputs for every bad session, every other session
byte-identical to the clean run."""
import numpy as np
import pytest

from mpc_amd import engine
from tests import py_yao_reference as ref
from tests import sha2pc_cases
from tests import yao_cases as cases
from tests import yao_shape_cases as sc

pytestmark = pytest.mark.gpu

S, PIECE, KEYLEN = 1027, 64, 32


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


class Clean:
    """handles of the small circuit for S sessions, a clean run of them (compared with the reference, every session) and the
    evaluator's labels of that run"""

    def __init__(self, ctx, S, extra_stride):
        self.circ, self.g, self.S = sc.circuit("small")[0], sc.geometry("small", KEYLEN), S
        self.sessions = sc.sessions("small", KEYLEN, S)
        self.dc = engine.DeviceCircuit(ctx, self.circ)
        self.dy = cases.DeviceYao(self.dc, self.g, S, extra_stride=extra_stride)
        self.run = self.dy.run(self.sessions)
        assert not self.run["verdicts"].any()
        for s in range(S):
            cases.assert_equal_to_reference(self.run, sc.reference("small", KEYLEN, s), s)
        self.labels = np.stack([cases.ot_labels(self.run["ot_wires"][s], self.sessions[s]["ebits"]) for s in range(S)])

    def close(self):
        self.dy.close()
        self.dc.close()


@pytest.fixture(scope="module")
def clean(ctx):
    """created with GC_YAO_PIECE=64 (read at create alone), the default tile of 4"""
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("GC_YAO_TILE", raising=False)
        mp.setenv("GC_YAO_PIECE", str(PIECE))
        assert engine.yao_kernel_shape() == (sc.DEFAULT_SHAPE[0], PIECE)
        c = Clean(ctx, S, extra_stride=16)
    assert c.dy.gb.batch.tile_instances == c.dy.ev.batch.tile_instances == 4
    yield c
    c.close()


def spoil_word(m1, s, off):
    m1[s, off + 3] ^= 1


def others_unchanged(got, clean, bad):
    keep = np.ones(len(clean), bool)
    keep[list(bad)] = False
    same = (np.asarray(got)[keep] == np.asarray(clean)[keep]).reshape(int(keep.sum()), -1).all(1)
    assert same.all(), "sessions %s changed" % np.flatnonzero(keep)[~same][:8]


def test_m1_with_eight_bad_sessions_in_one_call(clean):
    c, dy, g = clean, clean.dy, clean.g
    goff, h = ref.gate_offsets(g), sc.hostile_gates(g, PIECE)
    lo, hi = h["pair"]
    at_gates = 4 + KEYLEN
    spoilt = {0: ([0], ref.verdict(ref.KEY)),
              3: ([at_gates], ref.verdict(ref.GATES)),
              4: ([goff[h["last"]]], ref.verdict(ref.ROWS, h["last"])),
              5: ([goff[hi], goff[lo]], ref.verdict(ref.ROWS, lo)),
              6: ([0, goff[7]], ref.verdict(ref.KEY)),
              1023: ([goff[0]], ref.verdict(ref.ROWS, 0)),
              1024: ([at_gates], ref.verdict(ref.GATES)),
              1026: ([goff[h["first_of_piece"]]], ref.verdict(ref.ROWS, h["first_of_piece"]))}
    m1 = c.run["m1"].copy()
    want = np.zeros(S, np.uint32)
    for s, (offs, v) in spoilt.items():
        for off in offs:
            spoil_word(m1, s, off)
        assert ref.evaluator_accept(g, m1[s].tobytes())[1] == v  # the expected words are the reference's
        want[s] = v
    bad = sorted(spoilt)
    dy.set_slots(0, m1)
    v1 = dy.accept()
    assert (v1 == want).all(), (np.flatnonzero(v1 != want)[:8], v1[bad], want[bad])
    dy.d_labels.upload(c.labels)
    m2, v2 = dy.eval()
    assert (v2 == want).all(), (np.flatnonzero(v2 != want)[:8], v2[bad], want[bad])
    assert not m2[bad].any()
    others_unchanged(m2, c.run["m2"], bad)
    # the host form: the lowest bad session and its code, the same verdicts
    with pytest.raises(engine.YaoSessionError) as e:
        dy.ev.accept(m1)
    assert (e.value.code, e.value.bad_session) == (engine.GC_E_ARG, 0) and (np.asarray(e.value.verdict) == want).all()
    # a clean message clears all of it
    dy.set_slots(0, c.run["m1"])
    assert not dy.accept().any()
    m2, v2 = dy.eval()
    assert not v2.any() and (m2 == c.run["m2"]).all()


def test_m2_with_flipped_labels_in_four_sessions(clean):
    c, dy, g = clean, clean.dy, clean.g
    nout, slot = g.nout, ref.slot3(g)
    flips = {1: [0], 2: [nout - 1], 1024: [5], 1026: [7, 3]}
    m2 = c.run["m2"].copy()
    want = np.zeros(S, np.uint32)
    rg = sha2pc_cases.ref.Geometry(g.ng, g.ne, g.nout, sum(g.rows))
    for s, outs in flips.items():
        for j in outs:
            m2[s, 16 * j + 9] ^= 0x10
        out_wires = sha2pc_cases.oracle_garble(c.circ, rg)(c.sessions[s]["key"], c.sessions[s]["rnd"])[1]
        want[s] = ref.garbler_result(g, {"out": out_wires}, m2[s].tobytes())[3]
        assert want[s] == ref.verdict(ref.LABEL, min(outs))
    bad = sorted(flips)
    dy.set_slots(1, m2)
    m3, len3, bits, v = dy.garbler_result()
    assert (v == want).all(), (np.flatnonzero(v != want)[:8], v[bad], want[bad])
    assert not m3[bad, :slot].any() and not len3[bad].any() and not bits[bad].any()
    others_unchanged(len3, c.run["len3"], bad)
    others_unchanged(bits, c.run["bits"], bad)
    for s in range(S):
        if s not in flips:
            assert (m3[s, :len3[s]] == c.run["m3"][s, :len3[s]]).all(), s


def test_m3_lengths_that_do_not_fit_in_the_first_and_the_last_session(clean):
    c, dy, g = clean, clean.dy, clean.g
    slot, stride = ref.slot3(g), dy.stride[2]
    m3 = np.zeros((S, slot), np.uint8)
    for s in range(S):
        m3[s, :c.run["len3"][s]] = c.run["m3"][s, :c.run["len3"][s]]
    bad = [0, 1026]
    want = np.zeros(S, np.uint32)
    for s in bad:
        m3[s, :4] = np.frombuffer(ref.be32(stride - 3), np.uint8)
        assert 4 + (stride - 3) > stride
        want[s] = ref.evaluator_result(g, m3[s].tobytes(), stride)[1]
        assert want[s] == ref.verdict(ref.LENGTH)
    dy.set_slots(2, m3)
    bits, v = dy.evaluator_result()
    assert (v == want).all(), (np.flatnonzero(v != want)[:8], v[bad])
    assert not bits[bad].any()
    others_unchanged(bits, c.run["bits"], bad)


def test_captured_accept_eval_and_results_around_a_bad_message(ctx, monkeypatch):
    """accept_dev + eval_dev in one graph, the two result calls in another, replayed over a clean M1, one with a wrong gate
    count in session 1, and the clean one again: accept's reset of its per-session minimum must be part of the graph"""
    monkeypatch.delenv("GC_YAO_TILE", raising=False)
    monkeypatch.delenv("GC_YAO_PIECE", raising=False)
    assert engine.yao_kernel_shape() == sc.DEFAULT_SHAPE
    n = 5
    c = Clean(ctx, n, extra_stride=0)
    dy, g, run = c.dy, c.g, c.run
    nb8 = ref.bits_bytes(g)
    d_v = [ctx.zeros(16 * n) for _ in range(4)]  # one verdict array per call
    filled = [dy.d_slots[1], dy.d_slots[2], dy.d_len3, dy.d_gbits_out, dy.d_ebits_out] + d_v

    def evaluator_side():
        dy.ev.accept_dev(dy.d_slots[0], dy.stride[0], d_v[0])
        dy.ev.eval_dev(dy.d_labels, dy.d_slots[1], dy.stride[1], d_v[1])

    def result_side():
        dy.gb.result_dev(dy.d_slots[1], dy.stride[1], dy.d_slots[2], dy.stride[2], dy.d_len3, dy.d_gbits_out, d_v[2])
        dy.ev.result_dev(dy.d_slots[2], dy.stride[2], dy.d_ebits_out, d_v[3])

    dy.set_slots(0, run["m1"])
    dy.d_labels.upload(c.labels)
    graphs = [ctx.capture(evaluator_side), ctx.capture(result_side)]

    def replay():
        for d in filled:
            d.zero(cases.FILL)
        for gr in graphs:
            gr.launch()
        v = np.stack([d.download(np.uint32, (n,)) for d in d_v], 1)
        len3 = dy.d_len3.download(np.uint32, (n,))
        return {"m2": dy.slots(1), "m3": dy.slots(2, np.where(v[:, 2] != 0, dy.len[2], len3)), "len3": len3, "verdicts": v,
                "bits": dy.d_gbits_out.download(np.uint8, (n, nb8)), "ebits": dy.d_ebits_out.download(np.uint8, (n, nb8))}

    def assert_clean(got):
        assert not got["verdicts"].any(), got["verdicts"]
        for k in ("m2", "len3", "bits", "ebits"):
            assert (got[k] == run[k]).all(), k
        for s in range(n):
            assert (got["m3"][s, :run["len3"][s]] == run["m3"][s, :run["len3"][s]]).all(), s

    try:
        assert_clean(replay())
        m1 = run["m1"].copy()
        spoil_word(m1, 1, 4 + KEYLEN)
        assert ref.evaluator_accept(g, m1[1].tobytes())[1] == ref.verdict(ref.GATES)
        dy.set_slots(0, m1)
        got = replay()
        want = [0, ref.verdict(ref.GATES), 0, 0, 0]
        assert list(got["verdicts"][:, 0]) == want and list(got["verdicts"][:, 1]) == want
        assert not got["m2"][1].any()
        others_unchanged(got["m2"], run["m2"], [1])
        # the garbler is handed 16 nout zero bytes for session 1: no label of its wires
        assert got["verdicts"][1, 2] & 0xff == ref.LABEL and got["len3"][1] == 0 and not got["bits"][1].any()
        others_unchanged(got["bits"], run["bits"], [1])
        dy.set_slots(0, run["m1"])
        assert_clean(replay())
    finally:
        for gr in graphs:
            gr.close()
        for d in d_v:
            d.close()
        c.close()
