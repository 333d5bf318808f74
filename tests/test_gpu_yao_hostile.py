"""Hostile peers of the gc_yao_* calls: three sessions, session 1 bad, sessions 0 and 2 byte-identical to the clean run.  The
exact verdict word, zero outputs for the bad session, and the host form's return code and bad_session — for a wrong key-length
word, a wrong gate count, wrong row words (gate 0, the last gate, the gate whose row word is the first word of a piece, two
gates at once), flipped bits in the labels of M2, and lengths of M3 that do not fit or fit with bits to drop.  Nothing here is
more than wrong bytes in well-sized buffers."""
import numpy as np
import pytest

from mpc_amd import engine
from mpc_amd.circuit import synthetic_levelised
from tests import py_yao_reference as ref
from tests import sha2pc_cases
from tests import yao_cases as cases

pytestmark = pytest.mark.gpu

S, BAD = 3, 1
_, PIECE = engine.yao_kernel_shape()


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


class Clean:
    """handles of one circuit, a clean run of three sessions, and the evaluator's labels of that run"""

    def __init__(self, ctx, circ, ng, ne, tag):
        self.circ, self.g = circ, ref.geometry(circ, ng, ne, 32)
        self.sessions = [cases.session(self.g, "hostile/%s/%d" % (tag, s)) for s in range(S)]
        self.dc = engine.DeviceCircuit(ctx, circ)
        self.dy = cases.DeviceYao(self.dc, self.g, S, extra_stride=16)
        self.run = self.dy.run(self.sessions)
        assert not self.run["verdicts"].any()
        self.labels = np.stack([cases.ot_labels(self.run["ot_wires"][s], self.sessions[s]["ebits"]) for s in range(S)])

    def close(self):
        self.dy.close()
        self.dc.close()


@pytest.fixture(scope="module")
def wide(ctx):
    """M1 of five pieces, gate 158's row word the first word of piece 1"""
    c = Clean(ctx, synthetic_levelised(8, 96, 0.5, 21, ninputs=14, or_frac=0.1, inv_frac=0.1), 5, 9, "wide")
    yield c
    c.close()


@pytest.fixture(scope="module")
def small(ctx):
    c = Clean(ctx, sha2pc_cases.small_circuit(3, 9)[0], 3, 9, "small")
    yield c
    c.close()


def others_unchanged(got, clean):
    for s in (0, 2):
        assert (np.asarray(got[s]) == np.asarray(clean[s])).all(), "session %d changed" % s


def check_bad_m1(c, m1, want, code):
    """accept and eval of a spoilt M1, device forms and host forms"""
    dy = c.dy
    dy.set_slots(0, m1)
    v = dy.accept()
    assert list(v) == [0, want, 0]
    dy.d_labels.upload(c.labels)
    m2, v2 = dy.eval()
    assert list(v2) == [0, want, 0] and not m2[BAD].any()
    others_unchanged(m2, c.run["m2"])
    with pytest.raises(engine.YaoSessionError) as e:
        dy.ev.accept(m1)
    assert (e.value.code, e.value.bad_session, list(e.value.verdict)) == (code, BAD, [0, want, 0])
    with pytest.raises(engine.YaoSessionError) as e:
        dy.ev.eval(c.labels)
    assert (e.value.code, e.value.bad_session, list(e.value.verdict)) == (code, BAD, [0, want, 0])
    assert not e.value.out[BAD].any()
    others_unchanged(e.value.out, c.run["m2"])
    # the next accept clears it
    dy.set_slots(0, c.run["m1"])
    assert not dy.accept().any()
    m2, v2 = dy.eval()
    assert not v2.any() and (m2 == c.run["m2"]).all()


def spoil_word(m1, off):
    m1 = m1.copy()
    m1[BAD, off + 3] ^= 1
    return m1


def test_m1_with_a_wrong_key_length_word(wide):
    check_bad_m1(wide, spoil_word(wide.run["m1"], 0), ref.verdict(ref.KEY), engine.GC_E_ARG)
    m1 = wide.run["m1"].copy()
    m1[BAD, :4] = np.frombuffer(ref.be32(16), np.uint8)  # a key length the reference would take: this handle serves 32
    check_bad_m1(wide, m1, ref.verdict(ref.KEY), engine.GC_E_ARG)


def test_m1_with_a_wrong_gate_count(wide):
    check_bad_m1(wide, spoil_word(wide.run["m1"], 4 + 32), ref.verdict(ref.GATES), engine.GC_E_ROWS)


def test_m1_with_wrong_row_words(wide):
    goff = ref.gate_offsets(wide.g)
    first_of_piece = [i for i, o in enumerate(goff) if o % PIECE == 0 and o]
    assert first_of_piece, "a gate's row word is the first word of a piece"
    last = len(goff) - 1
    for gate in (0, last, first_of_piece[0]):
        check_bad_m1(wide, spoil_word(wide.run["m1"], goff[gate]), ref.verdict(ref.ROWS, gate), engine.GC_E_ROWS)
        assert ref.evaluator_accept(wide.g, spoil_word(wide.run["m1"], goff[gate])[BAD].tobytes())[1] == ref.verdict(ref.ROWS, gate)
    # two bad gates in different pieces: the lowest is reported
    lo, hi = first_of_piece[0] - 1, last - 3
    assert goff[lo] // PIECE != goff[hi] // PIECE
    check_bad_m1(wide, spoil_word(spoil_word(wide.run["m1"], goff[hi]), goff[lo]), ref.verdict(ref.ROWS, lo), engine.GC_E_ROWS)
    # every check at once: the key word is asked first
    check_bad_m1(wide, spoil_word(spoil_word(wide.run["m1"], goff[0]), 0), ref.verdict(ref.KEY), engine.GC_E_ARG)


def check_bad_m2(c, m2, want):
    dy, nb8, slot = c.dy, ref.bits_bytes(c.g), ref.slot3(c.g)
    dy.set_slots(1, m2)
    m3, len3, bits, v = dy.garbler_result()
    assert list(v) == [0, want, 0]
    assert not m3[BAD, :slot].any() and len3[BAD] == 0 and not bits[BAD].any()
    for s in (0, 2):
        assert len3[s] == c.run["len3"][s] and (m3[s, :len3[s]] == c.run["m3"][s, :len3[s]]).all() and (bits[s] == c.run["bits"][s]).all()
    with pytest.raises(engine.YaoSessionError) as e:
        dy.gb.result(m2)
    assert (e.value.code, e.value.bad_session, list(e.value.verdict)) == (engine.GC_E_ARG, BAD, [0, want, 0])
    hm3, hlen3, hbits = e.value.out
    assert not hm3[BAD].any() and hlen3[BAD] == 0 and not hbits[BAD].any()
    for s in (0, 2):
        assert hlen3[s] == c.run["len3"][s] and (hm3[s, :hlen3[s]] == c.run["m3"][s, :hlen3[s]]).all() and (hbits[s] == c.run["bits"][s]).all()
    assert ref.garbler_result(c.g, {"out": sha2pc_cases.oracle_garble(c.circ, sha2pc_cases.ref.Geometry(c.g.ng, c.g.ne, c.g.nout, sum(c.g.rows)))(
        c.sessions[BAD]["key"], c.sessions[BAD]["rnd"])[1]}, m2[BAD].tobytes())[3] == want


@pytest.mark.parametrize("which", ["small", "wide"])
def test_m2_with_flipped_label_bits(which, small, wide):
    """nout = 11: one partial ballot; nout = 96: two ballots, the last label in the second"""
    c = small if which == "small" else wide
    nout = c.g.nout

    def flip(m2, j):
        m2[BAD, 16 * j + 9] ^= 0x10
        return m2

    check_bad_m2(c, flip(c.run["m2"].copy(), 0), ref.verdict(ref.LABEL, 0))
    check_bad_m2(c, flip(c.run["m2"].copy(), nout - 1), ref.verdict(ref.LABEL, nout - 1))
    check_bad_m2(c, flip(flip(c.run["m2"].copy(), nout - 1), 0), ref.verdict(ref.LABEL, 0))


def test_m3_lengths(small):
    c, dy = small, small.dy
    nb8, slot, stride = ref.bits_bytes(c.g), ref.slot3(c.g), small.dy.stride[2]
    clean = np.zeros((S, slot), np.uint8)
    for s in range(S):
        clean[s, :c.run["len3"][s]] = c.run["m3"][s, :c.run["len3"][s]]
    # n too long for the slot's stride (device form) and for the packed slot (host form)
    for n in (stride - 3, 0xffffffff):
        m3 = clean.copy()
        m3[BAD, :4] = np.frombuffer(ref.be32(n), np.uint8)
        dy.set_slots(2, m3)
        bits, v = dy.evaluator_result()
        assert list(v) == [0, ref.verdict(ref.LENGTH), 0] and not bits[BAD].any()
        others_unchanged(bits, c.run["bits"])
        with pytest.raises(engine.YaoSessionError) as e:
            dy.ev.result(m3)
        assert (e.value.code, e.value.bad_session, list(e.value.verdict)) == (engine.GC_E_ARG, BAD, [0, ref.verdict(ref.LENGTH), 0])
        assert not e.value.out[BAD].any()
        others_unchanged(e.value.out, c.run["bits"])
    # n longer than ceil(nout / 8) but fitting: accepted, the high bits dropped
    value = int.from_bytes(c.run["bits"][BAD].tobytes(), "little")
    n = nb8 + 3
    assert 4 + n <= stride
    long = (value | 1 << c.g.nout | 1 << (8 * n - 1)).to_bytes(n, "big")
    raw = np.full((S, stride), cases.FILL, np.uint8)
    raw[:, :slot] = clean
    raw[BAD, :4 + n] = np.frombuffer(ref.be32(n) + long, np.uint8)
    dy.d_slots[2].upload(raw)
    bits, v = dy.evaluator_result()
    assert not v.any() and (bits == c.run["bits"]).all()
    assert ref.evaluator_result(c.g, raw[BAD].tobytes(), stride) == (c.run["bits"][BAD].tobytes(), 0)
