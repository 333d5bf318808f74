"""tests/yao_shape_cases.py gives what the GPU cases of tests/test_gpu_yao_shapes.py and tests/test_gpu_yao_hostile_shapes.py
rely on: rows and labels of M1 across piece boundaries with 4, 8 and 12 bytes in the earlier piece, row words on the first
and the last word of a piece, a row at a piece's start, message tails of 0, 1, 2 and 3 words, a last piece that is exactly
full, the wide circuit's piece counts, the spoilt gates of the hostile test in the pieces it says, and directed results with
their highest bit at the edges of the decode kernel's ballots.  No GPU: a change of a circuit generator cannot empty a case
unseen."""
import pytest

from tests import py_yao_reference as ref
from tests import yao_shape_cases as sc


@pytest.mark.parametrize("keylen,piece", [(32, 64), (16, 80)])
def test_small_circuit_edges_at_small_pieces(keylen, piece):
    g = sc.geometry("small", keylen)
    assert sc.crossings(sc.row_offsets(g), piece) == {4, 8, 12}
    assert sc.crossings(sc.label_offsets(g), piece) == {8}
    assert sc.gates_first_word(g, piece) and sc.gates_last_word(g, piece)
    assert sc.begin_at_a_piece(sc.row_offsets(g), piece)
    assert sc.tail_words(g) == 2 and not sc.last_piece_full(g, piece)
    if keylen == 32:
        assert (ref.len1(g), sc.npieces(g, piece)) == (1160, 19)


def test_small_circuit_at_24_byte_keys_has_no_tail_and_a_full_last_piece():
    g = sc.geometry("small", 24)
    assert sc.tail_words(g) == 0 and sc.last_piece_full(g, 64) and sc.npieces(g, 64) * 64 == ref.len1(g)
    assert sc.crossings(sc.row_offsets(g), 64) == {4, 8, 12}


BITWISE = {(67, 16): (3508, 1), (67, 24): (3516, 3), (69, 16): (3612, 3), (69, 24): (3620, 1)}


@pytest.mark.parametrize("bits,keylen", sorted(BITWISE))
def test_bitwise_and_lengths_and_tails(bits, keylen):
    g = sc.geometry("and%d" % bits, keylen)
    assert (g.ng, g.ne, g.nout, len(g.rows), sum(g.rows)) == (bits, bits, bits, bits, 2 * bits)
    assert (ref.len1(g), sc.tail_words(g)) == BITWISE[bits, keylen]
    at_labels = sc.label_offsets(g)[0]
    assert at_labels % 16 == ref.len1(g) % 16
    # a label's first byte is 4 tail words behind a line: 16 - 4 tail bytes of it lie in the earlier piece
    assert sc.crossings(sc.label_offsets(g), 64) == {16 - 4 * sc.tail_words(g)}
    assert sc.crossings(sc.row_offsets(g), 64) == {4, 8, 12}
    # at the default piece the message is one piece: the tail is all that differs there
    assert sc.npieces(g, sc.DEFAULT_SHAPE[1]) == 1


def test_the_chosen_set_covers_every_tail_and_every_crossing():
    chosen = [("small", 32), ("small", 16), ("small", 24)] + [("and%d" % b, k) for b, k in BITWISE]
    gs = [sc.geometry(n, k) for n, k in chosen]
    assert {sc.tail_words(g) for g in gs} == {0, 1, 2, 3}
    assert set().union(*(sc.crossings(sc.row_offsets(g), 64) for g in gs)) == {4, 8, 12}
    assert set().union(*(sc.crossings(sc.label_offsets(g), 64) for g in gs)) == {4, 8, 12}


def test_wide_circuit_pieces():
    g = sc.geometry("wide", 32)
    assert (g.ng, g.ne) == (5, 9) and ref.len1(g) == 20008
    assert sc.npieces(g, 4096) == 5 and sc.npieces(g, 16384) == 2


def test_hostile_gates_lie_where_the_gpu_test_says():
    g = sc.geometry("small", 32)
    h = sc.hostile_gates(g, 64)
    lo, hi = h["pair"]
    assert 0 < lo < hi < h["last"] == len(g.rows) - 1
    assert sc.piece_of_gate(g, 64, lo) != sc.piece_of_gate(g, 64, hi)
    assert ref.gate_offsets(g)[h["first_of_piece"]] % 64 == 0 and h["first_of_piece"] not in (0, lo, hi, h["last"])
    # 1 027 sessions in tiles of 4: the last tile holds three, and 1 023 / 1 024 are the two sides of a tile boundary
    assert 1027 % 4 == 3 and 1023 // 4 != 1024 // 4 == 1026 // 4


@pytest.mark.parametrize("nout", sc.DIRECTED_NOUT)
def test_directed_results(nout):
    vs = sc.directed_values(nout)
    assert len(vs) == len(set(vs)) and all(0 <= v < 1 << nout for v in vs)
    assert {0, 1, 1 << 7, 1 << 8, 1 << 63, (1 << 64) - 1, 1 << (nout - 1), (1 << nout) - 1} <= set(vs)
    if nout > 64:
        assert {1 << 64, (1 << 64) | 1} <= set(vs)
    # a dead wave in the last decode block (four sessions a block), a ragged tile of 16 sessions in k_yao_m2_out
    assert len(vs) % 4 and len(vs) % 16
    # highest set bits: none, inside the first ballot, its last bit, the second ballot's first bit, the last output
    tops = {v.bit_length() - 1 for v in vs}
    assert {-1, 0, 7, 8, 63, nout - 1} <= tops and (nout == 64 or 64 in tops)
    # ones in the first ballot alone next to a second (and third) ballot of zeros, and the other way round
    if nout > 64:
        assert any(v and v < 1 << 64 for v in vs) and (1 << 64) in vs
    g = sc.geometry("and%d" % nout, 32)
    assert g.nout == nout and (nout % 16 != 0) == (nout != 64)
    for s, (v, ses) in enumerate(zip(vs, sc.directed_sessions(nout))):
        assert ses["gbits"] == [1] * nout and sum(b << i for i, b in enumerate(ses["ebits"])) == v
        assert ses["key"] == sc.session("and%d" % nout, 32, s)["key"]
        want = sc.directed_expectation(nout, v)
        assert want["m3"] == ref.pack_result(g, want["bits"]) and want["len3"] == len(want["m3"])
    assert sc.directed_expectation(nout, 0) == {"m3": bytes(4), "len3": 4, "bits": bytes((nout + 7) // 8)}
