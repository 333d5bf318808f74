"""What keeps the device cases of tests/test_gpu_stream_batch_geometry.py, _hostile.py and _alias.py honest, without a GPU: every
step of tests/stream_batch_cases.py is garbled once by the oracle, read by tests/hostile_fuzz.parse, and has the byte geometry
it claims — where its table rows lie against the 4096-byte piece boundaries of k_sb_serialise / k_sb_ingest, how long it is,
how it ends; gc_stream_batch_step_bytes gives the oracle's length; every circuit is inside the keyed scope at 3, 5 and 67
sessions.  The mutants of the hostile test reach the coverage it asks for by the oracle's and hostile_fuzz.stricter's verdict
alone, and every generated in-place step has a size (is not refused by its shape)."""
import numpy as np
import pytest

import oracle
from mpc_amd import engine
from tests import hostile_fuzz as hf
from tests import keyed_geometry as kg
from tests import stream_batch_cases as sc
from tests.util import drbg


def garbled(name):
    c, in_, out_ = sc.case(name)
    og = oracle.Stream(drbg("geo-key", 32), drbg("geo-rnd", 16 * (len(in_) + 1)), in_)
    data = og.garble(c.Gates, c.NumWires, in_, out_)
    parsed, err = hf.parse(data, c.NumGates)
    assert err is None and parsed[-1][6] + 16 * parsed[-1][7] == len(data)
    return c, in_, out_, data, parsed


@pytest.mark.parametrize("name", sc.NAMES)
def test_case_has_the_geometry_it_claims(name):
    c, in_, out_, data, parsed = garbled(name)
    claim = sc.GEOMETRY[name]
    n = len(data)
    rows = sc.rows_of(parsed)
    assert n == claim["nbytes"] and n <= 20 * sc.PIECE
    assert engine.stream_batch_step_bytes(c.Gates, c.NumWires, in_, out_) == n
    assert len(rows) == c.slab_rows() and rows == sorted(rows)
    if "nrows" in claim:
        assert len(rows) == claim["nrows"]
    else:
        assert len(rows) > 0
    bounds = range(sc.PIECE, n, sc.PIECE)
    straddles = {b - off for off, b in sc.straddlers(parsed, n)}
    ends_on = [off for off in rows if off + 16 in bounds]
    starts_on = [off for off in rows if off in bounds]
    print("%s: %d bytes (%d mod 4), %d pieces, %d rows, straddles %s, rows ending on a boundary %s, starting on one %s" % (
        name, n, n % 4, -(-n // sc.PIECE), len(rows), sorted(straddles), ends_on, starts_on))
    assert straddles >= claim.get("straddles", set())
    if claim.get("ends_on"):
        assert ends_on and starts_on
    if "widths" in claim:
        assert {2 if data[q[0]] & 0x10 else 4 for q in parsed} == claim["widths"]
    # the step ends in structure: a flipped last byte is one the ingester must count
    assert not sc.row_mask(parsed, n)[-1]
    if name == "tiny":
        assert n < 16 and parsed[0][1] == 0 and parsed[0][3] and not parsed[0][2] & 0x20  # a short-form XOR into a global wire
    if name == "norows":
        assert -(-n // sc.PIECE) == 2 and {q[1] for q in parsed} == {0, 1}
    if name.startswith("straddle"):
        assert {q[1] for q in parsed} >= {2, 3, 4}  # AND, OR and INV


def test_tails_reach_every_length_residue_and_the_exact_piece_counts():
    lens = {name: sc.GEOMETRY[name]["nbytes"] for name in sc.TAIL_CASES}
    assert [lens["tail%d" % t] - sc.PIECE for t in sc.TAILS] == [0, 1, 2, 3, 5, 15, 16, 17]
    assert lens["tail2x"] == 2 * sc.PIECE
    assert {n % 4 for n in lens.values()} == {0, 1, 2, 3}


@pytest.mark.parametrize("name", sc.NAMES)
def test_case_is_inside_the_keyed_scope(name):
    c, _, _ = sc.case(name)
    fig = kg.plan_figures(c)
    for S in sc.SESSIONS:
        shape = kg.Shape(*fig, S)
        assert shape.keyed and shape.ti == 1, (name, S, shape.as_tuple())
    assert sc.PATH[name] == 1  # (keyed with the wires in LDS: path 1 of gc_batch_keyed_path)


def test_hostile_mutants_reach_the_coverage_by_the_oracles_verdict():
    """the conditions tests/test_gpu_stream_batch_hostile.py asserts on the device, predicted here from the oracle and
    hostile_fuzz.stricter alone: an accepted mutant is one the oracle walks for every session and the engine does not refuse by
    design"""
    from tests import test_gpu_stream_batch_hostile as hb
    kinds, accepted, refused = {}, 0, 0
    for k in range(len(hf.programs())):
        prog = hb.Program(k)
        for m, (mut, mng, what) in enumerate(prog.mutants()):
            kinds[what] = kinds.get(what, 0) + 1
            blocks = prog.session_blocks(m, mut, mng)
            why = hf.stricter(mut, mng, prog.ntmp, prog.nw)
            ok = why is None and all(u is not None for u in prog.oracle_run(blocks, mng)[0])
            accepted, refused = accepted + ok, refused + (not ok)
    print("mutants by kind %s, accepted %d, refused %d" % (kinds, accepted, refused))
    hb.check_coverage(kinds, accepted, refused)


def test_every_generated_in_place_step_has_a_size():
    from tests import test_gpu_stream_batch_alias as al
    shapes = set()
    for k in range(al.NSTEPS):
        gates, nwires, in_, out_, what = al.step(k)
        assert 8 <= len(gates) <= 40
        assert engine.stream_batch_step_bytes(gates, nwires, in_, out_) > 0, (k, engine.lib().gc_last_error())
        assert set(in_) & set(out_)
        shapes |= what
    assert shapes >= {"out repeats an id", "in repeats an id", "all of out in in", "read before and after the set"}
    assert {int(op) for k in range(al.NSTEPS) for op in al.step(k)[0]["op"]} == {0, 1, 2, 3, 4}
