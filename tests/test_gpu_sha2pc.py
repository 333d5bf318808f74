"""The four sha2pc rounds for S sessions per call (gc_sha2pc_*) on the device: Go's own transcript as one session among
three, every byte of every round of a small circuit against the Python reference at the shapes where the kernels change
path, a second call on the same handles, and the host forms."""
import hashlib

import numpy as np
import pytest

from mpc_amd import LABEL, engine
from tests import go_transcript as gt
from tests import py_sha2pc_reference as ref
from tests import sha2pc_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


def composed(ctx, dc, g, s):
    """one session through the existing one-session calls (gc_co_*, gc_garble, gc_eval), encoded on the host"""
    lb = gt.label_bytes
    A, ainv = engine.co_sender_setup(s["a"])
    r1 = b"R1" + s["sid"] + gt.CURVE_CHUNK + A.tobytes()
    pts = engine.co_receiver_choices(ctx, A, [int.from_bytes(b, "big") for b in s["scalars"]], s["ebits"])
    signs = np.packbits(pts[:, 63] & 1, bitorder="little").tobytes()
    r2 = b"R2" + s["sid"] + gt.CURVE_CHUNK + pts[:, :32].tobytes() + signs
    gar = dc.garble(s["key"], s["rnd"], batch=1)
    io, slab = gar["io"][0], gar["slab"][0]
    win, wout = io[:g.ng + g.ne], io[g.ng + g.ne:]
    ct = engine.co_sender_encrypt(ctx, s["a"], ainv, pts, win[g.ng:])
    ginputs = b"".join(lb(win[i]["l1" if s["gbits"][i] else "l0"]) for i in range(g.ng))
    hints = b"".join(lb(w["l0"]) + lb(w["l1"]) for w in wout)
    r3 = b"R3" + s["sid"] + s["key"] + lb(slab) + ginputs + hints + ct.tobytes()
    got = engine.co_receiver_decrypt(ctx, A, [int.from_bytes(b, "big") for b in s["scalars"]], s["ebits"], ct)
    inputs = np.zeros(g.ng + g.ne, LABEL)
    inputs[:g.ng] = [win[i]["l1" if s["gbits"][i] else "l0"] for i in range(g.ng)]
    inputs[g.ng:] = got
    out = dc.eval(s["key"], slab, inputs=inputs[None, :], batch=1)[0]
    bits = [1 if out[j] == wout[j]["l1"] else 0 for j in range(g.nout)]
    assert all(out[j] == wout[j]["l1" if bits[j] else "l0"] for j in range(g.nout))
    digest = np.packbits(np.array(bits, np.uint8), bitorder="little").tobytes()
    return {"r1": r1, "r2": r2, "r3": r3, "digest": digest, "A": A.tobytes(), "AaInv": ainv.tobytes(),
            "verdicts": (0, 0, 0, 0)}


def test_gos_transcript_is_session_1_of_3(ctx, sha_circ):
    g = cases.SHA256XOR
    sessions = [cases.seeded_session(g, "t0"), cases.go_session("transcript"), cases.seeded_session(g, "t2")]
    dc = engine.DeviceCircuit(ctx, sha_circ)
    dr = cases.DeviceRounds(dc, g, 3)
    assert dr.len == [80, 8240, gt.ROUND3_LEN] and dr.stride[2] == 707152
    got = dr.run(sessions)
    h = lambda a: hashlib.sha256(a.tobytes()).hexdigest()
    assert not got["verdicts"].any()
    assert (h(got["r1"][1]), h(got["r2"][1]), h(got["r3"][1])) == gt.CASES["transcript"][1]
    assert got["digest"][1].tobytes().hex() == gt.EXP_FINAL
    for s in (0, 2):
        cases.assert_equal_to_reference(got, composed(ctx, dc, g, sessions[s]), s)
    dr.close()
    dc.close()


@pytest.mark.parametrize("S,ne", [(1, 67), (3, 9), (65, 1), (130, 1)])
def test_small_circuit_against_the_python_reference(ctx, S, ne):
    """(1, 67): past one wave of OTs and a partial sign byte; (65, 1), (130, 1): past one and two bstrides of 64"""
    circ, g = cases.small_circuit(3, ne)
    sessions = [cases.seeded_session(g, "small/%d/%d/%d" % (S, ne, s)) for s in range(S)]
    garble, evaluate = cases.oracle_garble(circ, g), cases.oracle_evaluate(circ, g)
    dc = engine.DeviceCircuit(ctx, circ)
    dr = cases.DeviceRounds(dc, g, S)
    got = dr.run(sessions)
    for s in range(S):
        cases.assert_equal_to_reference(got, cases.reference_rounds(g, sessions[s], garble, evaluate), s)
    assert got["digest"].any()
    dr.close()
    dc.close()


def test_handles_serve_a_second_call_and_the_host_forms_agree(ctx):
    S, ne = 3, 9
    circ, g = cases.small_circuit(3, ne)
    garble, evaluate = cases.oracle_garble(circ, g), cases.oracle_evaluate(circ, g)
    dc = engine.DeviceCircuit(ctx, circ)
    dr = cases.DeviceRounds(dc, g, S)
    first = [cases.seeded_session(g, "reuse/a/%d" % s) for s in range(S)]
    second = [cases.seeded_session(g, "reuse/b/%d" % s) for s in range(S)]
    one = dr.run(first)
    two = dr.run(second)
    assert (one["r3"] != two["r3"]).any()
    for s in range(S):
        cases.assert_equal_to_reference(two, cases.reference_rounds(g, second[s], garble, evaluate), s)
    # the host forms on packed payloads
    rows = lambda what: cases.rows_of(second, what)
    A, ainv, r1 = dr.gb.round1(rows("a"), rows("sid"))
    A2, sid2, r2 = dr.ev.round2(r1, rows("scalars"), rows("ebits"))
    r3 = dr.gb.round3(rows("a"), ainv, rows("sid"), r2, rows("key"), rows("rnd"), rows("gbits"))
    digest = dr.ev.round4(A2, sid2, rows("scalars"), rows("ebits"), r3)
    for name, host in (("r1", r1), ("r2", r2), ("r3", r3), ("digest", digest), ("A", A), ("AaInv", ainv), ("A2", A2),
                       ("sid2", sid2)):
        assert host.shape == two[name].shape and (host == two[name]).all(), name
    # a bad session of a host form: every good session is written, the lowest bad one is reported
    a = rows("a").copy()
    a[1] = 0
    with pytest.raises(engine.Sha2pcSessionError) as e:
        dr.gb.round1(a, rows("sid"))
    assert e.value.code == engine.GC_E_ARG and e.value.bad_session == 1
    assert list(e.value.verdict) == [0, engine.SHA2PC_SETUP, 0]
    bA, bainv, br1 = e.value.out
    assert not br1[1].any() and not bA[1].any() and (br1[0] == r1[0]).all() and (br1[2] == r1[2]).all()
    bad2 = r2.copy()
    bad2[2, 16:48] = 0xFF  # X >= p at index 0 of session 2
    with pytest.raises(engine.Sha2pcSessionError) as e:
        dr.gb.round3(rows("a"), ainv, rows("sid"), bad2, rows("key"), rows("rnd"), rows("gbits"))
    assert e.value.code == engine.GC_E_POINT and e.value.bad_session == 2
    assert list(e.value.verdict) == [0, 0, engine.SHA2PC_POINT]
    assert not e.value.out[2].any() and (e.value.out[:2] == r3[:2]).all()
    dr.close()
    dc.close()


def test_create_refuses_what_it_cannot_serve(ctx):
    circ, g = cases.small_circuit(3, 9)
    dc = engine.DeviceCircuit(ctx, circ)
    with pytest.raises(engine.EngineError) as e:
        engine.Sha2pcGarbler(dc, 3, 8, 2)
    assert e.value.code == engine.GC_E_ARG and b"input count" in engine.lib().gc_last_error()
    with pytest.raises(engine.EngineError):
        engine.Sha2pcEvaluator(dc, 12, 0, 2)
    with pytest.raises(engine.EngineError):
        engine.Sha2pcEvaluator(dc, 3, 9, 0)
    dc.close()
