"""Hostile input to the sha2pc rounds of S sessions (gc_sha2pc_*): one call of 8 sessions carries one fault each in sessions
1 - 7.  The expected verdicts and bytes come from the Python reference on the same bytes (checked on the CPU below); a bad
session's outputs are zero and every other session is what the clean run gives.  All shapes are fixed and no payload byte
is an index, so nothing here can reach an address."""
import functools

import numpy as np
import pytest

from tests import go_transcript as gt
from tests import py_sha2pc_reference as ref
from tests import sha2pc_cases as cases

S, NG, NE = 8, 3, 9
V = ref.verdict


def non_residue_x():
    """an X below p for which x^3 - 3x + b is no square"""
    return next(x for x in range(2, 100) if ref.decompress(x, 0) is None)


@functools.lru_cache(maxsize=None)
def hostile_case():
    """the clean reference run of 8 sessions, the tampered Round 2 and Round 3 payloads, and what the reference says to them"""
    circ, g = cases.small_circuit(NG, NE)
    garble, evaluate = cases.oracle_garble(circ, g), cases.oracle_evaluate(circ, g)
    sessions = [cases.seeded_session(g, "hostile/%d" % s) for s in range(S)]
    clean = [cases.reference_rounds(g, s, garble, evaluate) for s in sessions]
    assert all(c["verdicts"] == (0, 0, 0, 0) for c in clean)
    r2 = [bytearray(c["r2"]) for c in clean]
    r2[1][0] = ord("Q")                                                  # the Round 2 magic
    r2[2][5] ^= 0x40                                                     # the sid
    r2[3][13] = ord("3")                                                 # the curve chunk: "P-356"
    r2[4][16:48] = (gt.P + 1).to_bytes(32, "big")                        # X >= p at index 0
    r2[5][16 + 32 * (NE - 1):16 + 32 * NE] = non_residue_x().to_bytes(32, "big")  # a non-residue X at the last index
    r2[6][16 + 32 * NE] ^= 1 << 4                                        # the sign bit of point 4: -B, a valid point
    want3 = [ref.garbler_round3(g, s["a"], c["AaInv"], s["sid"], bytes(p), s["key"], s["rnd"], s["gbits"], garble)
             for s, c, p in zip(sessions, clean, r2)]
    # session 7: a table byte, chosen as the first row whose change turns an output label into neither hint
    r3 = [bytearray(p) for p, _ in want3]
    for row in range(g.rows):
        trial = bytearray(r3[7])
        trial[42 + 16 * row + 3] ^= 0x10
        _, v = ref.evaluator_round4(g, clean[7]["A"], sessions[7]["sid"], sessions[7]["scalars"], sessions[7]["ebits"],
                                    bytes(trial), evaluate)
        if v & 0xFF == ref.LABEL:
            r3[7] = trial
            break
    want4 = [ref.evaluator_round4(g, c["A"], s["sid"], s["scalars"], s["ebits"], bytes(p), evaluate)
             for s, c, p in zip(sessions, clean, r3)]
    return {"circ": circ, "g": g, "sessions": sessions, "clean": clean, "r2": r2, "want3": want3, "r3": r3, "want4": want4}


def test_the_reference_fails_the_checks_the_faults_aim_at():
    c = hostile_case()
    v3 = [v for _, v in c["want3"]]
    assert v3 == [0, V(ref.MAGIC), V(ref.SESSION), V(ref.CURVE), V(ref.POINT, 0), V(ref.POINT, NE - 1), 0, 0]
    for s in range(1, 6):
        assert not any(c["want3"][s][0])
    # the flipped sign bit: the session stays good, ciphertext 4 alone is another (that of -B)
    good, clean = c["want3"][6][0], c["clean"][6]["r3"]
    at = len(clean) - 32 * NE
    assert good[:at] == clean[:at]
    assert [good[at + 32 * i:at + 32 * i + 32] != clean[at + 32 * i:at + 32 * i + 32] for i in range(NE)] == [i == 4 for i in range(NE)]
    v4 = [v for _, v in c["want4"]]
    assert v4[0] == 0 and v4[1:6] == [V(ref.MAGIC)] * 5 and v4[7] & 0xFF == ref.LABEL
    assert not any(c["want4"][7][0]) and c["want4"][0][0] == c["clean"][0]["digest"]
    # session 6 decrypts a label of -B's ciphertext with B's scalar: whatever the reference makes of it is what is expected
    assert v4[6] == 0 or v4[6] & 0xFF == ref.LABEL


@pytest.mark.gpu
def test_one_fault_per_session_leaves_the_others_untouched():
    from mpc_amd import engine
    c = hostile_case()
    g, sessions = c["g"], c["sessions"]
    ctx = engine.Context(0)
    dc = engine.DeviceCircuit(ctx, c["circ"])
    dr = cases.DeviceRounds(dc, g, S)
    clean = dr.run(sessions)
    for s in range(S):
        cases.assert_equal_to_reference(clean, c["clean"][s], s)
    # rounds 1 and 2 once more, then the tampered Round 2 payloads into the slots
    dr.round1()
    dr.round2()
    dr.set_payloads(1, np.stack([np.frombuffer(bytes(p), np.uint8) for p in c["r2"]]))
    r3, v3 = dr.round3()
    assert [int(v) for v in v3] == [v for _, v in c["want3"]]
    for s in range(S):
        assert r3[s].tobytes() == c["want3"][s][0], "round 3, session %d" % s
    for s in range(1, 6):
        assert not r3[s].any()
    assert (r3[0] == clean["r3"][0]).all() and (r3[7] == clean["r3"][7]).all()
    # the tampered table byte of session 7 into the slots
    dr.set_payloads(2, np.stack([np.frombuffer(bytes(p), np.uint8) for p in c["r3"]]))
    digest, v4 = dr.round4()
    assert [int(v) for v in v4] == [v for _, v in c["want4"]]
    for s in range(S):
        assert digest[s].tobytes() == c["want4"][s][0], "round 4, session %d" % s
    assert (digest[0] == clean["digest"][0]).all() and not digest[7].any()
    dr.close()
    dc.close()
    ctx.close()
