"""circuit.Garbler / circuit.Evaluator for S sessions per call (gc_yao_*) on the device: every byte of M1, M2, M3, len3 and
the bits of every session against the Python restatement (tests/py_yao_reference.py) at the shapes where the kernels change
path, the three key lengths, a message of several pieces with a row across a piece boundary, aes_128 against the one-session
wire call, keyed path 2, a whole chain through the Chou-Orlandi OT calls, a second call on the same handles, the host forms
and a captured send."""
import numpy as np
import pytest

import oracle
from mpc_amd import engine
from mpc_amd.circuit import synthetic_levelised
from tests import py_yao_reference as ref
from tests import sha2pc_cases
from tests import yao_cases as cases
from tests.util import bits_lsb, drbg

pytestmark = pytest.mark.gpu

TILE, PIECE = engine.yao_kernel_shape()  # host arithmetic: no device needed


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


def run_and_compare(ctx, circ, g, S, tag, extra_stride=0, path=0):
    sessions = [cases.session(g, "%s/%d" % (tag, s)) for s in range(S)]
    dc = engine.DeviceCircuit(ctx, circ)
    dy = cases.DeviceYao(dc, g, S, extra_stride)
    if path:
        dy.gb.batch.set_keyed_path(path)
        dy.ev.batch.set_keyed_path(path)
        assert dy.gb.batch.keyed_path == dy.ev.batch.keyed_path == path
    got = dy.run(sessions)
    for s in range(S):
        cases.assert_equal_to_reference(got, cases.reference(circ, g, sessions[s]), s)
    dy.close()
    dc.close()
    return got


@pytest.mark.parametrize("S,ng,ne", [(1, 3, 67), (3, 3, 9), (65, 1, 1), (130, 0, 2), (TILE - 1, 3, 9), (TILE, 3, 9), (TILE + 1, 3, 9)])
def test_small_circuit_against_the_python_reference(ctx, S, ng, ne):
    """(65, 1, 1), (130, 0, 2): past one and two bstrides of 64, and no garbler input; TILE - 1 .. TILE + 1: around the M1
    kernels' session tile"""
    circ, _ = sha2pc_cases.small_circuit(ng, ne)
    got = run_and_compare(ctx, circ, ref.geometry(circ, ng, ne, 32), S, "small/%d/%d/%d" % (S, ng, ne))
    assert got["bits"].any() or S == 1


@pytest.mark.parametrize("keylen", [16, 24, 32])
def test_every_key_length_and_a_wider_stride(ctx, keylen):
    circ, _ = sha2pc_cases.small_circuit(3, 9)
    run_and_compare(ctx, circ, ref.geometry(circ, 3, 9, keylen), 3, "keylen/%d" % keylen, extra_stride=32)


def test_a_message_of_several_pieces_with_a_row_across_a_boundary(ctx):
    circ = synthetic_levelised(8, 96, 0.5, 21, ninputs=14, or_frac=0.1, inv_frac=0.1)
    g = ref.geometry(circ, 5, 9, 32)
    goff = ref.gate_offsets(g)
    roff = [o + 4 + 16 * r for o, n in zip(goff, g.rows) for r in range(n)]
    assert ref.len1(g) > 2 * PIECE, "M1 spans at least three pieces"
    assert any(o < p * PIECE < o + 16 for o in roff for p in range(1, ref.len1(g) // PIECE + 1)), "a row lies across a piece boundary"
    run_and_compare(ctx, circ, g, 3, "pieces")


def test_keyed_path_2_gives_the_same_bytes(ctx):
    circ, _ = sha2pc_cases.small_circuit(3, 9)
    g = ref.geometry(circ, 3, 9, 32)
    one = run_and_compare(ctx, circ, g, 3, "path")
    two = run_and_compare(ctx, circ, g, 3, "path", path=2)
    for k in ("m1", "m2", "m3", "len3", "bits"):
        assert (one[k] == two[k]).all(), k


def test_aes_128_against_the_one_session_wire_call(ctx, aes_circ):
    S, g = 3, ref.geometry(aes_circ, 128, 128, 32)
    keys, pts = [drbg("yao/aes/k%d" % s, 16) for s in range(S)], [drbg("yao/aes/p%d" % s, 16) for s in range(S)]
    sessions = [cases.session(g, "aes/%d" % s) for s in range(S)]
    for s in range(S):
        sessions[s]["gbits"] = list(bits_lsb(int.from_bytes(keys[s], "big"), 128))
        sessions[s]["ebits"] = list(bits_lsb(int.from_bytes(pts[s], "big"), 128))
    dc = engine.DeviceCircuit(ctx, aes_circ)
    dy = cases.DeviceYao(dc, g, S)
    got = dy.run(sessions)
    assert not got["verdicts"].any()
    for s in range(S):
        one = dc.garble_wire(sessions[s]["key"], sessions[s]["rnd"], batch=1)
        head = ref.be32(32) + sessions[s]["key"]
        wire = one["wire"][0, :dc.tables_wire_bytes].tobytes()
        m1 = got["m1"][s].tobytes()
        assert m1[:len(head)] == head and m1[len(head):len(head) + len(wire)] == wire, "session %d: tables differ from gc_garble_wire" % s
        io = one["io"][0]
        own = b"".join(ref.gt.label_bytes(io[i]["l1" if sessions[s]["gbits"][i] else "l0"]) for i in range(128))
        assert m1[len(head) + len(wire):] == own
        ct = int.from_bytes(got["bits"][s].tobytes(), "little").to_bytes(16, "big")
        assert ct == oracle.aes_encrypt(keys[s], pts[s]) and got["ebits"][s].tobytes() == got["bits"][s].tobytes()
        assert int(got["len3"][s]) == 4 + len(ct.lstrip(b"\0")) and got["m3"][s, 4:int(got["len3"][s])].tobytes() == ct.lstrip(b"\0")
    dy.close()
    dc.close()


def test_a_whole_chain_through_the_chou_orlandi_calls(ctx):
    """the OT between ot_wires_dev and eval_dev is gc_co_multi_*_dev: setup, choices, encrypt, decrypt"""
    S, ng, ne = 3, 3, 9
    circ, _ = sha2pc_cases.small_circuit(ng, ne)
    g = ref.geometry(circ, ng, ne, 32)
    sessions = [cases.session(g, "chain/%d" % s) for s in range(S)]
    dc = engine.DeviceCircuit(ctx, circ)
    dy = cases.DeviceYao(dc, g, S)
    dy.load(sessions)
    m1 = dy.send()
    z = lambda n: ctx.zeros(n)
    d_a = ctx.to_device(np.frombuffer(drbg("yao/chain/a", 32 * S), np.uint8))
    d_sc = ctx.to_device(np.frombuffer(drbg("yao/chain/scalars", 32 * S * ne), np.uint8))
    d_choice = ctx.to_device(dy.ebits)
    d_A, d_ainv, d_pts, d_ct, d_st = z(64 * S), z(64 * S), z(64 * S * ne), z(32 * S * ne), z(32)
    engine.co_multi_sender_setup_dev(ctx, d_a, S, d_A, d_ainv, d_st)
    assert not dy.accept().any()
    engine.co_multi_receiver_choices_dev(ctx, d_A, d_sc, d_choice, S, ne, d_pts, d_st)
    dy.gb.ot_wires_dev(dy.d_wires)
    engine.co_multi_sender_encrypt_dev(ctx, d_a, d_ainv, d_pts, dy.d_wires, S, ne, 0, d_ct, d_st)
    engine.co_multi_receiver_decrypt_dev(ctx, d_A, d_sc, d_choice, d_ct, S, ne, 0, dy.d_labels, d_st)
    m2, v2 = dy.eval()
    m3, len3, gbits, v3 = dy.garbler_result()
    ebits, v4 = dy.evaluator_result()
    assert not d_st.download(np.uint64, (4,))[[0, 2]].any() and not (v2.any() or v3.any() or v4.any())
    for s in range(S):
        want = cases.reference(circ, g, sessions[s])
        assert m1[s].tobytes() == want["m1"] and m2[s].tobytes() == want["m2"] and m3[s, :len3[s]].tobytes() == want["m3"]
        assert gbits[s].tobytes() == ebits[s].tobytes() == want["bits"]  # = the plaintext circuit (cases.reference asserts it)
    dy.close()
    dc.close()


def test_a_second_call_the_host_forms_and_a_captured_send(ctx):
    S, ng, ne = 3, 3, 9
    circ, _ = sha2pc_cases.small_circuit(ng, ne)
    g = ref.geometry(circ, ng, ne, 32)
    dc = engine.DeviceCircuit(ctx, circ)
    dy = cases.DeviceYao(dc, g, S)
    first = [cases.session(g, "reuse/a/%d" % s) for s in range(S)]
    second = [cases.session(g, "reuse/b/%d" % s) for s in range(S)]
    one = dy.run(first)
    two = dy.run(second)
    assert (one["m1"] != two["m1"]).any()
    for s in range(S):
        cases.assert_equal_to_reference(two, cases.reference(circ, g, second[s]), s)
    # the host forms on packed messages
    rows = lambda what: cases.rows_of(second, what)
    m1 = dy.gb.send(rows("key"), rows("rnd"), rows("gbits"))
    wires = dy.gb.ot_wires()
    assert not dy.ev.accept(m1).any()
    m2 = dy.ev.eval(np.stack([cases.ot_labels(wires[s], second[s]["ebits"]) for s in range(S)]))
    m3, len3, gbits = dy.gb.result(m2)
    ebits = dy.ev.result(m3)
    assert (m1 == two["m1"]).all() and (m2 == two["m2"]).all() and (len3 == two["len3"]).all()
    assert wires.tobytes() == two["ot_wires"].tobytes() and (gbits == two["bits"]).all() and (ebits == two["bits"]).all()
    for s in range(S):
        assert (m3[s, :len3[s]] == two["m3"][s, :len3[s]]).all() and not m3[s, len3[s]:].any()
    # a captured send replayed after d_keys, d_rnd and d_bits changed = an uncaptured call on the new contents
    dy.load(first)
    dy.d_slots[0].zero(cases.FILL)
    graph = ctx.capture(lambda: dy.gb.send_dev(dy.d_keys, dy.d_rnd, dy.d_gbits, dy.d_slots[0], dy.stride[0]))
    graph.launch()
    assert (dy.slots(0) == one["m1"]).all()
    for d, what in ((dy.d_keys, "key"), (dy.d_rnd, "rnd"), (dy.d_gbits, "gbits")):
        d.upload(rows(what))
    dy.d_slots[0].zero(cases.FILL)
    graph.launch()
    assert (dy.slots(0) == two["m1"]).all()
    graph.close()
    dy.close()
    dc.close()


def test_create_refuses_what_it_cannot_serve(ctx):
    circ, _ = sha2pc_cases.small_circuit(3, 9)
    dc = engine.DeviceCircuit(ctx, circ)
    with pytest.raises(engine.EngineError) as e:
        engine.YaoGarbler(dc, 3, 8, 32, 2)
    assert e.value.code == engine.GC_E_ARG and b"input count" in engine.lib().gc_last_error()
    with pytest.raises(engine.EngineError) as e:
        engine.YaoEvaluator(dc, 3, 9, 20, 2)
    assert e.value.code == engine.GC_E_KEYSIZE
    with pytest.raises(engine.EngineError):
        engine.YaoEvaluator(dc, 12, 0, 32, 2)
    with pytest.raises(engine.EngineError):
        engine.YaoGarbler(dc, 3, 9, 32, 0)
    dc.close()
