"""The other two phases of a session-batched stream and its way to host memory against the oracle values that
tests/test_gpu_stream_batch.reference() holds: the garbler's own input labels (select), the decoded result, the stream bytes
in windows of pinned host memory, the evaluator fed from host memory with a verdict that stays, and one program end to end."""
import threading

import numpy as np
import pytest

from mpc_amd import engine
from mpc_amd.circuit import LABEL
from tests import hostile_fuzz as hf
from tests.test_gpu_stream_batch import check_store, reference
from tests.test_stream_batch_windows import CAPS, HEADER, Model

pytestmark = pytest.mark.gpu

KEYLEN = 32
NEVER_SET = 0x5000  # a wire id no step of the program names


def headers(n=3):
    """the 20 bytes in front of step k (any bytes do: they are the caller's framing, the same for every session)"""
    return [bytes(np.random.default_rng([18, k]).integers(0, 256, HEADER, dtype=np.uint8)) for k in range(n)]


class Garbler:
    """a StreamBatch at the start of the program: the store holds the primary inputs"""

    def __init__(self, ctx, ref, S, run_program=False):
        self.ref, self.S = ref, S
        self.d_keys = engine.DeviceBuffer(ctx, data=ref["keys"])
        self.d_rnd = engine.DeviceBuffer(ctx, data=ref["rnd"])
        self.sb = engine.StreamBatch(ctx, S, self.d_keys, KEYLEN, self.d_rnd, ref["prim"])
        if run_program:
            n = max(engine.stream_batch_step_bytes(c.Gates, c.NumWires, i, o) for c, i, o in ref["steps"])
            stride = (n + 3) & ~3
            d_out = engine.DeviceBuffer(ctx, shape=S * stride)
            for c, in_, out_ in ref["steps"]:
                self.sb.garble(c.Gates, c.NumWires, in_, out_, d_out, stride)
            d_out.close()

    def close(self):
        self.sb.close()
        self.d_keys.close(), self.d_rnd.close()


def labels_of(ref, ids, bits):
    """LABEL [S, len(ids)]: l1 where the bit is not zero, else l0, from the oracle's wires"""
    out = np.zeros(bits.shape, LABEL)
    for j, w in enumerate(ids):
        out[:, j] = np.where(bits[:, j] != 0, ref["wires"][w]["l1"], ref["wires"][w]["l0"])
    return out


def mixed(bits):
    """the same bits with every other 1 written as 0x80: a non-zero byte is 1"""
    b = bits.astype(np.uint8).copy()
    b[:, ::2] *= 0x80
    return b


# ---- select ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [5, 67, 1027])
def test_select_gives_the_oracles_input_labels(S):
    ctx = engine.Context(0)
    ref = reference(S, 0, KEYLEN)
    g = Garbler(ctx, ref, S)
    prim = ref["prim"]
    bits = mixed(ref["bits"])
    assert set(np.unique(bits)) == {0, 1, 0x80}
    d_out = engine.DeviceBuffer(ctx, shape=(S, len(prim)), dtype=LABEL)
    g.sb.select_labels(prim, engine.DeviceBuffer(ctx, data=bits), d_out)
    want = labels_of(ref, prim, bits)
    assert (d_out.numpy() == want).all()
    assert (g.sb.select_labels(prim, bits) == want).all()  # the host form
    # one id; an id repeated; a wire never set: 0 or R[s]
    r = ref["wires"][prim[0]]
    R = np.zeros(S, LABEL)
    R["d0"], R["d1"] = r["l0"]["d0"] ^ r["l1"]["d0"], r["l0"]["d1"] ^ r["l1"]["d1"]
    one = g.sb.select_labels([prim[7]], bits[:, 7:8])
    assert (one == want[:, 7:8]).all()
    ids = [prim[3], NEVER_SET, prim[3], prim[140], NEVER_SET]
    b = np.zeros((S, 5), np.uint8)
    b[:, 2] = 1
    b[S // 2:, 3] = 7
    b[:, 4] = 0xff
    got = g.sb.select_labels(ids, b)
    w3, w140 = ref["wires"][prim[3]], ref["wires"][prim[140]]
    assert (got[:, 0] == w3["l0"]).all() and (got[:, 2] == w3["l1"]).all()
    assert (got[:, 3] == np.where(b[:, 3] != 0, w140["l1"], w140["l0"])).all()
    assert (got[:, 1] == np.zeros(S, LABEL)).all() and (got[:, 4] == R).all()
    assert g.sb.select_labels([], np.zeros((S, 0), np.uint8)).shape == (S, 0)
    # an id at GC_STREAM_MAX_WIRES (2^28 by default) is refused, by both calls
    for call in (lambda: g.sb.select_labels([prim[0], 1 << 28], b[:, :2]), lambda: g.sb.decode([1 << 28], want[:, :1])):
        with pytest.raises(engine.EngineError) as err:
            call()
        assert err.value.code == engine.GC_E_ARG
    g.close()
    ctx.close()


def test_select_sweeps_the_grid_a_second_time():
    """70 000 ids, more than one grid holds along the ids (1 024 tiles of 64), drawn with repetition from the program's wires
    after the program has run"""
    S, n = 3, 70000
    ctx = engine.Context(0)
    ref = reference(S, 0, KEYLEN)
    g = Garbler(ctx, ref, S, run_program=True)
    wires = ref["prim"] + ref["outs"]
    rng = np.random.default_rng(70000)
    pick = rng.integers(0, len(wires), n)
    ids = np.array(wires, np.uint32)[pick]
    bits = rng.integers(0, 2, (S, n), dtype=np.uint8) * rng.choice(np.array([1, 0x80, 0xff], np.uint8), (S, n))
    l0 = np.stack([ref["wires"][w]["l0"] for w in wires], axis=1)  # [S, wires]
    l1 = np.stack([ref["wires"][w]["l1"] for w in wires], axis=1)
    want = np.where(bits != 0, l1[:, pick], l0[:, pick])
    d_out = engine.DeviceBuffer(ctx, shape=(S, n), dtype=LABEL)
    g.sb.select_labels(ids, engine.DeviceBuffer(ctx, data=bits), d_out)
    got = d_out.numpy()
    assert (got[:, :65536] == want[:, :65536]).all() and (got[:, 65536:] == want[:, 65536:]).all()
    # ... and decode of those labels gives the bits back, past the first sweep too
    d_bits, d_bad = engine.DeviceBuffer(ctx, shape=(S, n)), engine.DeviceBuffer(ctx, data=np.full(S, 0xFFFFFFFF, np.uint32))
    g.sb.decode(ids, d_out, d_bits, d_bad)
    assert (d_bits.numpy() == (bits != 0)).all() and (d_bad.numpy() == 0).all()
    g.close()
    ctx.close()


# ---- decode ---------------------------------------------------------------------------------------------------------------------

def evaluator_labels(ref, S):
    outs = ref["outs"]
    lab = np.zeros((S, len(outs)), LABEL)
    for j, o in enumerate(outs):
        for s in range(S):
            lab[s, j] = ref["ev"][o][s]
    vals = np.array([[ref["vals"][s][o] for o in outs] for s in range(S)], np.uint8)
    return lab, vals


@pytest.mark.parametrize("S", [5, 67, 1027])
def test_decode_gives_the_plaintext_values(S):
    ctx = engine.Context(0)
    ref = reference(S, 0, KEYLEN)
    g = Garbler(ctx, ref, S, run_program=True)
    outs = ref["outs"]
    n = len(outs)
    lab, vals = evaluator_labels(ref, S)
    d_bits = engine.DeviceBuffer(ctx, shape=(S, n))
    d_bad = engine.DeviceBuffer(ctx, data=np.full(S, 0xFFFFFFFF, np.uint32))
    g.sb.decode(outs, engine.DeviceBuffer(ctx, data=lab), d_bits, d_bad)
    assert (d_bits.numpy() == vals).all() and (d_bad.numpy() == 0).all()
    bits, bad = g.sb.decode(outs, lab)  # the host form
    assert (bits == vals).all() and (bad == 0).all()
    # one bit flipped in label 3 of session 2, and session 4 all random
    rng = np.random.default_rng(S)
    tam = lab.copy()
    tam["d1"][2, 3] ^= np.uint64(1 << 17)
    tam["d0"][4] = rng.integers(1, 1 << 63, n, dtype=np.uint64)
    d_bad.upload(np.full(S, 0xFFFFFFFF, np.uint32))
    g.sb.decode(outs, engine.DeviceBuffer(ctx, data=tam), d_bits, d_bad)
    bits, bad = d_bits.numpy(), d_bad.numpy()
    want = vals.copy()
    want[2, 3] = 0xff
    want[4] = 0xff
    want_bad = np.zeros(S, np.uint32)
    want_bad[2], want_bad[4] = 1, n
    assert (bits == want).all() and (bad == want_bad).all()
    hb, hbad = g.sb.decode(outs, tam)
    assert (hb == want).all() and (hbad == want_bad).all()
    # no ids: the counts are still zeroed
    d_bad.upload(np.full(S, 0xFFFFFFFF, np.uint32))
    g.sb.decode([], engine.DeviceBuffer(ctx, shape=16), d_bits, d_bad)
    assert (d_bad.numpy() == 0).all()
    g.close()
    ctx.close()


# ---- windows --------------------------------------------------------------------------------------------------------------------

def step_args(ref, k):
    c, in_, out_ = ref["steps"][k]
    return c.Gates, c.NumWires, in_, out_


def expected_stream(ref, s, hdr, times=1):
    return b"".join(hdr[k] + ref["streams"][s][k] for k in range(3)) * times


def drain_one(out, model, got):
    v = out.next_view()
    line = model.event("n")
    if v is None:
        assert line.startswith("n none")
        return False
    assert line.startswith("n (") and int(line.split()[2].rstrip(")")) == v.shape[1]
    got.append(v.copy())
    out.release()
    assert not model.event("r").startswith("r none")
    return True


def run_through_windows(out, model, ref, hdr, got):
    """every step, a consumer that takes one window whenever the garbler is told BUSY — the handle and the model in step"""
    for k in range(3):
        n = HEADER + len(ref["streams"][0][k])
        while True:
            line = model.event("s %d" % n)
            try:
                assert out.garble(hdr[k], *step_args(ref, k)) == n
                assert line.startswith("s ok"), line
                break
            except engine.EngineError as e:
                assert e.code == engine.GC_E_BUSY and line.startswith("s busy"), (e.code, line)
                assert drain_one(out, model, got)
    out.flush()
    model.event("f")
    while drain_one(out, model, got):
        pass


@pytest.mark.parametrize("S", [5, 67])
@pytest.mark.parametrize("nwindows", [2, 3])
@pytest.mark.parametrize("cap", CAPS)
def test_windows_hold_header_and_oracle_bytes(cap, nwindows, S):
    ctx = engine.Context(0)
    ref = reference(S, 0, KEYLEN)
    g = Garbler(ctx, ref, S)
    out, model, hdr, got = g.sb.out(cap, nwindows), Model(cap, nwindows), headers(), []
    run_through_windows(out, model, ref, hdr, got)
    total = sum(HEADER + len(x) for x in ref["streams"][0])
    for s in range(S):
        assert b"".join(w[s].tobytes() for w in got) == expected_stream(ref, s, hdr), "session %d" % s
    assert out.stats() == (model.n_sealed, total, model.grown, model.busy) and model.n_sealed == len(got)
    if cap == 4096:
        assert out.stats()[2] == 2  # steps 1 and 2 exceed the window and each lands on an empty one
    check_store(g.sb, ref)
    with pytest.raises(engine.EngineError) as err:
        out.release()
    assert err.value.code == engine.GC_E_ARG
    out.close(), g.close()
    ctx.close()


def test_busy_leaves_the_store_and_the_repeated_call_is_exact():
    S, cap = 5, 4096
    ctx = engine.Context(0)
    ref = reference(S, 0, KEYLEN)
    g = Garbler(ctx, ref, S)
    out, hdr = g.sb.out(cap, 2), headers()
    with pytest.raises(engine.EngineError) as err:
        g.sb.out(cap, 1)
    assert err.value.code == engine.GC_E_ARG
    out.garble(hdr[0], *step_args(ref, 0))
    out.garble(hdr[1], *step_args(ref, 1))  # seals window 0, grows window 1
    first = out.next_view()                 # ... and now both are held: one handed out, one filling with no room
    assert first.shape == (S, HEADER + len(ref["streams"][0][0]))
    step3_outs = ref["steps"][2][2]
    for rep in range(2):
        with pytest.raises(engine.EngineError) as err:
            out.garble(hdr[2], *step_args(ref, 2))
        assert err.value.code == engine.GC_E_BUSY
        assert "window" in str(err.value)
    assert out.stats() == (1, first.shape[1] + HEADER + len(ref["streams"][0][1]), 1, 2)
    done = [o for k in range(2) for o in ref["steps"][k][2]]
    for w in ref["prim"][::9] + done:
        assert (g.sb.get(w) == ref["wires"][w]).all(), w
    for o in step3_outs:
        assert (g.sb.get(o)["l0"] == np.zeros(S, LABEL)).all(), o  # never set
    got = [first.copy()]
    out.release()
    assert out.garble(hdr[2], *step_args(ref, 2)) == HEADER + len(ref["streams"][0][2])
    out.flush()
    while True:
        v = out.next_view()
        if v is None:
            break
        got.append(v.copy())
        out.release()
    for s in range(S):
        assert b"".join(w[s].tobytes() for w in got) == expected_stream(ref, s, hdr), "session %d" % s
    assert out.stats()[2:] == (2, 2)
    check_store(g.sb, ref)
    # the plain call stays legal beside the handle and its bytes are part of no window
    n = len(ref["streams"][0][0])
    d_out = engine.DeviceBuffer(ctx, shape=S * ((n + 3) & ~3))
    assert g.sb.garble(*step_args(ref, 0), d_out, (n + 3) & ~3) == n
    assert d_out.numpy().reshape(S, -1)[3, :n].tobytes() == ref["streams"][3][0]
    out.flush()
    assert out.next() is None
    out.close(), g.close()
    ctx.close()


def test_a_consumer_thread_takes_the_windows_of_twenty_passes():
    S, cap, times = 5, 18236, 20
    ctx = engine.Context(0)
    ref = reference(S, 0, KEYLEN)
    g = Garbler(ctx, ref, S)
    out, hdr, got, done, failed = g.sb.out(cap, 3), headers(), [], threading.Event(), []

    def consumer():
        try:
            while True:
                finished = done.is_set()  # (read before looking: a window sealed before `done` is still seen)
                v = out.next_view()
                if v is None:
                    if finished:
                        return
                    continue
                got.append(v.copy())
                out.release()
        except Exception as e:  # noqa: BLE001 (reported by the main thread)
            failed.append(e)

    t = threading.Thread(target=consumer)
    t.start()
    busy = 0
    try:
        for _ in range(times):
            for k in range(3):
                while not failed:
                    try:
                        out.garble(hdr[k], *step_args(ref, k))
                        break
                    except engine.EngineError as e:
                        assert e.code == engine.GC_E_BUSY
                        busy += 1
        out.flush()
    finally:
        done.set()
        t.join()
    assert failed == []
    for s in range(S):
        assert b"".join(w[s].tobytes() for w in got) == expected_stream(ref, s, hdr, times), "session %d" % s
    sealed, nbytes, grown, nbusy = out.stats()
    assert sealed == len(got) and nbytes == times * len(expected_stream(ref, 0, hdr)) and grown == 0 and nbusy == busy
    check_store(g.sb, ref)
    out.close(), g.close()
    ctx.close()


# ---- the evaluator from host memory -------------------------------------------------------------------------------------------

def one_window(ctx, ref, S):
    """the whole program in ONE window: (garbler, out handle, base address, stride, [offset of step k's block], header list)"""
    g = Garbler(ctx, ref, S)
    hdr = headers()
    out = g.sb.out(20000, 2)
    offs, at = [], 0
    for k in range(3):
        offs.append(at + HEADER)
        at += out.garble(hdr[k], *step_args(ref, k))
    out.flush()
    base, stride, n = out.next()
    assert n == at
    return g, out, base, stride, offs


def block_args(ref, k):
    c, in_, out_ = ref["steps"][k]
    return c.NumGates, c.NumWires, max(max(in_), max(out_)) + 1


def evaluator(ctx, ref, g, S):
    se = engine.StreamEvalBatch(ctx, S, g.d_keys, KEYLEN)
    se.set_wires(ref["prim"], engine.DeviceBuffer(ctx, data=labels_of(ref, ref["prim"], ref["bits"])))
    return se


def check_outputs(se, ref, sessions):
    for o in ref["outs"]:
        got = se.get(o)
        for s in sessions:
            assert (int(got[s]["d0"]), int(got[s]["d1"])) == ref["ev"][o][s], (o, s)


@pytest.mark.parametrize("S,ref_session", [(5, 0), (67, 41)])
def test_evaluator_reads_the_garblers_windows_in_place(S, ref_session):
    ctx = engine.Context(0)
    ref = reference(S, 0, KEYLEN)
    g, out, base, stride, offs = one_window(ctx, ref, S)
    assert engine.lib().gc_host_is_pinned(base) == 1
    se = evaluator(ctx, ref, g, S)
    assert (se.bad() == 0).all()  # before any block
    for k in range(3):
        n = len(ref["streams"][0][k])
        assert se.circuit_host(*block_args(ref, k), base + offs[k], stride, n, ref_session) == n
    se.uploads_wait()
    assert (se.bad() == 0).all()
    check_outputs(se, ref, range(S))
    with pytest.raises(engine.EngineError) as err:
        se.circuit_host(*block_args(ref, 0), base + offs[0], stride, len(ref["streams"][0][0]), S)  # no such session
    assert err.value.code == engine.GC_E_ARG
    out.release()
    se.close(), out.close(), g.close()
    ctx.close()


def test_evaluator_reads_pageable_blocks_and_keeps_its_verdict():
    """a pageable copy at an odd stride; one structure byte of session 1 inverted in the second block: bad[1] == 1 after the
    third block too, and every other session stays exact"""
    S = 5
    ctx = engine.Context(0)
    ref = reference(S, 0, KEYLEN)
    g, out, base, stride, offs = one_window(ctx, ref, S)
    view = np.frombuffer((engine.C.c_uint8 * (S * stride)).from_address(base), np.uint8).reshape(S, stride)
    odd = stride + 13
    blocks = np.zeros((S, odd), np.uint8)
    blocks[:, :stride] = view
    out.release()
    assert engine.lib().gc_host_is_pinned(blocks.ctypes.data) == 0
    gates, err = hf.parse(ref["streams"][0][1], ref["steps"][1][0].NumGates)
    assert err is None
    tam = blocks.copy()
    tam[1, offs[1] + gates[4][5][0]] ^= 0xff  # a wire id byte of the fifth gate
    for data, bad1 in ((blocks, 0), (tam, 1)):
        se = evaluator(ctx, ref, g, S)
        for k in range(3):
            n = len(ref["streams"][0][k])
            buf = data.copy()
            assert se.circuit_host(*block_args(ref, k), buf.ctypes.data + offs[k], odd, n, 0 if k != 1 else 3) == n
            buf[:] = 0xEE  # the call has returned: the pageable bytes may be reused
            if k >= 1:
                bad = se.bad()
                assert bad[1] == bad1 and (np.delete(bad, 1) == 0).all(), (k, bad)
        check_outputs(se, ref, [s for s in range(S) if s != 1 or not bad1])
        se.close()
    out.close(), g.close()
    ctx.close()


def test_a_hostile_reference_block_keeps_the_parsers_refusal_codes():
    """one hostile_fuzz mutant per refusal code of parse_block (the full set runs in test_gpu_stream_batch_hostile.py): the host
    form answers what the device form answers for the same bytes, and the valid block still evaluates afterwards"""
    S = 5
    ctx = engine.Context(0)
    ref = reference(S, 0, KEYLEN)
    g, out, base, stride, offs = one_window(ctx, ref, S)
    view = np.frombuffer((engine.C.c_uint8 * (S * stride)).from_address(base), np.uint8).reshape(S, stride)
    ng, ntmp, nw = block_args(ref, 0)
    n = len(ref["streams"][0][0])
    valid = np.ascontiguousarray(view[:, offs[0]: offs[0] + n])
    out.release()
    probe, se = evaluator(ctx, ref, g, S), evaluator(ctx, ref, g, S)
    d_bad = engine.DeviceBuffer(ctx, shape=S, dtype=np.uint32)
    rng = np.random.default_rng(181)
    seen = {}
    for _ in range(200):
        if len(seen) == 3:
            break
        mut, mng, what = hf.mutate(rng, valid[0].tobytes(), ng)
        width = max(4, (len(mut) + 3) & ~3)
        blocks = np.zeros((S, width), np.uint8)
        blocks[:, : len(mut)] = np.frombuffer(mut, np.uint8)
        try:
            probe.circuit(mng, ntmp, nw, mut, engine.DeviceBuffer(ctx, data=blocks), width, d_bad)
            continue
        except engine.EngineError as e:
            code = e.code
        if code in seen or "gc_batch_keyed_supported" in engine.lib().gc_last_error().decode():
            continue
        seen[code] = what
        with pytest.raises(engine.EngineError) as err:
            se.circuit_host(mng, ntmp, nw, blocks, width, len(mut), 0)
        assert err.value.code == code, what
    assert sorted(seen) == sorted([engine.GC_E_GATE, engine.GC_E_ROWS, engine.GC_E_ARG]), seen
    assert se.circuit_host(ng, ntmp, nw, valid, n, n, 2) == n
    assert (se.bad() == 0).all()
    for o in ref["steps"][0][2]:
        got = se.get(o)
        for s in range(S):
            assert (int(got[s]["d0"]), int(got[s]["d1"])) == ref["ev"][o][s], (o, s)
    probe.close(), se.close(), out.close(), g.close()
    ctx.close()


# ---- end to end -----------------------------------------------------------------------------------------------------------------

def test_one_program_end_to_end_for_67_sessions():
    """select -> set_wires; windows -> circuit_host; output labels -> decode: plain_program's bits for every session"""
    S = 67
    ctx = engine.Context(0)
    ref = reference(S, 0, KEYLEN)
    g = Garbler(ctx, ref, S)
    prim, outs, hdr = ref["prim"], ref["outs"], headers()
    d_labels = engine.DeviceBuffer(ctx, shape=(S, len(prim)), dtype=LABEL)
    g.sb.select_labels(prim, engine.DeviceBuffer(ctx, data=mixed(ref["bits"])), d_labels)
    se = engine.StreamEvalBatch(ctx, S, g.d_keys, KEYLEN)
    se.set_wires(prim, d_labels)
    out = g.sb.out(14078, 3)
    k_eval = 0

    def evaluate_windows():
        nonlocal k_eval
        while True:
            w = out.next()
            if w is None:
                return
            base, stride, n = w
            at = 0
            while at < n:  # the caller reads the framing: here it knows the steps
                blk = len(ref["streams"][0][k_eval])
                assert se.circuit_host(*block_args(ref, k_eval), base + at + HEADER, stride, blk, k_eval) == blk
                at += HEADER + blk
                k_eval += 1
            se.uploads_wait()
            out.release()

    for k in range(3):
        while True:
            try:
                out.garble(hdr[k], *step_args(ref, k))
                break
            except engine.EngineError as e:
                assert e.code == engine.GC_E_BUSY
                evaluate_windows()
    out.flush()
    evaluate_windows()
    assert k_eval == 3 and (se.bad() == 0).all()
    lab = np.stack([se.get(o) for o in outs], axis=1)
    bits, bad = g.sb.decode(outs, lab)
    assert (bad == 0).all()
    assert (bits == np.array([[ref["vals"][s][o] for o in outs] for s in range(S)], np.uint8)).all()
    se.close(), out.close(), g.close()
    ctx.close()
