"""The intake of a session-batched evaluator (gc_stream_eval_batch_in_*): the S byte streams of the program of
tests/stream_batch_intake_cases.py, garbled through gc_stream_batch_out_* behind their 20-byte OpCircuit headers, fed in chunks
that respect no step boundary.  After every run the store must be what one gc_stream_eval_batch_circuit_host call per step
leaves, and session 0's what the oracle's StreamEvaluator computes from the same bytes.  No input here provokes a device
fault: every hostile one is refused on the host or only counted on the device."""
import struct

import numpy as np
import pytest

from mpc_amd import engine
from mpc_amd.circuit import LABEL
from tests import hostile_fuzz as hf
from tests import stream_batch_intake_cases as ic

pytestmark = pytest.mark.gpu

KEYLEN = 32
SESSIONS = (3, 67)
_made = {}


def garbled(S):
    """once per S: (the garbler's windows [(u8 [S, len])], the streams u8 [S, total] = their concatenation, the store u32-pairs
    LABEL [S, wires] that the per-step route leaves).  The windows are 2 000 bytes, so most hold several steps and none a
    whole number of the chunks below."""
    if S in _made:
        return _made[S]
    ref = ic.reference(S, KEYLEN)
    ctx = engine.Context(0)
    d_keys, d_rnd = engine.DeviceBuffer(ctx, data=ref["keys"]), engine.DeviceBuffer(ctx, data=ref["rnd"])
    sb = engine.StreamBatch(ctx, S, d_keys, KEYLEN, d_rnd, ref["prim"])
    out, windows = sb.out(2000, 2), []

    def drain():
        while True:
            v = out.next_view()
            if v is None:
                return
            windows.append(v.copy())
            out.release()

    for k, (c, in_, out_) in enumerate(ref["steps"]):
        while True:
            try:
                out.garble(ref["hdr"][k], c.Gates, c.NumWires, in_, out_)
                break
            except engine.EngineError as e:
                assert e.code == engine.GC_E_BUSY
                drain()
    out.flush()
    drain()
    streams = np.concatenate(windows, axis=1)
    assert (streams == ref["framed"]).all() and len(windows) >= 3  # the garbler's bytes are the oracle's
    # the per-step route, the header read on the host from session 0
    se = evaluator(ctx, ref, d_keys, S)
    at = 0
    while at < streams.shape[1]:
        op, _, ngates, ntmp, nwires = struct.unpack(">5I", streams[0, at: at + ic.HEADER].tobytes())
        assert op == ic.OP_CIRCUIT
        rest = np.ascontiguousarray(streams[:, at + ic.HEADER:])
        at += ic.HEADER + se.circuit_host(ngates, ntmp, nwires, rest, rest.shape[1], rest.shape[1], 0)
    assert (se.bad() == 0).all()
    store = se.return_labels(ref["every"])
    for j, w in enumerate(ref["every"]):
        assert [(int(x["d0"]), int(x["d1"])) for x in store[:, j]] == ref["ev"][w], w
    se.close(), out.close(), sb.close(), d_keys.close(), d_rnd.close()
    ctx.close()
    _made[S] = (windows, streams, store)
    return _made[S]


def evaluator(ctx, ref, d_keys, S):
    se = engine.StreamEvalBatch(ctx, S, d_keys, KEYLEN)
    se.set_wires(ref["prim"], engine.DeviceBuffer(ctx, data=ref["inlab"]))
    return se


class Eval:
    def __init__(self, S, ref_session=0, cap=1 << 20):
        self.ref, self.S = ic.reference(S, KEYLEN), S
        self.ctx = engine.Context(0)
        self.d_keys = engine.DeviceBuffer(self.ctx, data=self.ref["keys"])
        self.se = evaluator(self.ctx, self.ref, self.d_keys, S)
        self.it = self.se.intake(ref_session, cap)

    def feed_all(self, chunks):
        for c in chunks:
            assert self.it.feed(c) == (c.shape[1], ic.OP_CIRCUIT)

    def store(self):
        return self.se.return_labels(self.ref["every"])

    def close(self):
        self.it.close(), self.se.close(), self.d_keys.close()
        self.ctx.close()


def fixed(streams, n):
    return [streams[:, at: at + n] for at in range(0, streams.shape[1], n)]


@pytest.mark.parametrize("S", SESSIONS)
@pytest.mark.parametrize("chunking", ["whole", "windows", 1, 7, 4096])
def test_any_chunking_leaves_the_store_of_the_per_step_route(chunking, S):
    windows, streams, store = garbled(S)
    total = streams.shape[1]
    chunks = [streams] if chunking == "whole" else windows if chunking == "windows" else fixed(streams, chunking)
    ev = Eval(S)
    ev.feed_all(chunks)
    assert (ev.se.bad() == 0).all()
    assert (ev.store() == store).all()
    steps, nbytes, uploads, carried = ev.it.stats()
    assert (steps, nbytes, uploads) == (ic.NSTEPS, total, len(chunks))
    if chunking in ("whole", "windows"):
        assert carried == 0  # the garbler never splits a step over two windows
    else:
        offs = ev.ref["offs"]
        ends = range(chunking, total, chunking)
        assert carried == sum(e - max(o for o in offs if o <= e) for e in ends)
    ev.close()


@pytest.mark.parametrize("S", SESSIONS)
def test_a_cut_at_every_byte_of_the_first_two_messages(S):
    """message 0 has 16-bit ids and rows of every kind, message 1 a gate with 32-bit ids: the cut falls on each of the 20 header
    bytes, on op bytes, inside ids of both widths, inside rows and exactly on both message ends.  One handle serves every cut:
    the outputs of the two steps are zeroed in between (neither step reads what it writes)."""
    _, streams, store = garbled(S)
    ev = Eval(S)
    ref = ev.ref
    end = ref["offs"][2]
    two = np.ascontiguousarray(streams[:, :end])
    outs = ref["steps"][0][2] + ref["steps"][1][2]
    cols = [ref["every"].index(w) for w in outs]
    d_zero = engine.DeviceBuffer(ev.ctx, shape=(S, len(outs)), dtype=LABEL, zero=True)
    parsed = [hf.parse(ref["streams"][0][k], ref["steps"][k][0].NumGates)[0] for k in (0, 1)]
    assert {q[3] for q in parsed[0]} == {True} and False in {q[3] for q in parsed[1]}
    for cut in range(1, end + 1):
        ev.se.set_wires(outs, d_zero)
        assert ev.it.feed(two[:, :cut]) == (cut, ic.OP_CIRCUIT)
        if cut < end:
            assert ev.it.feed(two[:, cut:]) == (end - cut, ic.OP_CIRCUIT)
        got = ev.se.return_labels(outs)
        assert (got == store[:, cols]).all(), cut
    assert ev.it.stats()[:2] == (2 * end, end * end) and (ev.se.bad() == 0).all()
    ev.close()


@pytest.mark.parametrize("ref_session,pinned,pad", [(0, False, 13), (-1, False, 0), (-1, True, 24), (0, True, 0)])
def test_reference_session_memory_kind_and_stride(ref_session, pinned, pad):
    S = 67
    windows, streams, store = garbled(S)
    ev = Eval(S, ref_session % S)
    keep = []
    for w in windows:
        n = w.shape[1]
        if pinned:
            p = engine.PinnedArray((S, n + pad), np.uint8)
            keep.append(p)
            a = p.a
        else:
            a = np.zeros((S, n + pad), np.uint8)
        a[:] = 0xEE
        a[:, :n] = w
        assert engine.lib().gc_host_is_pinned(a.ctypes.data) == int(pinned)
        assert ev.it.feed(a.ctypes.data, n + pad, n) == (n, ic.OP_CIRCUIT)
        if not pinned:
            a[:] = 0x77  # the call has returned: pageable bytes may be reused
    ev.se.uploads_wait()
    assert (ev.se.bad() == 0).all() and (ev.store() == store).all()
    ev.close()
    for p in keep:
        p.close()


@pytest.mark.parametrize("S", SESSIONS)
def test_the_feed_stops_in_front_of_an_op_return(S):
    _, streams, store = garbled(S)
    total = streams.shape[1]
    ref = ic.reference(S, KEYLEN)
    ids = ref["outs"][:9]
    ret = np.frombuffer(struct.pack(">I", ic.OP_RETURN) + struct.pack(">%dI" % len(ids), *ids), np.uint8)
    second = np.ascontiguousarray(streams[:, : ref["offs"][1]])  # a fresh OpCircuit behind it: step 0 once more
    buf = np.concatenate([streams, np.tile(ret, (S, 1)), second], axis=1)
    for cut in (None, total + 4, total + 11, total + 2, total + 3, total + 1):
        ev = Eval(S)
        if cut is None:     # the word and its ids in the same chunk as the last step
            assert ev.it.feed(buf[:, : total + len(ret)]) == (total, ic.OP_RETURN)
        elif cut >= total + 4:  # the word in this chunk, (some of) its ids in the next
            assert ev.it.feed(buf[:, :cut]) == (total, ic.OP_RETURN)
        else:               # the word itself across two chunks: its first bytes are taken, the next feed reports it
            assert ev.it.feed(buf[:, :cut]) == (cut, ic.OP_CIRCUIT)
            assert ev.it.feed(buf[:, cut: total + len(ret)]) == (0, ic.OP_RETURN)
            assert ev.it.word_bytes_taken() == cut - total
        assert ev.it.stats()[:2] == (ic.NSTEPS, total)
        assert (buf[:, total:total + len(ret)] == ret).all()  # the bytes behind the stop are untouched
        # the caller reads the ids itself and answers with the labels
        got_ids = struct.unpack(">%dI" % len(ids), buf[0, total + 4: total + len(ret)].tobytes())
        cols = [ref["every"].index(w) for w in got_ids]
        assert (ev.se.return_labels(got_ids) == store[:, cols]).all()
        assert ev.it.feed(buf[:, total + len(ret):]) == (second.shape[1], ic.OP_CIRCUIT)
        assert ev.it.stats()[:2] == (ic.NSTEPS + 1, total + second.shape[1]) and (ev.se.bad() == 0).all()
        ev.close()


def test_one_fault_per_session_marks_that_session_alone():
    S = 67
    _, streams, store = garbled(S)
    ref = ic.reference(S, KEYLEN)
    offs = ref["offs"]
    tam = streams.copy()
    gates5, _ = hf.parse(ref["streams"][0][5], ref["steps"][5][0].NumGates)
    faults = {5: offs[2] + 4 + 3,                         # step
              9: offs[3] + 8 + 2,                         # numGates
              13: offs[4] + 16 + 1,                       # numWires
              21: offs[5] + ic.HEADER + gates5[6][5][1]}  # an id byte of the seventh gate
    for s, at in faults.items():
        tam[s, at] ^= 0x5A
    rows6 = [q for q in hf.parse(ref["streams"][0][6], ref["steps"][6][0].NumGates)[0] if q[7]]
    for q in rows6:  # a byte of every row of the seventh step: data, not structure (a row is read or not by the active labels)
        for j in range(q[7]):
            tam[30, offs[6] + ic.HEADER + q[6] + 16 * j + 5] ^= 0x01
    for chunks in ([tam], fixed(tam, 1000)):
        ev = Eval(S, ref_session=1)
        ev.feed_all(chunks)
        bad = ev.se.bad()
        assert {s: int(bad[s]) for s in np.nonzero(bad)[0]} == {s: 1 for s in faults}
        got = ev.store()
        clean = [s for s in range(S) if s not in faults and s != 30]
        assert (got[clean] == store[clean]).all()
        want = ic.oracle_eval(ref, 30, tam[30])
        assert [(int(x["d0"]), int(x["d1"])) for x in got[30]] == [want[w] for w in ref["every"]]
        assert (got[30] != store[30]).any()
        ev.close()


def test_a_lying_reference_session_is_refused_on_the_host():
    S = 3
    _, streams, store = garbled(S)
    ref = ic.reference(S, KEYLEN)
    offs = ref["offs"]
    ev = Eval(S, cap=4096)
    # numGates = 0xffffffff in every session's fourth header: refused when the header is read, nothing sized by it
    lie = streams.copy()
    lie[:, offs[3] + 8: offs[3] + 12] = 0xFF
    ev.feed_all([np.ascontiguousarray(streams[:, : offs[3]])])
    cache, stats = ev.se.cache_stats(), ev.it.stats()
    with pytest.raises(engine.EngineError) as err:
        ev.it.feed(np.ascontiguousarray(lie[:, offs[3]:]))
    assert err.value.code == engine.GC_E_ROWS and ev.it.taken == 0
    assert ev.se.cache_stats() == cache and ev.it.stats()[:2] == stats[:2]
    # ... also behind messages of the same chunk, which stay evaluated
    ev2 = Eval(S, cap=4096)
    with pytest.raises(engine.EngineError) as err:
        ev2.it.feed(lie)
    assert err.value.code == engine.GC_E_ROWS and ev2.it.taken == offs[3] and ev2.it.stats()[:2] == (3, offs[3])
    done = [ref["every"].index(w) for k in range(3) for w in ref["steps"][k][2]]
    assert (ev2.store()[:, done] == store[:, done]).all()
    # the handle goes on with the correct rest of the stream
    ev2.feed_all([np.ascontiguousarray(streams[:, offs[3]:])])
    assert (ev2.store() == store).all() and (ev2.se.bad() == 0).all()
    ev2.close()
    # a header that claims 700 gates (3 520 bytes at the least: under the cap) in front of valid gates that never end:
    # GC_E_ROWS when the kept bytes would pass the cap of 4 096, and not before
    gate = bytes([0x10]) + struct.pack(">3H", ref["prim"][3], ref["prim"][4], 600)  # XOR, 16-bit ids, into global 600
    msg = np.frombuffer(struct.pack(">5I", ic.OP_CIRCUIT, 0, 700, 4, 1000) + gate * 600, np.uint8)
    assert len(msg) == 4220
    endless = np.tile(msg, (S, 1))
    held = 0
    for at in range(0, 4000, 1000):
        assert ev.it.feed(np.ascontiguousarray(endless[:, at: at + 1000])) == (1000, ic.OP_CIRCUIT)
        held += 1000
    before = ev.it.stats()
    with pytest.raises(engine.EngineError) as err:
        ev.it.feed(np.ascontiguousarray(endless[:, 4000:4100]))
    assert err.value.code == engine.GC_E_ROWS and ev.it.taken == 0
    assert ev.it.stats()[:2] == before[:2] and ev.se.cache_stats() == cache
    # ... and 1 000 gates cannot fit under it at all: refused with the header
    with pytest.raises(engine.EngineError) as err:
        ev.it.feed(np.tile(np.frombuffer(struct.pack(">5I", ic.OP_CIRCUIT, 0, 1000, 4, 1000), np.uint8), (S, 1)))
    assert err.value.code == engine.GC_E_ROWS
    # an invalid gate operation in the fifth message: GC_E_GATE, the fourth is evaluated
    bad_op = streams.copy()
    bad_op[:, offs[4] + ic.HEADER] = 0x17
    with pytest.raises(engine.EngineError) as err:
        ev.it.feed(np.ascontiguousarray(bad_op[:, offs[3]:]))
    assert err.value.code == engine.GC_E_GATE and ev.it.taken == offs[4] - offs[3]
    assert ev.it.stats()[0] == 4
    ev.feed_all([np.ascontiguousarray(streams[:, offs[4]:])])
    assert (ev.store() == store).all() and (ev.se.bad() == 0).all()
    ev.close()
