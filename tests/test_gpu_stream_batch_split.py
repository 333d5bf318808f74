"""The split form of the stream-batch window handle (gc_stream_batch_out_create_split) and the path-2 fallback of
the two handles, against the oracle values of tests/test_gpu_stream_batch.reference(): a step is cut over the windows by
k_sb_serialise_range, every window but a flushed one leaves exactly full, none grows, and for every session the windows in
order are byte for byte `prefix | step` over the steps.  Every session is compared in every test, and every split test asserts
that a step was in fact cut (split_steps > 0).  The ring rule is tests/test_stream_batch_split_windows.SplitModel."""
import threading
import time

import numpy as np
import pytest

import oracle
from mpc_amd import engine
from mpc_amd.circuit import LABEL
from tests import hostile_fuzz as hf
from tests import keyed_geometry as kg
from tests import stream_batch_cases as sc
from tests import stream_batch_intake_cases as ic
from tests.test_gpu_stream_batch import check_store, reference, rnd_streams
from tests.test_gpu_stream_batch_io import Garbler, drain_one, expected_stream, headers, labels_of, step_args
from tests.test_stream_batch_split_windows import HEADER, SplitModel, smallest_ring

pytestmark = pytest.mark.gpu

KEYLEN = 32


def up16(n):
    return (n + 15) // 16 * 16


def run_split(out, model, steps, got):
    """steps: [(prefix, (gates, nwires, in_, out_), bytes of the step without the prefix)] through the handle and the model in
    step, with a consumer that takes one window whenever the garbler is told BUSY; then flush and drain"""
    for prefix, args, nbytes in steps:
        n = len(prefix) + nbytes
        while True:
            line = model.event("s %d" % n)
            try:
                assert out.garble(prefix, *args) == n
                assert line.startswith("s ok"), line
                break
            except engine.EngineError as e:
                assert e.code == engine.GC_E_BUSY and line.startswith("s busy"), (e.code, line)
                assert drain_one(out, model, got)
    out.flush()
    model.event("f")
    while drain_one(out, model, got):
        pass


def program_steps(ref, hdr):
    return [(hdr[k], step_args(ref, k), len(ref["streams"][0][k])) for k in range(3)]


def check_windows(out, model, got, want_of_session, S):
    """the bytes of every session, the window lengths, and both sets of counters against the model"""
    for s in range(S):
        assert b"".join(w[s].tobytes() for w in got) == want_of_session(s), "session %d" % s
    assert all(w.shape[1] == model.c for w in got[:-1]) and 0 < got[-1].shape[1] <= model.c
    assert out.stats() == (model.n_sealed, model.total, 0, model.busy) and model.n_sealed == len(got)
    assert out.split_stats() == (model.split_steps, model.segments) and model.split_steps > 0


# ---- 1. bytes -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [5, 67])
@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("window_bytes", [4096, 5000, 1000])
def test_split_windows_hold_header_and_oracle_bytes(window_bytes, extra, S):
    ctx = engine.Context(0)
    ref = reference(S, 0, KEYLEN)
    g = Garbler(ctx, ref, S)
    hdr, got = headers(), []
    nwindows = smallest_ring(window_bytes, HEADER + max(len(x) for x in ref["streams"][0])) + extra
    out, model = g.sb.out(window_bytes, nwindows, split=True), SplitModel(window_bytes, nwindows)
    assert model.c == {4096: 4096, 5000: 5008, 1000: 1008}[window_bytes]
    run_split(out, model, program_steps(ref, hdr), got)
    check_windows(out, model, got, lambda s: expected_stream(ref, s, hdr), S)
    if window_bytes == 1000:
        assert model.segments >= 3 + 12  # the middle step alone lies in 12 windows or more
    check_store(g.sb, ref)
    with pytest.raises(engine.EngineError) as err:
        out.release()
    assert err.value.code == engine.GC_E_ARG
    out.close(), g.close()
    ctx.close()


def test_split_stats_of_an_unsplit_handle_are_zeros():
    S = 5
    ctx = engine.Context(0)
    ref = reference(S, 0, KEYLEN)
    g = Garbler(ctx, ref, S)
    out, hdr = g.sb.out(4096, 2), headers()
    out.garble(hdr[0], *step_args(ref, 0))
    out.garble(hdr[1], *step_args(ref, 1))
    assert out.split_stats() == (0, 0) and out.stats()[2] == 1  # the unsplit handle grew instead
    out.close(), g.close()
    ctx.close()


# ---- 2. where the cut falls -----------------------------------------------------------------------------------------------------

def test_the_first_cut_at_every_residue_mod_16_and_inside_the_prefix():
    """a leading step with a prefix of 0 .. 15 bytes moves the first cut of the second step through every residue mod 16; with
    windows of 2 576 bytes and a leading prefix of 20, the window has 4 bytes left: the cut lies inside the second step's prefix"""
    S = 3
    ctx = engine.Context(0)
    ref = reference(S, 0, KEYLEN)
    g = Garbler(ctx, ref, S)
    hdr = headers()
    n0 = len(ref["streams"][0][0])
    residues = set()
    for window_bytes, lead in [(4096, p) for p in range(16)] + [(2576, 20)]:
        pre = [hdr[0][:lead], hdr[1], hdr[2]]
        nwindows = smallest_ring(window_bytes, HEADER + len(ref["streams"][0][1]))
        out, model, got = g.sb.out(window_bytes, nwindows, split=True), SplitModel(window_bytes, nwindows), []
        cut = model.c - (lead + n0)  # the byte of `prefix | step 2` that is the first of the next window
        assert 0 < cut
        if window_bytes == 4096:
            residues.add(cut % 16)
        else:
            assert cut < HEADER
        run_split(out, model, [(pre[k], step_args(ref, k), len(ref["streams"][0][k])) for k in range(3)], got)
        check_windows(out, model, got, lambda s: b"".join(pre[k] + ref["streams"][s][k] for k in range(3)), S)
        out.close()
    assert residues == set(range(16))
    check_store(g.sb, ref)
    g.close()
    ctx.close()


def one_step_with_the_cut_at(g, ref, x):
    """the one step of a geometry case through a split handle whose FIRST cut is in front of byte x of the step: windows of x
    rounded up to 16 and a prefix that fills the difference.  Returns the windows and the prefix."""
    cap = up16(x)
    prefix = bytes(range(0x40, 0x40 + cap - x))
    n = len(ref["streams"][0][0])
    nwindows = smallest_ring(cap, len(prefix) + n)
    out, model, got = g.sb.out(cap, nwindows, split=True), SplitModel(cap, nwindows), []
    assert model.c == cap and len(prefix) + x == cap
    run_split(out, model, [(prefix, step_args(ref, 0), n)], got)
    check_windows(out, model, got, lambda s: prefix + ref["streams"][s][0], g.S)
    out.close()
    return got, prefix


@pytest.mark.parametrize("name", ["straddle", "straddle_long", "tail2x"])
def test_the_cut_around_a_row_that_lies_across_a_piece_boundary(name):
    """the cut at the row's first byte, one behind it, at its byte 15 and one behind its end — for the first, a middle and the
    last row of the case that straddles a 4 096-byte boundary of the step"""
    S = 3
    ctx = engine.Context(0)
    ref = sc.reference(name, S)
    g = Garbler(ctx, ref, S)
    c = ref["steps"][0][0]
    n = len(ref["streams"][0][0])
    parsed, err = hf.parse(ref["streams"][0][0], c.NumGates)
    assert err is None
    strad = sc.straddlers(parsed, n)
    assert strad and sc.GEOMETRY[name]["straddles"]
    rows = sorted({strad[0], strad[len(strad) // 2], strad[-1]})
    for off, boundary in rows:
        assert off < boundary < off + 16
        for x in (off, off + 1, off + 15, off + 16):
            one_step_with_the_cut_at(g, ref, x)
    check_store(g.sb, ref)
    g.close()
    ctx.close()


def test_the_cut_inside_a_four_byte_wire_id():
    S = 3
    ctx = engine.Context(0)
    ref = sc.reference("straddle_long", S)
    g = Garbler(ctx, ref, S)
    parsed, err = hf.parse(ref["streams"][0][0], ref["steps"][0][0].NumGates)
    assert err is None
    wide = [q for q in parsed if not q[3] and q[0] > 2 * sc.PIECE]
    assert wide
    q = wide[len(wide) // 2]
    for x in (q[5][0] + 1, q[5][1] + 2, q[5][-1] + 3):  # inside the first, the second and the last id of the gate
        got, prefix = one_step_with_the_cut_at(g, ref, x)
        assert got[0].shape[1] == len(prefix) + x
    g.close()
    ctx.close()


# ---- 3. busy and too large ------------------------------------------------------------------------------------------------------

def test_busy_with_k_minus_1_windows_free_and_a_step_that_is_too_large():
    S, cap, nwindows = 5, 4096, 4
    ctx = engine.Context(0)
    ref = reference(S, 0, KEYLEN)
    g = Garbler(ctx, ref, S)
    out, hdr = g.sb.out(cap, nwindows, split=True), headers()
    with pytest.raises(engine.EngineError) as err:
        g.sb.out(cap, 1, split=True)
    assert err.value.code == engine.GC_E_ARG
    # too large: (nwindows - 1) * cap + 1 bytes with the prefix; refused whatever is free, with both numbers in the text
    big, in_, out_ = sc.build([], (nwindows - 1) * cap + 1 - HEADER)
    assert engine.stream_batch_step_bytes(big.Gates, big.NumWires, in_, out_) + HEADER == 12289
    before = [g.sb.get(w).copy() for w in in_ + out_]
    with pytest.raises(engine.EngineError) as err:
        out.garble(hdr[0], big.Gates, big.NumWires, in_, out_)
    assert err.value.code == engine.GC_E_ARG
    text = engine.lib().gc_last_error().decode()
    assert "12289" in text and "12288" in text and "4096" in text, text
    assert out.stats() == (0, 0, 0, 0) and out.split_stats() == (0, 0) and g.sb.cache_stats()[2] == 0
    for w, want in zip(in_ + out_, before):
        assert (g.sb.get(w) == want).all(), w
    # ... and the handle stays usable: steps 1 and 2 lie in windows 0 .. 3 (2 572 + 11 546 = 3 * 4 096 + 1 830)
    n = [HEADER + len(ref["streams"][0][k]) for k in range(3)]
    assert out.garble(hdr[0], *step_args(ref, 0)) == n[0]
    assert out.garble(hdr[1], *step_args(ref, 1)) == n[1]
    assert out.stats() == (3, n[0] + n[1], 0, 0) and out.split_stats() == (1, 5)
    # step 3 needs window 3, which fills, and window 0, which is sealed and then handed out: k - 1 = 1 window free
    step3_outs = ref["steps"][2][2]
    got = []
    for rep in range(3):
        if rep == 1:
            first = out.next_view()
            assert first.shape == (S, cap)
        with pytest.raises(engine.EngineError) as err:
            out.garble(hdr[2], *step_args(ref, 2))
        assert err.value.code == engine.GC_E_BUSY and "window" in str(err.value)
        assert out.stats() == (3, n[0] + n[1], 0, rep + 1) and out.split_stats() == (1, 5)
    done = [o for k in range(2) for o in ref["steps"][k][2]]
    for w in ref["prim"][::9] + done:
        assert (g.sb.get(w) == ref["wires"][w]).all(), w
    for o in step3_outs:
        assert (g.sb.get(o)["l0"] == np.zeros(S, LABEL)).all(), o  # never set
    got.append(first.copy())
    out.release()
    assert out.garble(hdr[2], *step_args(ref, 2)) == n[2]  # the repeated call after one release is exact
    assert out.split_stats() == (2, 7)
    out.flush()
    while True:
        v = out.next_view()
        if v is None:
            break
        got.append(v.copy())
        out.release()
    for s in range(S):
        assert b"".join(w[s].tobytes() for w in got) == expected_stream(ref, s, hdr), "session %d" % s
    assert [w.shape[1] for w in got] == [cap] * 4 + [sum(n) - 4 * cap]
    assert out.stats() == (5, sum(n), 0, 3)
    check_store(g.sb, ref)
    out.close(), g.close()
    ctx.close()


# ---- 4. end to end --------------------------------------------------------------------------------------------------------------

def test_split_windows_into_the_intake_end_to_end_for_67_sessions():
    """select -> set_wires; split windows of 1 000 bytes, handed as they come to the evaluator's intake; return_labels ->
    decode: the plaintext of the reference for every session"""
    S, window_bytes = 67, 1000
    ctx = engine.Context(0)
    ref = reference(S, 0, KEYLEN)
    g = Garbler(ctx, ref, S)
    prim, outs = ref["prim"], ref["outs"]
    hdr = [ic.header(k, c, in_, out_) for k, (c, in_, out_) in enumerate(ref["steps"])]
    se = engine.StreamEvalBatch(ctx, S, g.d_keys, KEYLEN)
    se.set_wires(prim, engine.DeviceBuffer(ctx, data=g.sb.select_labels(prim, ref["bits"])))
    it = se.intake(0, 1 << 20)
    nwindows = smallest_ring(window_bytes, HEADER + max(len(x) for x in ref["streams"][0]))
    out = g.sb.out(window_bytes, nwindows, split=True)
    lens = []

    def feed_windows():
        while True:
            w = out.next()
            if w is None:
                return
            base, stride, n = w
            assert it.feed(base, stride, n) == (n, ic.OP_CIRCUIT)
            lens.append(n)
            se.uploads_wait()  # (the window is read by DMA: it goes back to the ring when the upload has left)
            out.release()

    for k in range(3):
        while True:
            try:
                out.garble(hdr[k], *step_args(ref, k))
                break
            except engine.EngineError as e:
                assert e.code == engine.GC_E_BUSY
                feed_windows()
    out.flush()
    feed_windows()
    total = sum(HEADER + len(x) for x in ref["streams"][0])
    assert sum(lens) == total and all(n == 1008 for n in lens[:-1])  # no window was sealed short before the last
    assert out.split_stats()[0] == 3 and it.stats()[:2] == (3, total)
    assert (se.bad() == 0).all()
    bits, bad = g.sb.decode(outs, se.return_labels(outs))
    assert (bad == 0).all()
    assert (bits == np.array([[ref["vals"][s][o] for o in outs] for s in range(S)], np.uint8)).all()
    it.close(), se.close(), out.close(), g.close()
    ctx.close()


# ---- 5. a consumer thread -------------------------------------------------------------------------------------------------------

def test_a_consumer_thread_takes_the_split_windows_of_twenty_passes():
    S, window_bytes, times, limit = 5, 5000, 20, 120.0
    ctx = engine.Context(0)
    ref = reference(S, 0, KEYLEN)
    g = Garbler(ctx, ref, S)
    out, hdr, got, done, failed = g.sb.out(window_bytes, 4, split=True), headers(), [], threading.Event(), []
    deadline = time.monotonic() + limit

    def consumer():
        try:
            while time.monotonic() < deadline:
                finished = done.is_set()  # (read before looking: a window sealed before `done` is still seen)
                v = out.next_view()
                if v is None:
                    if finished:
                        return
                    time.sleep(0)  # (yield: the garbling thread needs the interpreter)
                    continue
                got.append(v.copy())
                out.release()
            failed.append("the consumer ran out of time")
        except Exception as e:  # noqa: BLE001 (reported by the main thread)
            failed.append(e)

    t = threading.Thread(target=consumer)
    t.start()
    busy = 0
    try:
        for _ in range(times):
            for k in range(3):
                while not failed:
                    assert time.monotonic() < deadline, "the garbler ran out of time"
                    try:
                        out.garble(hdr[k], *step_args(ref, k))
                        break
                    except engine.EngineError as e:
                        assert e.code == engine.GC_E_BUSY
                        busy += 1
                        time.sleep(0)
        out.flush()
    finally:
        done.set()
        t.join(limit)
    assert not t.is_alive() and failed == []
    for s in range(S):
        assert b"".join(w[s].tobytes() for w in got) == expected_stream(ref, s, hdr, times), "session %d" % s
    sealed, nbytes, grown, nbusy = out.stats()
    total = times * len(expected_stream(ref, 0, hdr))
    assert sealed == len(got) == (total + 5007) // 5008 and nbytes == total and grown == 0 and nbusy == busy
    assert all(w.shape[1] == 5008 for w in got[:-1])
    assert out.split_stats()[0] >= times  # the middle step is larger than a window
    check_store(g.sb, ref)
    out.close(), g.close()
    ctx.close()


# ---- 6. the fallback ------------------------------------------------------------------------------------------------------------

def test_fallback_runs_the_step_the_key_table_keeps_out_on_path_2():
    """edge_over at 3 sessions: its wires are in LDS and the tile's key table does not fit.  With the fallback both handles run
    it on the keyed HBM-wire kernels: the garbler's bytes and store are the oracle's Stream, the evaluator's labels its
    StreamEvaluator's; the same step through a split handle lies in two windows with the same bytes.  (One global wire per
    circuit input: the evaluator's circuit is what it parses out of the block, its inputs the distinct wires read.)"""
    S = 3
    ctx = engine.Context(0)
    c = kg.build("edge_over")
    assert not kg.predict("edge_over", S).keyed
    prim, out_ = list(range(1000, 1000 + c.num_inputs)), [900]
    keys, rnd = kg.edge_keys("stream-batch/fallback", S, KEYLEN), rnd_streams("fallback", S, len(prim))
    bits = np.random.default_rng(6).integers(0, 2, (S, len(prim)), dtype=np.uint8)
    blocks, l0, active, inlab = [], [], [], np.zeros((S, len(prim)), LABEL)
    for s in range(S):
        og, oe = oracle.Stream(keys[s].tobytes(), rnd[s].tobytes(), prim), oracle.StreamEval(keys[s].tobytes())
        for j, w in enumerate(prim):
            wire = og.get(w)
            inlab[s, j] = wire["l1"] if bits[s, j] else wire["l0"]
            oe.set(w, inlab[s, j])
        blocks.append(og.garble(c.Gates, c.NumWires, prim, out_))
        assert oe.circuit(c.NumGates, c.NumWires, max(prim) + 1, blocks[-1]) == len(blocks[-1])
        l0.append(og.get(out_[0]))
        active.append(oe.get(out_[0]))
    n = len(blocks[0])
    stride = (n + 3) & ~3
    d_keys, d_rnd = engine.DeviceBuffer(ctx, data=keys), engine.DeviceBuffer(ctx, data=rnd)
    sb = engine.StreamBatch(ctx, S, d_keys, KEYLEN, d_rnd, prim)
    d_out = engine.DeviceBuffer(ctx, shape=S * stride)
    with pytest.raises(engine.EngineError) as err:  # the default refuses, and loads nothing
        sb.garble(c.Gates, c.NumWires, prim, out_, d_out, stride)
    assert err.value.code == engine.GC_E_ARG and "gc_batch_keyed_supported" in engine.lib().gc_last_error().decode()
    assert sb.cache_stats()[2] == 0
    sb.set_fallback(1)
    assert sb.garble(c.Gates, c.NumWires, prim, out_, d_out, stride) == n
    buf = d_out.numpy().reshape(S, stride)
    for s in range(S):
        assert buf[s, :n].tobytes() == blocks[s], "session %d" % s
        assert sb.get(out_[0])[s] == l0[s], "session %d" % s
    assert sb.cache_stats()[0] == 1 and sb.cache_stats()[2:] == (1, 0)
    # the evaluator: refused by default, exact with the fallback
    se = engine.StreamEvalBatch(ctx, S, d_keys, KEYLEN)
    se.set_wires(prim, engine.DeviceBuffer(ctx, data=inlab))
    d_bad = engine.DeviceBuffer(ctx, shape=S, dtype=np.uint32)
    with pytest.raises(engine.EngineError) as err:
        se.circuit(c.NumGates, c.NumWires, max(prim) + 1, blocks[1], d_out, stride, d_bad)
    assert err.value.code == engine.GC_E_ARG and "gc_batch_keyed_supported" in engine.lib().gc_last_error().decode()
    se.set_fallback(1)
    d_bad.zero(0xFF)
    assert se.circuit(c.NumGates, c.NumWires, max(prim) + 1, blocks[1], d_out, stride, d_bad) == n
    assert (d_bad.numpy() == 0).all() and se.cache_stats()[2] == 1
    got = se.get(out_[0])
    for s in range(S):
        assert (int(got[s]["d0"]), int(got[s]["d1"])) == active[s], "session %d" % s
    # the same step, cached, through a split handle: two windows, the same bytes
    window_bytes = up16((n + HEADER) // 2 + 1000)
    out, windows, hdr = sb.out(window_bytes, 3, split=True), [], headers(1)
    assert out.garble(hdr[0], c.Gates, c.NumWires, prim, out_) == HEADER + n
    out.flush()
    while True:
        v = out.next_view()
        if v is None:
            break
        windows.append(v.copy())
        out.release()
    assert [w.shape[1] for w in windows] == [window_bytes, HEADER + n - window_bytes]
    assert out.split_stats() == (1, 2) and out.stats()[2] == 0 and sb.cache_stats()[2] == 1
    for s in range(S):
        assert b"".join(w[s].tobytes() for w in windows) == hdr[0] + blocks[s], "session %d" % s
        assert sb.get(out_[0])[s] == l0[s], "session %d" % s
    out.close(), se.close(), sb.close()
    ctx.close()
