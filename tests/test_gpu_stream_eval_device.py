"""The streaming evaluator's DEVICE verdicts (mpc_amd/csrc/stream_eval_dev.cpp: evdev_blocks, k_eval_verify), case by case: the
host follows a verdict without looking at the block's repeat pattern again, so a verdict under the wrong mate, a compare that
skips bytes or two first occurrences of one wire that go unnoticed evaluate the block under the wrong wire binding — and a
kernel that refuses too much sends every block back to the host's parser without failing anything.  The scripts of
tests/stream_eval_dev_cases.py (checked against the oracle on the CPU by tests/test_stream_eval_dev_cases.py) run through three
evaluators: the engine's, the oracle's StreamEval on the very same bytes (changed bytes included) and an engine evaluator under
GC_STREAM_NO_SKELETON (every block parsed gate by gate).  Behind every step the wires of its blocks are equal in all three, and
the engine's counters moved by exactly what the script says: (parsed, matched) of gc_stream_eval_stats, (device blocks,
fallbacks) of gc_stream_eval_dev_stats, device blocks + fallbacks = blocks guessed."""
import os

import numpy as np
import pytest

import oracle
from mpc_amd import engine
from tests import stream_eval_dev_cases as cases

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("GC_STREAM_NO_DEVICE_MATCH") or os.environ.get("GC_STREAM_NO_SKELETON")),
                                 reason="the device match is switched off (GC_STREAM_NO_DEVICE_MATCH / GC_STREAM_NO_SKELETON)")]


def _feed(ev, data, hold):
    """(bytes used, blocks, more, status) of gc_stream_eval_blocks on the buffer: pageable, or in pinned memory"""
    try:
        if hold is None:
            used, nb, more = ev.blocks(data)
        else:
            hold.a[:len(data)] = np.frombuffer(data, np.uint8)
            used, nb, more = ev.blocks_at(hold.a.ctypes.data, len(data))
        return used, nb, more, 0
    except engine.EngineError as e:
        return ev.last_blocks + (e.code,)


def _run(case, pinned):
    ctx = engine.Context(0)
    ge, oe = engine.StreamEval(ctx, case.key), oracle.StreamEval(case.key)
    os.environ["GC_STREAM_NO_SKELETON"] = "1"
    try:
        gp = engine.StreamEval(ctx, case.key)  # the same bytes, every block parsed
    finally:
        del os.environ["GC_STREAM_NO_SKELETON"]
    for w, lab in case.first.items():
        for ev in (ge, oe, gp):
            ev.set(w, lab)
    hold = engine.PinnedArray((case.max_data,), np.uint8) if pinned else None
    for n, s in enumerate(case.steps):
        what = "%s step %d (%s %s)" % (case.name, n, s.kind, s.note)
        e = s.expect
        dev0, st0 = ge.dev_stats(), ge.stats()
        if s.kind == "one":
            b = s.blocks[0]
            for ev in (ge, oe, gp):
                assert ev.circuit(b.c.NumGates, b.c.NumWires, b.nwires, b.raw) == len(b.raw), what
        else:
            got, plain = _feed(ge, s.data, hold), _feed(gp, s.data, hold)
            for b in s.blocks[:s.taken]:
                assert oe.circuit(b.c.NumGates, b.c.NumWires, b.nwires, b.raw) == len(b.raw), what
            used = sum(20 + len(b.raw) for b in s.blocks[:s.taken])
            want = (used, s.taken, e["more"], cases.GC_E_ARG if e["error"] else 0)
            print("%s: %s, gate by gate %s, expected %s" % (what, got, plain, want))
            assert got == want, what
            assert plain == want, what
        dev1, st1 = ge.dev_stats(), ge.stats()
        d = {"dev": dev1[0] - dev0[0], "fallbacks": dev1[1] - dev0[1], "parsed": st1[0] - st0[0], "matched": st1[1] - st0[1]}
        print("%s: counters moved by %s, expected %s" % (what, d, {k: e[k] for k in d}))
        if s.kind == "buf" and not e["error"]:
            assert d["dev"] + d["fallbacks"] == e["guessed"], what
        assert d == {k: e[k] for k in d}, what
        for b in s.blocks[:s.taken]:
            for w in b.watch:
                assert ge.get(w) == oe.get(w) == gp.get(w), "%s: wire %d of block %s" % (what, w, b.name)
    assert gp.stats()[1] == 0 and gp.dev_stats() == (0, 0)
    ge.close()
    gp.close()
    if hold is not None:
        hold.close()
    ctx.close()


@pytest.mark.parametrize("pinned", [False, True])
def test_mates_of_one_shape(pinned):
    """1. bindings of one circuit that differ only in which ids repeat, interleaved in device-size buffers: every block is
    adopted under ITS pattern, whichever mate was guessed — the finer pattern for a coarser block (refused by the all-pairs
    distinctness loop alone) and the other way round (refused by the gf_canon compare alone)"""
    _run(cases.case_mates(), pinned)


def test_as_many_patterns_as_the_table_holds():
    """2. kSkelVariants patterns of one shape in forward, reverse and shuffled order: the walk reaches every mate"""
    _run(cases.case_full_table(), False)


def test_patterns_evicted_while_known_to_the_device():
    """3. a pattern more than the table holds, patterns that arrive inside a buffer: no block is adopted under a skeleton that
    is gone, and the split between device and host is the one the variant list's rules give (cases.HostModel)"""
    _run(cases.case_eviction(), False)


def test_id_widths_inside_one_block():
    """4. 16-bit and 32-bit records in one block, global ids in both"""
    _run(cases.case_widths(), False)


def test_blocks_that_name_about_kUniqLds_wires():
    """5. kUniqLds - 1 and kUniqLds distinct wires are the device's, kUniqLds + 1 the host matcher's; the last first occurrence
    equal to the first one is refused; (8.) fewer blocks than a device turn takes stay on the host"""
    _run(cases.case_uniq_edge(), False)


@pytest.mark.parametrize("pinned", [False, True])
def test_every_region_of_the_masked_compare(pinned):
    """6. an XOR made XNOR at offset 0, on both sides of every unrolled load's boundary, in the second trip of the 16-byte
    loop and in the tail bytes: refused; a changed row byte: adopted"""
    _run(cases.case_compare_regions(), pinned)


def test_ids_the_device_reads_but_must_not_trust():
    """7. a fresh wire in range: adopted, the binding follows; an id beyond the header's numWires: the call fails where the
    block is, the blocks in front of it are done, the stream goes on"""
    _run(cases.case_untrusted_ids(), False)


def test_thresholds_of_the_device_turn():
    """8. kMinDevBuffer to the byte; runs of known blocks in front of and behind a block met for the first time"""
    _run(cases.case_thresholds(), True)
