"""Which kernels a pass of a gc_batch runs (mpc_amd/csrc/engine.cpp: path_for), pinned as facts a caller can observe: the
row stride and tile width of the device arrays, whether the wires are in LDS, gc_batch_keyed_path, and gc_batch_last_launches
after a garble and after an eval pass.  Every row also runs garble and eval once and compares R, the tables, the output labels
and the decoded bits of every instance with the oracle.

The literals below were RECORDED by running this table on the library of the commit before the decision was gathered into one
function (the rows print what they see before they assert): a later change of the host side is checked against them, not
against a reading of the code."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mpc_amd import engine
from mpc_amd.circuit import GATE, Circuit, synthetic_levelised
from tests.test_gpu_batch_keyed import Pair
from tests.test_gpu_batch_keyed import ctx  # noqa: F401  (the module-scoped fixture)
from tests.test_gpu_garble_eval import KEY128, KEY256
from tests.util import drbg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def circuit(name):
    if name == "mix":  # every gate type, 480 gates, a flattened plan
        return synthetic_levelised(10, 48, 0.3, seed=5, ninputs=40, or_frac=0.1, inv_frac=0.1, xnor_frac=0.1)
    if name == "big":  # live labels beyond LDS, 14 levels of 2 500 gates (tests/test_gpu_garble_eval.py)
        return synthetic_levelised(14, 2500, 0.3, seed=77, ninputs=64, or_frac=0.05, inv_frac=0.08, xnor_frac=0.1)
    if name == "narrow":  # live labels beyond LDS, 900 levels of 64 gates: not wide
        return synthetic_levelised(900, 64, 0.3, seed=78, ninputs=64, or_frac=0.05, inv_frac=0.08, xnor_frac=0.1)
    assert name == "empty"  # no gate at all: the four outputs are the last four input wires
    return Circuit(8, [4, 4], [4], np.zeros(0, GATE), "empty")


def facts(p):
    """(stride, tile_instances, lds_wires, keyed_path): the same for the garbler's and the evaluator's batch"""
    f = [(b.stride, b.tile_instances, b.lds_wires, b.keyed_path) for b in (p.gb, p.ev)]
    assert f[0] == f[1]
    return list(f[0])


def arrays(p):
    return [int(engine.lib().gc_batch_dev_wires(b.h) or 0) for b in (p.gb, p.ev)]


def one_key(p, key=KEY256):
    """one garble and one eval pass under `key`, every instance against the oracle -> [launches of garble, launches of eval]"""
    p.one_key(key)
    got = p.results()
    for i in range(p.batch):
        p.check(got, i, key)
    return [p.gb.last_launches, p.ev.last_launches]


def keyed(p, tag):
    """the same with one 32-byte key per instance"""
    keys = np.frombuffer(drbg("paths/keys/" + tag, p.batch * 32), np.uint8).reshape(p.batch, 32)
    p.keyed(p.ctx.to_device(keys), 32)
    got = p.results()
    for i in range(p.batch):
        p.check(got, i, keys[i])
    return [p.gb.last_launches, p.ev.last_launches]


def setup(p, how):
    for b in (p.gb, p.ev):
        if how.startswith("schedule"):
            b.set_schedule(int(how[8]))
        if how == "schedule1+store_all":
            b.set_store_all(True)
        if how == "schedule0+nograph":
            b.set_graph(False)


def seen(row, *what):
    """print what a row sees (that is how the literals were recorded) -> the same as lists"""
    print("batch path row %s: %s" % (row, json.dumps(what)))
    return json.loads(json.dumps(what))


# ---- a circuit with a flattened plan (and the circuit without gates): schedules 1, 2, 0 and store_all -------------------------
# row: (circuit, batch, set-up) -> (stride, tile, lds_wires, keyed_path), (launches of garble, of eval), all wires readable
N_STEPS_MIX = 10  # gc_plan_info.n_steps of "mix": schedule 0 launches once per step
SCHEDULE_ROWS = {
    ("mix", 3, "schedule1"): [[3, 1, True, 1], [1, 1], False],
    ("mix", 3, "schedule2"): [[3, 1, True, 0], [1, 1], False],
    ("mix", 3, "schedule1+store_all"): [[3, 1, True, 0], [1, 1], True],
    ("mix", 3, "schedule0"): [[64, 1, False, 0], [10, 10], True],
    ("mix", 3, "schedule0+nograph"): [[64, 1, False, 0], [10, 10], True],
    ("mix", 70, "schedule1"): [[70, 1, True, 1], [1, 1], False],
    ("mix", 70, "schedule2"): [[70, 1, True, 0], [1, 1], False],
    ("mix", 70, "schedule1+store_all"): [[70, 1, True, 0], [1, 1], True],
    ("mix", 70, "schedule0"): [[128, 1, False, 0], [10, 10], True],
    ("mix", 70, "schedule0+nograph"): [[128, 1, False, 0], [10, 10], True],
    ("empty", 3, "schedule1"): [[3, 1, True, 0], [0, 0], False],
    ("empty", 3, "schedule2"): [[3, 1, True, 0], [0, 0], False],
    ("empty", 3, "schedule1+store_all"): [[3, 1, True, 0], [0, 0], True],
    ("empty", 3, "schedule0"): [[64, 1, False, 0], [0, 0], True],
    ("empty", 70, "schedule1"): [[70, 1, True, 0], [0, 0], False],
}


def can_read_wires(p):
    try:
        p.gb.read_wires()
        return True
    except engine.EngineError:
        return False


@pytest.mark.parametrize("row", list(SCHEDULE_ROWS), ids=lambda r: "%s-%d-%s" % r)
def test_schedule_rows(ctx, row):
    """schedule 1: flattened, one launch, keyed path 1 | schedule 2: the hash-phase LDS kernels, keyed path 0 | store_all: the
    LDS kernels, every wire present | schedule 0: one launch per step, recorded as a graph or not | no gates: no launch on any
    schedule, and garble still draws R and the input labels (they ARE the output labels the oracle is compared with)"""
    name, batch, how = row
    p = Pair(ctx, circuit(name), batch, "paths/%s/%d/%s" % row)
    setup(p, how)
    f = facts(p)
    launches = one_key(p)
    got = seen(row, f, launches, can_read_wires(p))
    assert facts(p) == f
    if name == "mix" and how.startswith("schedule0"):
        assert p.dc.info.n_steps == N_STEPS_MIX and launches == [N_STEPS_MIX, N_STEPS_MIX]
    if name == "empty":
        assert launches == [0, 0]
    want = SCHEDULE_ROWS[row]
    assert got == want
    p.close()


# the same batches with gc_batch_set_keyed_path(2): schedule 1 only (GC_E_ARG otherwise); the one-key passes are not affected
# row -> facts once forced, launches of the keyed garble and eval, all wires readable after them; then the one-key passes:
# launches, all wires readable
FORCED_ROWS = {
    ("mix", 3, "schedule1"): [[3, 1, True, 2], [1, 1], True, [1, 1], False],
    ("mix", 70, "schedule1"): [[70, 1, True, 2], [1, 1], True, [1, 1], False],
    ("mix", 3, "schedule1+store_all"): [[3, 1, True, 2], [1, 1], True, [1, 1], True],
    ("mix", 70, "schedule1+store_all"): [[70, 1, True, 2], [1, 1], True, [1, 1], True],
}


@pytest.mark.parametrize("row", list(FORCED_ROWS), ids=lambda r: "%s-%d-%s" % r)
def test_forced_keyed_rows(ctx, row):
    name, batch, how = row
    p = Pair(ctx, circuit(name), batch, "paths/forced/%s/%d/%s" % row)
    setup(p, how)
    for b in (p.gb, p.ev):
        b.set_keyed_path(2)
    f = facts(p)
    kl = keyed(p, "%s/%d/%s" % row)
    wires_after_keyed = can_read_wires(p)
    launches = one_key(p)
    got = seen(("forced",) + row, f, kl, wires_after_keyed, launches, can_read_wires(p))
    one = SCHEDULE_ROWS[row]
    assert f[:3] == one[0][:3] and f[3] == 2 and got[3:] == one[1:]  # the one-key row, but for the keyed path
    assert got == FORCED_ROWS[row]
    p.close()


@pytest.mark.parametrize("how", ["schedule2", "schedule0"])
def test_forcing_the_keyed_path_is_refused_off_schedule_1(ctx, how):
    p = Pair(ctx, circuit("mix"), 3, "paths/refused/" + how)
    setup(p, how)
    with pytest.raises(engine.EngineError):
        p.gb.set_keyed_path(2)
    assert facts(p) == SCHEDULE_ROWS[("mix", 3, how)][0]
    p.close()


# one batch taken through schedules 1 -> 2 -> 0 -> 1: (facts, launches, what became of the arrays of the stage before) per stage
WALK = [[[70, 1, True, 1], [1, 1], "first"], [[70, 1, True, 0], [1, 1], "kept"], [[128, 1, False, 0], [10, 10], "re-sized"],
        [[70, 1, True, 1], [1, 1], "re-sized"]]


def test_one_batch_through_the_schedules(ctx):
    """the arrays are re-sized only where the layout differs (where the stage before had the same stride and tile, the very
    same arrays serve), and every stage still matches the oracle"""
    p = Pair(ctx, circuit("mix"), 70, "paths/walk")
    got, before = [], None
    for s in (1, 2, 0, 1):
        setup(p, "schedule%d" % s)
        f, a = facts(p), arrays(p)
        same_layout = before is not None and f[:2] == before[0][:2]
        if same_layout:
            assert a == before[1], "schedule %d: same layout, other arrays" % s
        got.append([f, one_key(p), "first" if before is None else "kept" if same_layout else "re-sized"])
        before = (f, a)
    got = seen("walk", *got)
    for stage, s in zip(got, (1, 2, 0, 1)):
        assert stage[:2] == SCHEDULE_ROWS[("mix", 70, "schedule%d" % s)][:2]
    assert got == WALK
    p.close()


# ---- circuits whose wires live in HBM -----------------------------------------------------------------------------------------

HBM_BATCH3 = [[3, 1, False, 2], [1, 1], True]
WIDE_FACTS = [1, 1, False, 2]
LEVELS_BIG = 14


def test_fused_hbm_batch(ctx):
    """three instances of a circuit whose live labels exceed LDS: the fused HBM kernel, one launch, keyed path 2"""
    p = Pair(ctx, circuit("big"), 3, "paths/big3")
    f = facts(p)
    got = seen("big3", f, one_key(p), can_read_wires(p))
    assert got == HBM_BATCH3
    p.close()


def test_one_wide_instance_cooperative(ctx):
    """ONE instance of the same circuit: the wide form; as one cooperative launch where the context can"""
    p = Pair(ctx, circuit("big"), 1, "paths/big1")
    f = facts(p)
    seen("big1", f)
    assert f == WIDE_FACTS
    launches = one_key(p)
    state, timeouts = ctx.coop_stats()
    seen("big1 launches", launches, state, timeouts)
    if state == 0 or (state < 0 and timeouts == 0):
        p.close()
        pytest.skip("cooperative passes are not in use on this box (self-test / GC_NO_COOP)")
    assert launches == [1, 1]
    for b in (p.gb, p.ev):  # the debug profile is a build of the fused HBM kernel: the batch leaves the wide form
        b.debug_profile(True)
    assert one_key(p) == [1, 1] and facts(p) == f
    p.close()


NO_COOP = {"facts": [1, 1, False, 2], "first": [14, 14], "replayed": [14, 14], "other key size": [14, 14], "direct": [14, 14],
           "profiled": [[1, 1, False, 2], [1, 1]], "narrow": [[1, 1, False, 2], [1, 1]], "coop state": -1}


def no_coop_child():
    """(runs in a process with GC_NO_COOP=1) one wide instance as level launches, and what does not qualify as wide"""
    c = engine.Context(0)
    out = {}
    p = Pair(c, circuit("big"), 1, "paths/nocoop")
    out["facts"] = facts(p)
    out["first"] = one_key(p)
    out["replayed"] = one_key(p)            # the second call replays the recorded graph
    out["other key size"] = one_key(p, KEY128)  # ... and another key size records its own
    for b in (p.gb, p.ev):
        b.set_graph(False)
    out["direct"] = one_key(p)
    for b in (p.gb, p.ev):
        b.debug_profile(True)
    out["profiled"] = [facts(p), one_key(p)]
    p.close()
    p = Pair(c, circuit("narrow"), 1, "paths/narrow")  # levels of 64 gates: the fused HBM kernel, whatever the batch
    out["narrow"] = [facts(p), one_key(p)]
    p.close()
    out["coop state"] = c.coop_stats()[0]
    c.close()
    print("no-coop rows: " + json.dumps(out))


def test_one_wide_instance_level_launches_and_narrow_instance():
    """GC_NO_COOP=1 is read when a context first meets a wide pass, so in a child process: per-level launches
    (last_launches == levels), recorded as a graph, replayed, per key size, launched directly with the graph off; with the debug
    profile on the batch leaves the form; ONE instance of a narrow deep circuit never takes it (1 launch, not 900)"""
    code = "import os, sys; sys.path.insert(0, os.getcwd()); from tests.test_gpu_batch_paths import no_coop_child; no_coop_child()"
    args = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code]
    r = subprocess.run(args, cwd=ROOT, env=dict(os.environ, GC_NO_COOP="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "child exit status %d\n%s\n%s" % (r.returncode, r.stdout[-4000:], r.stderr[-4000:])
    line = [l for l in r.stdout.splitlines() if l.startswith("no-coop rows: ")][-1]
    print(line)
    got = json.loads(line[len("no-coop rows: "):])
    assert got["first"] == [LEVELS_BIG, LEVELS_BIG] and got["narrow"][1] == [1, 1] and got["profiled"][1] == [1, 1]
    assert got == NO_COOP
