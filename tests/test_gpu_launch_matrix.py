"""One row per kernel build that the launchers of a batch pass can select (mpc_amd/csrc/launch_dispatch.h: with_rounds over the
key length, with_flag over OR gates / debug profile / store_all, and the branches beside them).  Every row runs one garble and
one eval pass and compares R, the tables, the output labels and the decoded bits of EVERY instance with the oracle; and it
asserts the facts that show which launcher the pass took: gc_batch_keyed_path, whether the wires are in LDS, and
gc_batch_last_launches of both passes.

Rows: key lengths 16 / 24 / 32 bytes x
  * "mix" of tests/test_gpu_batch_paths.py (OR gates) and "mix0", the same generator without OR gates, three instances:
    schedule 1 (k_*_flat), schedule 2 and schedule 1 + store_all (k_*_lds without / with every wire stored), schedule 0 (the
    level kernels: k_*_level_split on a level with hashed gates, k_*_level on one without; also 70 instances, whose tile
    covers whole waves: the other build of k_*_level), schedules 1 and 2 with
    the debug profile (the PROF builds), the keyed calls on path 1 (k_*_flat_keyed) and on path 2 forced, plain and split form;
  * "big" of that file (live labels beyond LDS, OR gates): three instances on the fused HBM kernels, plain and profiled; ONE
    instance as a cooperative launch — or one launch per level where the context does not run cooperative passes: the row
    asserts whichever gc_ctx_coop_stats reports;
  * "col", the circuit without OR gates of test_global_wire_kernels_column_sliced_narrow_levels (every level narrow: k_*_col),
    three instances.
The streaming job and pool launchers, GC_LEVEL_WHOLE_GATES and GC_NO_COOP have their rows in tests/test_gpu_stream.py,
tests/test_gpu_limits.py and tests/test_gpu_batch_paths.py.

The oracle's run of an instance depends on the circuit, the instance's slice of the random stream (the same for every row of a
circuit and batch) and the key: it is computed once and shared between the rows."""
import functools

import numpy as np
import pytest

from mpc_amd.circuit import synthetic_levelised
from tests.test_gpu_batch_keyed import Pair
from tests.test_gpu_batch_keyed import ctx  # noqa: F401  (the module-scoped fixture)
from tests.test_gpu_batch_paths import LEVELS_BIG, circuit, facts, keyed, one_key, seen, setup
from tests.util import drbg

pytestmark = pytest.mark.gpu

KEYLENS = [16, 24, 32]


@functools.lru_cache(maxsize=None)
def build(name):
    if name == "mix0":  # "mix" without OR gates
        return synthetic_levelised(10, 48, 0.3, seed=5, ninputs=40, or_frac=0, inv_frac=0.1, xnor_frac=0.1)
    if name == "col":  # tests/test_gpu_garble_eval.py: 700 levels of 64 gates, no OR, live labels beyond LDS
        return synthetic_levelised(700, 64, 0.2, seed=79, ninputs=64, inv_frac=0.08, xnor_frac=0.1)
    return circuit(name)


_references = {}


class MatrixPair(Pair):
    """a Pair whose random stream and input bits depend on (circuit, batch) only, so that the oracle's runs are shared"""

    def __init__(self, ctx, name, batch):
        super().__init__(ctx, build(name), batch, "matrix/%s/%d" % (name, batch))
        self.name = name

    def reference(self, i, key):
        k = (self.name, self.batch, i, bytes(key))
        if k not in _references:
            _references[k] = super().reference(i, key)
        return _references[k]


def key_of(keylen):
    return drbg("matrix/key/%d" % keylen, keylen)


def keyed_with(p, keylen):
    """tests/test_gpu_batch_paths.py: keyed, at any key length"""
    if keylen == 32:
        return keyed(p, "matrix/%s/%d" % (p.name, p.batch))
    keys = np.frombuffer(drbg("matrix/keys/%s/%d/%d" % (p.name, p.batch, keylen), p.batch * keylen), np.uint8).reshape(p.batch, keylen)
    p.keyed(p.ctx.to_device(keys), keylen)
    got = p.results()
    for i in range(p.batch):
        p.check(got, i, keys[i])
    return [p.gb.last_launches, p.ev.last_launches]


# ---- circuits with a flattened plan: how -> (batch, wires in LDS, keyed path) ------------------------------------------------
LDS_ROWS = {
    "schedule1": (3, True, 1),
    "schedule2": (3, True, 0),
    "schedule1+store_all": (3, True, 0),
    "schedule0": (3, False, 0),
    "schedule0/70": (70, False, 0),
    "schedule1+prof": (3, True, 1),
    "schedule2+prof": (3, True, 0),
    "keyed1": (3, True, 1),
    "keyed2/plain": (3, True, 2),
    "keyed2/split": (3, True, 2),
}


@pytest.mark.parametrize("how", list(LDS_ROWS))
@pytest.mark.parametrize("name", ["mix", "mix0"])
@pytest.mark.parametrize("keylen", KEYLENS)
def test_lds_plan_rows(ctx, keylen, name, how):
    batch, lds, path = LDS_ROWS[how]
    assert (build(name).stats()["OR"] != 0) == (name == "mix")
    p = MatrixPair(ctx, name, batch)
    setup(p, "schedule1" if how.startswith("keyed") else how.split("/")[0])
    for b in (p.gb, p.ev):
        if how.endswith("+prof"):
            b.debug_profile(True)
        if how.startswith("keyed2"):
            form = 2 if how.endswith("split") else 1
            b.set_keyed_path(2)
            b.set_keyed_hbm_form(form)
            assert b.keyed_hbm_form == form
    f = facts(p)
    launches = keyed_with(p, keylen) if how.startswith("keyed") else one_key(p, key_of(keylen))
    seen((keylen, name, how), f, launches)
    assert f[2:] == [lds, path] and facts(p) == f
    steps = p.dc.info.n_steps
    assert steps > 1 and launches == ([steps, steps] if how.startswith("schedule0") else [1, 1])
    p.close()


# ---- circuits whose wires live in HBM -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["plain", "prof"])
@pytest.mark.parametrize("name", ["big", "col"])
@pytest.mark.parametrize("keylen", KEYLENS)
def test_fused_hbm_rows(ctx, keylen, name, how):
    """three instances, one launch: k_*_fused for "big" (plain and profiled), k_*_col for "col" (which has no profiled build:
    its profiled row is k_*_fused again, without OR gates)"""
    assert (build(name).stats()["OR"] != 0) == (name == "big")
    p = MatrixPair(ctx, name, 3)
    if how == "prof":
        for b in (p.gb, p.ev):
            b.debug_profile(True)
    f = facts(p)
    launches = one_key(p, key_of(keylen))
    seen((keylen, name, how), f, launches)
    assert f == [3, 1, False, 2] and facts(p) == f and launches == [1, 1]
    p.close()


@pytest.mark.parametrize("keylen", KEYLENS)
def test_one_wide_instance_rows(ctx, keylen):
    """ONE instance of "big": the cooperative launch where the context runs cooperative passes (state 1), one launch per level
    where it does not (state -1, no pass ever lost a workgroup)"""
    p = MatrixPair(ctx, "big", 1)
    f = facts(p)
    launches = one_key(p, key_of(keylen))
    state, timeouts = ctx.coop_stats()
    seen((keylen, "big", 1), f, launches, state, timeouts)
    assert f == [1, 1, False, 2] and facts(p) == f
    assert state != 0, "a wide pass has run: the context has decided"
    if state == 1:
        assert launches == [1, 1]
    elif timeouts == 0:
        assert launches == [LEVELS_BIG, LEVELS_BIG]
    else:  # cooperative passes went off on the way (a pass lost a workgroup and was done again): either form, per pass
        assert set(launches) <= {1, LEVELS_BIG}
    p.close()
