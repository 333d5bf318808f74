"""tests/keyed_split_cases.py builds what it says: the host plan's levels are the gate counts given, and the levels have the
column lanes the GPU cases of tests/test_gpu_batch_keyed_hbm_split.py rely on (1 024 lanes and the narrowest split level for
each role, a wide level of free gates only, one AND beside many XORs, narrow and wide levels in alternation)."""
import pytest

from mpc_amd.circuit import AND, XOR
from tests import keyed_split_cases as sc


@pytest.mark.parametrize("ti", [1, 4])
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_plan_levels_are_the_levels_given(name, ti):
    want = [{int(k): v for k, v in lv.items() if v} for lv in sc.CASES[name](ti)]
    assert sc.plan_levels(sc.build(name, ti)) == want


@pytest.mark.parametrize("ti", [1, 4])
def test_lane_counts(ti):
    total = lambda lv, ev: sum(sc.lanes(lv, ti, ev))
    b = sc.boundary(ti)
    assert total(b[0], False) == 1024 and total(b[1], False) == 1024 + ti
    assert total(b[2], True) == 1024 and total(b[3], True) == 1024 + ti
    f = sc.free_only(ti)[1]
    assert sc.lanes(f, ti, False)[0] == 0 and total(f, True) > 1024
    o = sc.one_and(ti)
    assert o[0] == {AND: 1, XOR: 400}  # as a level of its own: split at tiles of four, one pass at tiles of one
    assert sc.lanes(o[1], ti, False)[0] == 16 * ti and sc.lanes(o[1], ti, True)[0] == 8 * ti and total(o[1], True) > 1024
    n = sc.narrow_wide_narrow(ti)
    assert [total(lv, True) > 1024 for lv in n] == [False, True, False, True, False]
    assert [total(lv, False) > 1024 for lv in n] == [False, True, False, True, False]
