"""The expected values of the GPU tests of gc_kos_multi_* (tests/test_gpu_kos_multi.py) are oracle.kos_receiver_tags /
kos_sender_check run on every session alone.  Here the C oracle's tags of random sessions are pinned against the Python
restatement written from the Go text (tests/py_ot_reference.py) at the session lengths where the multi kernel's index changes
shape: no result labels at all (the sums run over the 256 labels of the choice vector only), one, and one past a byte
boundary of the packed choice bits.  The multi entry points themselves must exist for these values to be of use: the module
asks the library for them."""
import numpy as np
import pytest

import oracle
from mpc_amd import engine
from tests import py_ot_reference as po


def labels(rng, n):
    out = np.zeros(n, oracle.LABEL)
    out["d0"] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    out["d1"] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    return out


def tups(a):
    return [(int(l["d0"]), int(l["d1"])) for l in a]


@pytest.mark.parametrize("per", [0, 1, 129])
def test_oracle_tags_of_random_sessions_agree_with_the_python_restatement(per):
    L = engine.lib()
    assert hasattr(L, "gc_kos_multi_receiver_tags") and hasattr(L, "gc_kos_multi_sender_check")
    rng = np.random.default_rng(1000 + per)
    for s in range(2):  # sessions with different seed2, delta and labels, each alone
        seed2, delta = tups(labels(rng, 2))
        b, bcv = rng.integers(0, 2, per).astype(np.uint8), rng.integers(0, 2, 256).astype(np.uint8)
        sent, cvs = labels(rng, per), labels(rng, 256)
        result, cv = sent.copy(), cvs.copy()
        for a, f in ((result, b), (cv, bcv)):
            a["d0"][f.astype(bool)] ^= np.uint64(delta[0])
            a["d1"][f.astype(bool)] ^= np.uint64(delta[1])
        x, t0, t1 = oracle.kos_receiver_tags(seed2, result, b, cv, bcv)
        assert (x, t0, t1) == po.kos_receiver_tags(seed2, tups(result), list(b), tups(cv), list(bcv))
        assert oracle.kos_sender_check(seed2, sent, cvs, delta, x, t0, t1)
        assert not oracle.kos_sender_check(seed2, sent, cvs, delta, x, (t0[0] ^ 1, t0[1]), t1)
