"""OpReturn for S sessions (gc_stream_eval_batch_return_labels_dev / _return_labels): the active labels of a list
of wires as gc_label [S][n], against gc_stream_eval_batch_get_wire per id and fed into the garbler's decode.  The store is the one
the per-step gc_stream_eval_batch_circuit_host route leaves after the program of tests/stream_batch_intake_cases.py."""
import numpy as np
import pytest

from mpc_amd import engine
from mpc_amd.circuit import LABEL
from tests import stream_batch_intake_cases as ic

pytestmark = pytest.mark.gpu

KEYLEN = 32
NEVER_SET = 0x5000   # a wire id no step of the program names, inside the store
GROWS = 0x40100      # ... and one beyond it: the largest id of the program is below 0x20040, and the store at most doubles


class Both:
    """the garbler and the evaluator after the whole program: the garbler through gc_stream_batch_garble, the evaluator through
    one gc_stream_eval_batch_circuit_host per step on the oracle's framed bytes"""

    def __init__(self, ctx, S):
        self.ref = ref = ic.reference(S, KEYLEN)
        self.S = S
        self.d_keys = engine.DeviceBuffer(ctx, data=ref["keys"])
        self.d_rnd = engine.DeviceBuffer(ctx, data=ref["rnd"])
        self.sb = engine.StreamBatch(ctx, S, self.d_keys, KEYLEN, self.d_rnd, ref["prim"])
        stride = (max(len(x) for x in ref["streams"][0]) + 3) & ~3
        d_out = engine.DeviceBuffer(ctx, shape=S * stride)
        for c, in_, out_ in ref["steps"]:
            self.sb.garble(c.Gates, c.NumWires, in_, out_, d_out, stride)
        d_out.close()
        self.se = engine.StreamEvalBatch(ctx, S, self.d_keys, KEYLEN)
        self.se.set_wires(ref["prim"], engine.DeviceBuffer(ctx, data=ref["inlab"]))
        framed = ref["framed"]
        for k, (c, in_, out_) in enumerate(ref["steps"]):
            at, n = ref["offs"][k] + ic.HEADER, len(ref["streams"][0][k])
            blocks = np.ascontiguousarray(framed[:, at: at + n])
            assert self.se.circuit_host(c.NumGates, c.NumWires, max(max(in_), max(out_)) + 1, blocks, n, n, 0) == n
        assert (self.se.bad() == 0).all()

    def close(self):
        self.se.close(), self.sb.close()
        self.d_keys.close(), self.d_rnd.close()


def columns(se, ids):
    """LABEL [S, len(ids)] through one gc_stream_eval_batch_get_wire per distinct id"""
    col = {w: se.get(w) for w in set(ids)}
    return np.stack([col[w] for w in ids], axis=1)


@pytest.mark.parametrize("S", [3, 67])
def test_return_labels_equal_get_wire_per_id(S):
    ctx = engine.Context(0)
    b = Both(ctx, S)
    ref, se = b.ref, b.se
    every = ref["every"]
    assert len(every) >= 80
    for w in ref["outs"][::7]:  # the store is the oracle's
        got = se.get(w)
        assert [(int(x["d0"]), int(x["d1"])) for x in got] == ref["ev"][w], w
    for n in (1, 63, 64, 65, 130):
        ids = [every[(7 * j + n) % len(every)] for j in range(n)]  # (130 of them: some twice)
        d_out = engine.DeviceBuffer(ctx, data=np.full((S, n), 0xEE, np.uint8).repeat(16, axis=1).view(LABEL))
        assert se.return_labels_dev(ids, d_out) is d_out
        want = columns(se, ids)
        assert (d_out.numpy().reshape(S, n) == want).all(), n
        assert (se.return_labels(ids) == want).all(), n  # the host form
        d_out.close()
    # a repeated id, a never-set id (zero, as get_wire gives it), no ids
    ids = [every[40], NEVER_SET, every[40], every[5], NEVER_SET, every[40]]
    got = se.return_labels(ids)
    assert (got == columns(se, ids)).all() and (got[:, 1] == np.zeros(S, LABEL)).all() and (got[:, 0] == got[:, 5]).all()
    assert (got[:, 0] != np.zeros(S, LABEL)).all()
    assert se.return_labels([]).shape == (S, 0)
    # an id beyond the store makes it grow (zeros there) and leaves what it held
    before = se.return_labels(every)
    got = se.return_labels([every[3], GROWS, every[-1]])
    assert (got[:, 1] == np.zeros(S, LABEL)).all() and (got[:, 0] == before[:, 3]).all() and (got[:, 2] == before[:, -1]).all()
    assert (se.return_labels(every) == before).all() and (se.get(GROWS) == np.zeros(S, LABEL)).all()
    # an id at GC_STREAM_MAX_WIRES (2^28 by default) is refused, by both forms
    d_out = engine.DeviceBuffer(ctx, shape=(S, 2), dtype=LABEL)
    for call in (lambda: se.return_labels([every[0], 1 << 28]), lambda: se.return_labels_dev([every[0], 1 << 28], d_out)):
        with pytest.raises(engine.EngineError) as err:
            call()
        assert err.value.code == engine.GC_E_ARG
    b.close()
    ctx.close()


@pytest.mark.parametrize("S", [3, 67])
def test_returned_labels_decode_to_the_plaintext_result(S):
    ctx = engine.Context(0)
    b = Both(ctx, S)
    ref, outs = b.ref, b.ref["outs"]
    n = len(outs)
    d_lab = engine.DeviceBuffer(ctx, shape=(S, n), dtype=LABEL)
    d_bits = engine.DeviceBuffer(ctx, shape=(S, n))
    d_bad = engine.DeviceBuffer(ctx, data=np.full(S, 0xFFFFFFFF, np.uint32))
    b.se.return_labels_dev(outs, d_lab)
    b.sb.decode(outs, d_lab, d_bits, d_bad)
    vals = np.array([[ref["vals"][s][o] for o in outs] for s in range(S)], np.uint8)
    assert (d_bits.numpy().reshape(S, n) == vals).all() and (d_bad.numpy() == 0).all()
    assert 0 < vals.sum() < vals.size
    # one label of one session flipped: 0xff in exactly that entry
    lab = b.se.return_labels(outs)
    s, j = S - 1, n // 2
    lab["d1"][s, j] ^= np.uint64(1 << 40)
    bits, bad = b.sb.decode(outs, lab)
    want = vals.copy()
    want[s, j] = 0xff
    assert (bits == want).all() and bad[s] == 1 and bad.sum() == 1
    b.close()
    ctx.close()
