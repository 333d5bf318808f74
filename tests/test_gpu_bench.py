"""bench.py on the device: a plain run carries the headline alone, and what --dump-outputs writes is what the timed path
computed — the output bits against plaintext evaluation, R, the sampled garbled tables and the evaluator's output labels
against the oracle's garble / eval of the same instances."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from mpc_amd import LABEL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = bytes(range(32))  # bench.py's default 32-byte key


def words(labels):
    """LABEL records -> u32 words as float64, the dump's layout"""
    a = np.ascontiguousarray(labels, LABEL)
    return a.view(np.uint32).reshape(a.shape + (4,)).astype(np.float64)


def test_plain_run_dumps_what_the_last_step_computed(tmp_path, aes_circ):
    c = aes_circ
    batch, nin, nout = 256, c.num_inputs, c.num_outputs
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                        "--batch", str(batch), "--dump-outputs", str(out)],
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = lines[0]
    assert j["steps"] == 5 and j["warmup"] == 2 and j["full"] is False and j["config"]["outputs_ok"] and j["value"] > 0
    assert "garble_ms" not in j and "synthetic" not in j and "cpu_baseline" not in j
    d = {n[:-4]: np.load(out / n) for n in os.listdir(out)}
    assert sum(os.path.getsize(out / n) for n in os.listdir(out)) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert (d["instances"] == np.arange(batch)).all() and d["mismatches_all_steps"][0] == 0
    # bench.py's inputs at rank 0: seeded numpy generators (Context.random_u8)
    rnd = np.random.default_rng(1234).integers(0, 256, (batch, nin + 1, 16), dtype=np.uint8)
    bits = np.random.default_rng(4321).integers(0, 2, (batch, nin), dtype=np.uint8)
    for i in range(0, batch, 8):
        assert (d["decoded_outputs"][i] == c.compute_bits(bits[i])[c.NumWires - nout:]).all(), i
    tinst = d["garbled_tables_instances"].astype(int)
    assert len(tinst) == 16 and d["garbled_tables"].shape[:2] == (16, len(oracle.garble(
        c.Gates, c.NumWires, nin, KEY, rnd[0].tobytes())["slab"]))
    for t, i in enumerate(tinst):
        ref = oracle.garble(c.Gates, c.NumWires, nin, KEY, rnd[i].tobytes())
        assert (d["garbler_R"][i] == words(ref["R"])).all(), i
        assert (d["garbled_tables"][t] == words(ref["slab"])).all(), i
        w = np.zeros(c.NumWires, LABEL)
        w[:nin] = np.where(bits[i].astype(bool), ref["wires"]["l1"][:nin], ref["wires"]["l0"][:nin])
        oracle.eval_(c.Gates, c.NumWires, KEY, w, ref["slab"])
        assert (d["output_labels"][i] == words(w[c.NumWires - nout:])).all(), i
