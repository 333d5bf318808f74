"""The program of the intake and return-label tests (tests/test_gpu_stream_batch_intake.py, tests/test_gpu_stream_batch_return.py):
twelve steps of a few dozen gates in the form of tests/test_gpu_stream_batch.reference, with what the framing can go wrong on —
step 0 has OR, INV and XNOR gates and 16-bit ids, step 1 writes wires above 0xffff (32-bit ids on the wire) that step 2 reads,
step 7 is the in-place update of tests/test_stream_batch_host.alias_gates — and the OpCircuit header of
compiler/ssa/streamer.go:679-693 in front of every block."""
import struct

import numpy as np

import oracle
from mpc_amd.circuit import LABEL, WIRE, Circuit, synthetic_levelised
from tests import keyed_geometry as kg
from tests.test_stream_batch_host import alias_gates

HEADER = 20
OP_CIRCUIT, OP_RETURN = 1, 2
NSTEPS = 12
HIGH = 0x20000  # global ids from here on take 4 bytes on the wire


def make_program():
    """[(circuit, in_, out_)], prim: every step reads primary inputs and outputs of earlier steps"""
    prim = list(range(24))
    steps, known, nxt = [], list(prim), 100
    for k in range(NSTEPS):
        if k == 7:  # in = [0, 1], out = [0, 2]: global 0 and 2 are overwritten in place
            steps.append((Circuit(5, [1, 1], [2], alias_gates(), "alias"), [0, 1], [0, 2]))
            continue
        nin = 8 + 2 * (k % 3)
        c = synthetic_levelised(3, 5 + k % 4, 0.4, seed=200 + k, ninputs=nin, or_frac=0.15 if k % 2 == 0 else 0.0,
                                inv_frac=0.15 if k % 3 == 0 else 0.05, xnor_frac=0.1)
        rng = np.random.default_rng(300 + k)
        src = [w for w in known if w >= HIGH] + list(rng.permutation(known))  # (step 2 reads what step 1 wrote)
        in_ = [int(w) for w in dict.fromkeys(src)][:nin]
        base = HIGH + 16 if k == 1 else nxt
        out_ = [base + j for j in range(c.num_outputs)]
        nxt += 0 if k == 1 else c.num_outputs + 3
        steps.append((c, in_, out_))
        known += out_
    return steps, prim


def header(k, c, in_, out_, op=OP_CIRCUIT):
    return struct.pack(">5I", op, k, c.NumGates, c.NumWires, max(max(in_), max(out_)) + 1)


_refs = {}


def reference(S, keylen=32):
    """the oracle once per S: keys, random streams, per session the framed stream and its message offsets, every program wire of
    the garbler, the evaluator's input bits and labels, the label of every wire it holds at the end, and the plaintext values"""
    from tests.test_gpu_stream_batch import rnd_streams
    if (S, keylen) in _refs:
        return _refs[(S, keylen)]
    steps, prim = make_program()
    keys = kg.edge_keys("stream-batch/intake", S, keylen)
    rnd = rnd_streams("intake/%d" % S, S, len(prim))
    outs = list(dict.fromkeys(o for _, _, out_ in steps for o in out_))
    every = list(dict.fromkeys(prim + outs))
    bits = np.random.default_rng(S + keylen).integers(0, 2, (S, len(prim)), dtype=np.uint8)
    streams, wires, ev, vals = [], {w: np.zeros(S, WIRE) for w in every}, {w: [] for w in every}, []
    inlab = np.zeros((S, len(prim)), LABEL)
    for s in range(S):
        g = oracle.Stream(keys[s].tobytes(), rnd[s].tobytes(), prim)
        e = oracle.StreamEval(keys[s].tobytes())
        for w, b in zip(prim, bits[s]):
            wire = g.get(w)
            inlab[s, prim.index(w)] = wire["l1"] if b else wire["l0"]
            e.set(w, inlab[s, prim.index(w)])
        mine = []
        for c, in_, out_ in steps:
            data = g.garble(c.Gates, c.NumWires, in_, out_)
            assert e.circuit(c.NumGates, c.NumWires, max(max(in_), max(out_)) + 1, data) == len(data)
            mine.append(data)
        streams.append(mine)
        for w in every:
            wires[w][s] = g.get(w)
            ev[w].append(e.get(w))
        mine_vals = {}
        for w in every:  # (the plaintext value of a wire is which of the garbler's two labels the evaluator holds)
            l0, l1 = (int(wires[w][s]["l0"]["d0"]), int(wires[w][s]["l0"]["d1"])), (int(wires[w][s]["l1"]["d0"]), int(wires[w][s]["l1"]["d1"]))
            assert ev[w][s] in (l0, l1), (w, s)
            mine_vals[w] = int(ev[w][s] == l1)
        vals.append(mine_vals)
    hdr = [header(k, *st) for k, st in enumerate(steps)]
    framed = np.stack([np.frombuffer(b"".join(h + blk for h, blk in zip(hdr, streams[s])), np.uint8) for s in range(S)])
    offs = [0]
    for blk in streams[0]:
        offs.append(offs[-1] + HEADER + len(blk))
    _refs[(S, keylen)] = dict(steps=steps, prim=prim, keys=keys, rnd=rnd, streams=streams, wires=wires, outs=outs, every=every,
                              bits=bits, inlab=inlab, ev=ev, vals=vals, hdr=hdr, framed=framed, offs=offs)
    return _refs[(S, keylen)]


def oracle_eval(ref, s, stream):
    """{wire: (d0, d1)} for every program wire after oracle.StreamEval of session s has read `stream`, the framed bytes of
    that session (every message an OpCircuit)"""
    e = oracle.StreamEval(ref["keys"][s].tobytes())
    for w, lab in zip(ref["prim"], ref["inlab"][s]):
        e.set(w, lab)
    stream, at = bytes(stream), 0
    while at < len(stream):
        op, _, ngates, ntmp, nwires = struct.unpack(">5I", stream[at: at + HEADER])
        assert op == OP_CIRCUIT
        at += HEADER + e.circuit(ngates, ntmp, nwires, stream[at + HEADER:])
    return {w: e.get(w) for w in ref["every"]}
