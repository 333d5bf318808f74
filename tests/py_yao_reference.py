"""The three messages of the reference's 2-party driver restated on Python bytes for a general 2-party circuit and any AES
key length — TEST INFRASTRUCTURE, the reference of tests/test_yao_layout.py, tests/test_gpu_yao.py and
tests/test_gpu_yao_hostile.py.

Restated from circuit/garbler.go:38-180 (Garbler), circuit/evaluator.go:20-157 (Evaluator), circuit/helpers.go:18-27
(BitFromLabel), circuit/ioarg.go:51-65 (IO.Split) and the framing of p2p/protocol.go:216-261: SendUint32 is BE32, SendData
is BE32(len) and the bytes, SendLabel is BE(D0) || BE(D1) (tests/go_transcript.py: label_bytes).  The OT between the two
sides is the caller's, as it is in the engine: the evaluator's side takes the labels the OT delivered.

  M1  garbler -> evaluator   SendData(key), SendUint32(#gates), per gate SendUint32(#rows) and its rows, ng own labels
  M2  evaluator -> garbler   nout output labels
  M3  garbler -> evaluator   SendData(result.Bytes()), output i = bit i of result

Every function works on ONE session and returns its outputs and a verdict: 0, or code | index << 8 for the first check that
fails, in the reference's order.  A bad session's outputs are zero bytes of the right lengths, which is what the engine writes
for it (the reference returns an error and nothing)."""
from collections import namedtuple

import numpy as np

from tests import go_transcript as gt
from tests.py_sha2pc_reference import labels_from_bytes

KEY, GATES, ROWS, LABEL, LENGTH = 1, 2, 3, 4, 5
ROWS_OF_OP = {0: 0, 1: 0, 2: 2, 3: 3, 4: 1}  # XOR, XNOR, AND, OR, INV (circuit/garble.go:199-211)

# rows: the row count of every gate, in gate order
Geometry = namedtuple("Geometry", "ng ne nout keylen rows")


def geometry(circ, ng, ne, keylen):
    assert ng + ne == circ.num_inputs
    return Geometry(ng, ne, circ.num_outputs, keylen, tuple(ROWS_OF_OP[int(op)] for op in circ.Gates["op"]))


def be32(v):
    return int(v).to_bytes(4, "big")


def tables_bytes(g):
    return 4 + 4 * len(g.rows) + 16 * sum(g.rows)


def len1(g):
    return 4 + g.keylen + tables_bytes(g) + 16 * g.ng


def len2(g):
    return 16 * g.nout


def bits_bytes(g):
    return (g.nout + 7) // 8


def slot3(g):
    return 4 + bits_bytes(g)


def verdict(code, index=0):
    return code | index << 8


def gate_offsets(g):
    """byte offset in M1 of every gate's row word"""
    off, out = 4 + g.keylen + 4, []
    for n in g.rows:
        out.append(off)
        off += 4 + 16 * n
    return out


def garbler_send(g, key, rnd, bits, garble):
    """-> (M1, state).  garble(key, rnd) -> (input wires WIRE [ng + ne], output wires WIRE [nout], slab LABEL [rows])"""
    assert len(key) == g.keylen
    win, wout, slab = garble(key, rnd)
    assert len(win) == g.ng + g.ne and len(wout) == g.nout and len(slab) == sum(g.rows)
    lb = gt.label_bytes
    m1 = [be32(len(key)), key, be32(len(g.rows))]
    row = 0
    for n in g.rows:
        m1.append(be32(n))
        m1.append(lb(slab[row:row + n]))
        row += n
    m1 += [lb(win[i]["l1" if bits[i] else "l0"]) for i in range(g.ng)]
    m1 = b"".join(m1)
    assert len(m1) == len1(g)
    return m1, {"ot_wires": win[g.ng:], "out": wout}


def evaluator_accept(g, m1):
    """-> (state, verdict): the key, the slab and the garbler's labels of a well-formed M1"""
    assert len(m1) == len1(g)
    word = lambda off: int.from_bytes(m1[off:off + 4], "big")
    if word(0) != g.keylen:
        return None, verdict(KEY)
    key, off = m1[4:4 + g.keylen], 4 + g.keylen
    if word(off) != len(g.rows):
        return None, verdict(GATES)
    off += 4
    slab = []
    for i, n in enumerate(g.rows):
        if word(off) != n:
            return None, verdict(ROWS, i)
        slab.append(m1[off + 4:off + 4 + 16 * n])
        off += 4 + 16 * n
    return {"key": key, "slab": labels_from_bytes(b"".join(slab)), "glabels": labels_from_bytes(m1[off:off + 16 * g.ng])}, 0


def evaluator_eval(g, state, verdict_of_accept, ot_labels, evaluate):
    """-> (M2, verdict).  evaluate(key, slab LABEL [rows], inputs LABEL [ng + ne]) -> output labels LABEL [nout]"""
    if verdict_of_accept:
        return bytes(len2(g)), verdict_of_accept
    inputs = np.zeros(g.ng + g.ne, state["slab"].dtype)
    inputs[:g.ng] = state["glabels"]
    inputs[g.ng:] = ot_labels
    return gt.label_bytes(evaluate(state["key"], state["slab"], inputs)), 0


def pack_result(g, bits):
    """bits: the engine's array (output i in bit i % 8 of byte i / 8) -> SendData(result.Bytes())"""
    data = int.from_bytes(bits, "little")
    data = data.to_bytes((data.bit_length() + 7) // 8, "big")
    return be32(len(data)) + data


def garbler_result(g, state, m2):
    """-> (M3 over its slot bytes, len3, bits, verdict)"""
    assert len(m2) == len2(g)
    lb = gt.label_bytes
    bits = bytearray(bits_bytes(g))
    for j in range(g.nout):  # BitFromLabel: L0 is asked first
        l, w = m2[16 * j:16 * j + 16], state["out"][j]
        if l == lb(w["l0"]):
            continue
        if l != lb(w["l1"]):
            return bytes(slot3(g)), 0, bytes(bits_bytes(g)), verdict(LABEL, j)
        bits[j // 8] |= 1 << (j % 8)
    m3 = pack_result(g, bits)
    return m3, len(m3), bytes(bits), 0


def evaluator_result(g, m3, room):
    """m3: the slot's bytes, `room` of them -> (bits, verdict)"""
    n = int.from_bytes(m3[:4], "big")
    if 4 + n > room:
        return bytes(bits_bytes(g)), verdict(LENGTH)
    raw = int.from_bytes(m3[4:4 + n], "big") & ((1 << g.nout) - 1)
    return raw.to_bytes(bits_bytes(g), "little"), 0
