"""Steps of a session-batched streamed program built for the BYTE GEOMETRY of their serialised form, shared by
tests/test_stream_batch_geometry_host.py (which asserts the geometry on the host) and tests/test_gpu_stream_batch_geometry.py.

The serialiser and ingester (k_sb_serialise / k_sb_ingest) cut a step into pieces of PIECE = 4096 bytes; what can go wrong there
depends on where the 16-byte table rows lie against the piece boundaries and on how the step ends.  The sizes are those of the
wire format (tests/hostile_fuzz.parse reads it): a gate is one op byte, 2 or 3 ids of 2 or 4 bytes, 16 bytes per row; XOR and
XNOR have no rows, INV 1, AND 2, OR 3.  With 16-bit ids the gates are 7 (XOR), 21 (INV), 39 (AND) and 55 (OR) bytes long; a gate
that names a global id >= 0x10000 has 4-byte ids.  7, 21, 39, 55 have no common divisor, so a run of gates of any exact byte
length from a few hundred up exists: the builder places chosen gates at chosen offsets and fills the gaps exactly.

Shape of every circuit: NIN inputs, one tmp wire per gate, one output (the last gate, an XOR: the step ends in structure bytes).
Gate g reads the wire of gate g - 4 (an input for g < 4) and, unless it is an INV, either an input ("g": a global id on the
wire) or the wire of gate g - 1 ("t": tmp ids alone, which keep the 16-bit form whatever the global ids are).  Four interleaved
chains, joined by the three XORs at the end: every gate is live and the live set is a handful of wires.

case(name) gives (Circuit, in_, out_) for every name in NAMES; GEOMETRY[name] is what the case claims, PATH[name] the kernel path of
gc_batch_keyed_path it takes at 3, 5 and 67 sessions."""
import numpy as np

import oracle
from mpc_amd.circuit import AND, GATE, INV, OR, XNOR, XOR, Circuit
from mpc_amd.circuit import WIRE
from tests import keyed_geometry as kg

PIECE = 4096
NIN = 4
ROWS = {XOR: 0, XNOR: 0, AND: 2, OR: 3, INV: 1}
TAILS = (0, 1, 2, 3, 5, 15, 16, 17)
SESSIONS = (3, 5, 67)  # every case is inside gc_batch_keyed_supported at these


def gate_bytes(op, kind, g, long_ids):
    """size of gate g on the wire: kind "g" names an input's global id, "t" tmp ids alone, "o" writes the output"""
    nids = 2 if op == INV else 3
    wide = long_ids and (g < 4 or kind == "o" or (kind == "g" and op != INV))
    return 1 + nids * (4 if wide else 2) + 16 * ROWS[op]


def header_bytes(op, kind, g, long_ids):
    return gate_bytes(op, kind, g, long_ids) - 16 * ROWS[op]


def _alphabet(long_ids):
    """gates a gap may be filled with (g >= 4): [(size, op, kind)], at most one per size"""
    ab = [(op, "g") for op in (OR, AND, INV)] + [(XOR, "t")]
    if long_ids:
        ab += [(OR, "t"), (AND, "t"), (XOR, "g")]
    by_size = {}
    for op, kind in ab:
        by_size.setdefault(gate_bytes(op, kind, 4, long_ids), (op, kind))
    return sorted((n, op, kind) for n, (op, kind) in by_size.items())


def fill(nbytes, long_ids, turn=0):
    """[(op, kind)] of exactly nbytes, the fewest gates (a coin change); `turn` rotates which op a tie goes to, so that the
    gaps of one step do not all hold the same gate"""
    ab = _alphabet(long_ids)
    ab = ab[turn % len(ab):] + ab[: turn % len(ab)]
    best = [0] + [None] * nbytes
    how = [None] * (nbytes + 1)
    for n in range(1, nbytes + 1):
        for size, op, kind in ab:
            if size <= n and best[n - size] is not None and (best[n] is None or best[n - size] + 1 < best[n]):
                best[n], how[n] = best[n - size] + 1, (size, op, kind)
    assert best[nbytes] is not None, "no run of gates is %d bytes long" % nbytes
    out = []
    while nbytes:
        size, op, kind = how[nbytes]
        out.append((op, kind))
        nbytes -= size
    return out


def build(anchors, total, long_ids=False, base=0):
    """(Circuit, in_, out_) of exactly `total` serialised bytes.  anchors: [(op, j, off)] ascending — a gate of type op whose
    row j starts at byte off.  Four AND gates in front, XOR XOR XOR(-> the output) behind, exact fills between."""
    seq, pos = [], 0  # (op, kind)

    def put(op, kind):
        nonlocal pos
        pos += gate_bytes(op, kind, len(seq), long_ids)
        seq.append((op, kind))

    for _ in range(4):
        put(AND, "g")
    tail = 2 * gate_bytes(XOR, "t", 9, long_ids) + gate_bytes(XOR, "o", 9, long_ids)
    for turn, (op, j, off) in enumerate(anchors):
        start = off - 16 * j - header_bytes(op, "g", 9, long_ids)
        for f in fill(start - pos, long_ids, turn):
            put(*f)
        put(op, "g")
    for f in fill(total - tail - pos, long_ids, len(anchors)):
        put(*f)
    put(XOR, "t"), put(XOR, "t"), put(XOR, "o")
    assert pos == total
    return circuit_of(seq, base)


def circuit_of(seq, base=0):
    n = len(seq)
    gates = np.zeros(n, GATE)
    for g, (op, kind) in enumerate(seq):
        a = NIN + g - 4 if g >= 4 else g % NIN
        b = 0 if op == INV else (g + 1) % NIN if kind == "g" else NIN + g - 1
        if g >= n - 3:  # the join: ((c1 ^ c2) ^ c3) ^ c4 over the ends of the four chains
            a, b = NIN + g - 4, NIN + g - 1
        gates[g] = (a, b, NIN + g, op, 0)
    c = Circuit(NIN + n, [NIN // 2, NIN - NIN // 2], [1], gates, "geometry")
    return c, [base + 1 + i for i in range(NIN)], [base + 100]


def straddle(long_ids=False):
    """boundaries 1..15: a row that starts d = 1..15 bytes before the boundary (AND, OR and INV rows in turn, the OR's through
    its third row); boundary 16: the two rows of an AND meet on it — one ends there, one starts there.  17 pieces."""
    anchors = []
    for d in range(1, 16):
        op, j = ((AND, 0), (OR, 2), (INV, 0))[d % 3]
        anchors.append((op, j, d * PIECE - d))
    anchors.append((AND, 0, 16 * PIECE - 16))
    return build(anchors, 16 * PIECE + 1234 + 2 * long_ids, long_ids, 0x10000 if long_ids else 0)


def tiny():
    """one short-form XOR into a global wire: 7 bytes"""
    gates = np.zeros(1, GATE)
    gates[0] = (0, 1, 2, XOR, 0)
    return Circuit(3, [1, 1], [1], gates, "tiny"), [1, 2], [100]


def norows():
    """XOR and XNOR alone, 4 200 bytes: two pieces and not one table row"""
    seq = [(XNOR if g % 3 == 1 else XOR, "g" if g % 2 else "t") for g in range(600)]
    seq[0] = (XOR, "g")  # (gate 0 has no gate in front of it)
    return circuit_of(seq)


TAIL_CASES = ["tail%d" % t for t in TAILS] + ["tail2x"]
NAMES = ["straddle", "straddle_long"] + TAIL_CASES + ["tiny", "norows"]
_built = {}


def case(name):
    """(Circuit, in_, out_) of the named case, built once"""
    if name not in _built:
        if name.startswith("straddle"):
            _built[name] = straddle(name.endswith("long"))
        elif name == "tail2x":  # with a row of an OR 9 bytes in front of the one boundary
            _built[name] = build([(OR, 1, PIECE - 9)], 2 * PIECE)
        elif name.startswith("tail"):
            _built[name] = build([], PIECE + int(name[4:]))
        else:
            _built[name] = {"tiny": tiny, "norows": norows}[name]()
    return _built[name]


# name -> nbytes, row count is left to the parse; straddles: {boundary - row offset} the case must reach at the least
GEOMETRY = {"straddle": dict(nbytes=16 * PIECE + 1234, straddles=set(range(1, 16)), ends_on=True, starts_on=True, widths={2}),
            "straddle_long": dict(nbytes=16 * PIECE + 1236, straddles=set(range(1, 16)), ends_on=True, starts_on=True, widths={2, 4}),
            "tiny": dict(nbytes=7, nrows=0), "norows": dict(nbytes=4200, nrows=0),
            "tail2x": dict(nbytes=2 * PIECE, straddles={9})}
GEOMETRY.update({"tail%d" % t: dict(nbytes=PIECE + t) for t in TAILS})
# gc_batch_keyed_path at 3, 5 and 67 sessions: 1 = the wires of a tile in LDS (tests/test_stream_batch_geometry_host.py asserts it)
PATH = {name: 1 for name in NAMES}


def rows_of(parsed):
    """byte offset of every table row of a block, from hostile_fuzz.parse's gates"""
    return [q[6] + 16 * j for q in parsed for j in range(q[7])]


def row_mask(parsed, nbytes):
    """bool [nbytes]: is the byte part of a table row"""
    m = np.zeros(nbytes, bool)
    for off in rows_of(parsed):
        m[off: off + 16] = True
    return m


def straddlers(parsed, nbytes):
    """[(row offset, boundary)] of the rows with bytes on both sides of a piece boundary"""
    out = []
    for off in rows_of(parsed):
        b = (off // PIECE + 1) * PIECE
        if off < b < off + 16 and b < nbytes:
            out.append((off, b))
    return out


_refs = {}


def reference(name, S, keylen=32):
    """the oracle once per (case, S), in the form of tests/test_gpu_stream_batch.reference for a program of this one step"""
    from tests.test_gpu_stream_batch import rnd_streams
    if (name, S, keylen) in _refs:
        return _refs[(name, S, keylen)]
    c, in_, out_ = case(name)
    prim = list(in_)
    keys = kg.edge_keys("stream-batch/geometry/" + name, S, keylen)
    rnd = rnd_streams("geometry/%s/%d" % (name, S), S, len(prim))
    bits = np.random.default_rng(S + len(name)).integers(0, 2, (S, len(prim)), dtype=np.uint8)
    streams, wires, ev = [], {w: np.zeros(S, WIRE) for w in prim + out_}, {o: [] for o in out_}
    for s in range(S):
        g = oracle.Stream(keys[s].tobytes(), rnd[s].tobytes(), prim)
        e = oracle.StreamEval(keys[s].tobytes())
        for w, b in zip(prim, bits[s]):
            wire = g.get(w)
            e.set(w, wire["l1"] if b else wire["l0"])
        data = g.garble(c.Gates, c.NumWires, in_, out_)
        assert e.circuit(c.NumGates, c.NumWires, max(max(in_), max(out_)) + 1, data) == len(data)
        streams.append([data])
        for w in prim + out_:
            wires[w][s] = g.get(w)
        for o in out_:
            ev[o].append(e.get(o))
    _refs[(name, S, keylen)] = dict(steps=[(c, in_, out_)], prim=prim, keys=keys, rnd=rnd, streams=streams, wires=wires, outs=out_,
                                    bits=bits, ev=ev)
    return _refs[(name, S, keylen)]
