"""Host-only generators for the directed tests of the streaming evaluator's DEVICE verdicts (mpc_amd/csrc/stream_eval_dev.cpp:
evdev_blocks guesses where the blocks of a read buffer are, k_eval_verify says for each whether it equals the guessed byte
skeleton, which skeleton of that shape has the repeat pattern of its ids, and what the distinct ids are).

A case is a script for ONE evaluator: blocks handed over one by one (gc_stream_eval_circuit: the host's matcher / parser, which
is where skeletons and their device copies come from) and framed read buffers (gc_stream_eval_blocks).  Every block is the
oracle garbler's (oracle.Stream.garble), possibly with bytes changed afterwards; every step carries the counter deltas the
engine must show, worked out by HostModel below from the code's own rules and constants — never from what the engine gives.
tests/test_stream_eval_dev_cases.py checks the scripts against the oracle on the CPU, tests/test_gpu_stream_eval_device.py runs
them on the GPU."""
import functools
import hashlib
import os
import re
import struct

import numpy as np

import oracle
from mpc_amd.circuit import AND, GATE, INV, XOR, Circuit, synthetic_levelised
from tests.util import drbg

ROWS = {0: 0, 1: 0, 2: 2, 3: 3, 4: 1}  # table rows behind a record: XOR XNOR AND OR INV
GC_E_ARG = -5


# ---- the code's constants ------------------------------------------------------------------------------------------------------


@functools.lru_cache(None)
def source_constants():
    """the limits the cases sit on, read from the sources so that a changed limit moves the cases along: kUniqLds,
    kMinDevBuffer and the fewest blocks worth a device turn (stream_eval_dev.cpp), kSkelVariants (the evaluator's sources)"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpc_amd", "csrc")

    def text(*names):
        out = []
        for n in names:
            with open(os.path.join(csrc, n)) as f:
                out.append(f.read())
        return "\n".join(out)

    def const(src, name):
        m = re.findall(r"^\s*constexpr\s+(?:size_t|uint32_t|unsigned|int)\s+%s\s*=\s*(\d+)(?:\s*<<\s*(\d+))?\s*;" % re.escape(name), src, re.M)
        assert len(m) == 1, "%d definitions of %s" % (len(m), name)
        return int(m[0][0]) << int(m[0][1] or 0)

    dev = text("stream_eval_dev.cpp")
    items = re.findall(r"if \(nitems < (\d+)\) return GC_OK;", dev)
    assert len(items) == 1, "stream_eval_dev.cpp: %d tests of the fewest blocks of a device turn" % len(items)
    return {"kUniqLds": const(dev, "kUniqLds"), "kMinDevBuffer": const(dev, "kMinDevBuffer"), "min_items": int(items[0]),
            "kSkelVariants": const(text("stream_eval.cpp", "stream_eval_internal.h"), "kSkelVariants")}


# ---- the wire format -----------------------------------------------------------------------------------------------------------


def framed_stream(steps, blocks):
    """what the peer's connection carries: per block a 20-byte header (OpCircuit, step, gates, tmp wires, wires) and its bytes,
    then another operation's code"""
    return b"".join(struct.pack(">5I", 1, k, c.NumGates, c.NumWires, max(max(in_), max(out_)) + 1) + bytes(b)
                    for k, ((c, in_, out_), b) in enumerate(zip(steps, blocks))) + struct.pack(">I", 2)


def records(raw, ngates):
    """walk the records of a block (stream_garble.go:391-446: op byte, ids, rows):
    [(position of the op byte, op, [(position, size, names a tmp wire, id) per id], position of the rows, rows)]"""
    out, pos = [], 0
    for _ in range(ngates):
        p0, b = pos, raw[pos]
        op, sz = b & 0x0f, 2 if b & 0x10 else 4
        assert op <= 4, "operation %d at %d" % (op, p0)
        pos += 1
        tmp = [b & 0x80, b & 0x20] if op == INV else [b & 0x80, b & 0x40, b & 0x20]
        ids = []
        for t in tmp:
            ids.append((pos, sz, bool(t), int.from_bytes(raw[pos:pos + sz], "big")))
            pos += sz
        out.append((p0, op, ids, pos, ROWS[op]))
        pos += 16 * ROWS[op]
    assert pos == len(raw), "%d bytes walked of %d" % (pos, len(raw))
    return out


def global_fields(raw, ngates):
    """the global-id fields of a block in stream order: [(position, size, id)]"""
    return [(p, sz, v) for _, _, ids, _, _ in records(raw, ngates) for p, sz, t, v in ids if not t]


class Ident:
    """what the evaluator can tell a block by: its key (gates, tmp wires), its SHAPE — the bytes outside global ids and rows,
    with the layout of both — and the repeat pattern of its global ids (per field, the first field naming the same wire)"""

    def __init__(self, raw, c, nwires):
        self.key = (c.NumGates, c.NumWires)
        self.nbytes = len(raw)
        blank = bytearray(raw)
        first, canon, widths = {}, [], set()
        for p0, op, ids, rpos, rows in records(raw, c.NumGates):
            blank[rpos:rpos + 16 * rows] = bytes(16 * rows)
            for p, sz, t, v in ids:
                if not t:
                    blank[p:p + sz] = bytes(sz)
                    canon.append(first.setdefault(v, len(canon)))
                    widths.add(sz)
        self.shape = hashlib.sha256(bytes(blank)).digest()
        self.canon = tuple(canon)
        self.nuniq = len(first)
        self.id_widths = widths
        self.beyond = any(v >= nwires for v in first)  # names a wire beyond its header's numWires: refused (stricter than the
        #                                                reference's loop by design, see tests/hostile_fuzz.py)

    def same(self, o):
        return (self.key, self.nbytes, self.shape, self.canon) == (o.key, o.nbytes, o.shape, o.canon)


# ---- the model of the host's bookkeeping ---------------------------------------------------------------------------------------


class _Inst:
    def __init__(self, ident, name):
        self.ident, self.name, self.alive = ident, name, True


class HostModel:
    """What gc_stream_eval_blocks / gc_stream_eval_circuit do with a block, as far as the counters show it.  The rules, from
    stream_eval.cpp (eval_block) and stream_eval_dev.cpp (evdev_blocks):

      * per key a list of variants (skeletons), most recent first, at most kSkelVariants of them;
      * the host's path for a block: the first variant that equals it (shape and repeat pattern) is a MATCH and moves to the
        front; none: the block is PARSED, a new variant is inserted at the front and, if the list was full, the one at the
        back is evicted first (it is gone for the device too: its guesses of the buffer in hand are void, a verdict naming it
        is not followed);
      * a read buffer has a device turn at its start and behind every block the host's loop took: it needs kMinDevBuffer bytes
        left and guesses a run of blocks, each as the first variant of its key that fits — here all variants of a key have
        one length, so that is the front of the list AT GUESS TIME, the same for all blocks of the run —, the run ending at the
        first block of an unknown key or cut off by the buffer's end; a run of fewer than `min_items` blocks is left to the host;
      * the device knows the variants alive when the turn began; its verdict on a block is the one variant among them that
        has the guess's shape, the block's shape and the block's repeat pattern, provided that names at most kUniqLds wires;
      * the verdict is followed (the block ADOPTED: a device block, and a match) if the guess and the named variant are still
        alive and no id is beyond the header's numWires; adoption of a variant other than the guess moves it to the front;
      * every other block of the run is a FALLBACK and takes the host's path."""

    def __init__(self, consts=None):
        self.k = consts or source_constants()
        self.lists = {}

    def _host(self, ident, name, r):
        if ident.beyond:  # (no skeleton adopts such ids, the parser refuses them)
            return "error"
        v = self.lists.setdefault(ident.key, [])
        for i, inst in enumerate(v):
            if inst.ident.same(ident):
                v.insert(0, v.pop(i))
                r["matched"] += 1
                return "match"
        if len(v) >= self.k["kSkelVariants"]:
            v.pop().alive = False
        assert all(o.ident.nbytes == ident.nbytes for o in v), "model: the variants of a key have one length"
        v.insert(0, _Inst(ident, name))
        r["parsed"] += 1
        return "parse"

    def one(self, ident, name):
        r = {"parsed": 0, "matched": 0, "dev": 0, "fallbacks": 0}
        r["how"] = self._host(ident, name, r)
        return r

    def buffer(self, blocks, total):
        """blocks: [(ident, name)] as framed in the buffer, of which `total` bytes are handed over"""
        r = {"parsed": 0, "matched": 0, "dev": 0, "fallbacks": 0, "guessed": 0, "taken": 0, "more": False, "error": False,
             "walk": []}  # walk: (guessed variant's name, block's name, what became of the verdict)
        off, pos = [], 0
        for ident, _ in blocks:
            off.append(pos)
            pos += 20 + ident.nbytes
        whole = lambda j: off[j] + 20 + blocks[j][0].nbytes <= total

        def device_turn(i):
            if total - off[i] < self.k["kMinDevBuffer"] or not self.lists:
                return i
            run, j = [], i
            while j < len(blocks) and whole(j) and self.lists.get(blocks[j][0].key):
                g = self.lists[blocks[j][0].key][0]
                assert g.ident.nbytes == blocks[j][0].nbytes, "model: the variants of a key have one length"
                run.append(g)
                j += 1
            if len(run) < self.k["min_items"]:
                return i
            r["guessed"] += len(run)
            known = [inst for v in self.lists.values() for inst in v]
            for j, g in enumerate(run, i):
                ident, name = blocks[j]
                o = None
                if g.ident.shape == ident.shape:
                    o = next((x for x in known if x.ident.same(ident) and ident.nuniq <= self.k["kUniqLds"]), None)
                how = "refused" if o is None else "guess gone" if not g.alive else "mate gone" if not o.alive else \
                    "beyond" if ident.beyond else "adopted" if o is g else "adopted mate"
                r["walk"].append((g.name, name, how))
                if how.startswith("adopted"):
                    r["dev"] += 1
                    r["matched"] += 1
                    v = self.lists[ident.key]
                    if o is not g:
                        v.insert(0, v.pop(v.index(o)))
                else:
                    r["fallbacks"] += 1
                    if self._host(ident, name, r) == "error":
                        r["error"] = True
                        return j
                r["taken"] += 1
            return i + len(run)

        i = device_turn(0) if blocks else 0
        while not r["error"] and i < len(blocks) and off[i] + 20 <= total:
            if not whole(i):
                assert self.lists.get(blocks[i][0].key), "model: a cut-off block is one of a known key"
                break
            if self._host(blocks[i][0], blocks[i][1], r) == "error":
                r["error"] = True
                break
            r["taken"] += 1
            i += 1
            if i < len(blocks):
                i = device_turn(i)
        r["more"] = not r["error"] and i < len(blocks)
        return r


# ---- scripts -------------------------------------------------------------------------------------------------------------------


class Block:
    def __init__(self, c, in_, out_, raw, name, watch):
        self.c, self.in_, self.out_, self.name = c, list(in_), list(out_), name
        self.nwires = max(max(in_), max(out_)) + 1
        self.clean = raw      # the garbler's bytes
        self.raw = raw        # ... and what the evaluators get
        self.watch = list(watch)  # wires compared behind the step
        self.tamper = None    # (kind, position, where it was meant to land)

    def ident(self):
        if getattr(self, "_ident", (None,))[0] is not self.raw:
            self._ident = (self.raw, Ident(self.raw, self.c, self.nwires))
        return self._ident[1]

    def changed(self, raw, tamper, watch=()):
        assert len(raw) == len(self.raw)
        self.raw, self.tamper = bytes(raw), tamper
        self.watch += list(watch)
        return self


class Step:
    """kind "one": blocks[0] through gc_stream_eval_circuit; "buf": `data` through gc_stream_eval_blocks, of which the call
    takes blocks[:taken]; expect: the deltas of (parsed, matched) and (device blocks, fallbacks) and, for a buffer, the blocks
    guessed, `more`, `error` and the model's walk"""

    def __init__(self, kind, blocks, data, expect, note):
        self.kind, self.blocks, self.data, self.expect, self.note = kind, blocks, data, expect, note
        self.taken = expect.get("taken", 1)


class Case:
    def __init__(self, name, prim):
        self.name, self.prim = name, list(prim)
        self.key = drbg(name + "/key", 32)
        self.og = oracle.Stream(self.key, drbg(name + "/rnd", 16 * (len(prim) + 1)), prim)
        bits = np.frombuffer(drbg(name + "/bits", len(prim)), np.uint8) & 1
        self.first = {}  # the evaluators' labels of the primary wires
        for w, b in zip(prim, bits):
            wire = self.og.get(w)
            self.first[w] = (wire["l1"] if b else wire["l0"]).copy()
        self.model = HostModel()
        self.steps = []
        self.n = 0  # blocks garbled so far

    def garble(self, c, in_, out_, name, watch=None):
        raw = self.og.garble(c.Gates, c.NumWires, in_, out_)
        self.n += 1
        return Block(c, in_, out_, raw, name, out_ if watch is None else watch)

    def one(self, b, note=""):
        r = self.model.one(b.ident(), b.name)
        self.steps.append(Step("one", [b], None, r, note))
        return r

    def buf(self, blocks, total=None, note=""):
        data = framed_stream([(b.c, b.in_, b.out_) for b in blocks], [b.raw for b in blocks])
        data = data if total is None else data[:total]
        r = self.model.buffer([(b.ident(), b.name) for b in blocks], len(data))
        self.steps.append(Step("buf", blocks, data, r, note))
        return r

    def rest(self, note=""):
        """what the last buffer left (it was cut): the caller comes back with the bytes from there on"""
        last = self.steps[-1]
        blocks = last.blocks[last.taken:]
        return self.buf(blocks, note=note)

    @property
    def max_data(self):
        return max(len(s.data) for s in self.steps if s.kind == "buf")


# ---- the 240-gate circuit of the host test and its bindings ------------------------------------------------------------------


def small_circuit():
    return synthetic_levelised(6, 40, 0.4, seed=77, ninputs=12, inv_frac=0.1, xnor_frac=0.1)


def first_use_order(c):
    """the circuit's inputs in the order a block names them for the first time"""
    order = []
    for g in c.Gates:
        for w in ([int(g["in0"])] if g["op"] == INV else [int(g["in0"]), int(g["in1"])]):
            if w < c.num_inputs and w not in order:
                order.append(w)
    assert len(order) == c.num_inputs, "every input is read by a gate"
    return order


class SmallBinder:
    """bindings of the small circuit with 16-bit ids: inputs from a pool of primary wires, every block its own output wires;
    a pattern is a list of pairs (i, j) — in[j] = in[i] — and / or "outin": the first output lands on the first input's wire"""
    PRIM = list(range(64))
    OUT0, STRIDE = 1000, 48  # (8 wires behind every block's outputs stay free)

    def __init__(self, case, c=None):
        self.case, self.c = case, c or small_circuit()

    def wires(self, k, pattern):
        in_ = [self.PRIM[(7 * k + i) % len(self.PRIM)] for i in range(self.c.num_inputs)]
        out_ = [self.OUT0 + self.STRIDE * k + i for i in range(self.c.num_outputs)]
        for p in pattern:
            if p == "outin":
                out_[0] = in_[0]
            else:
                in_[p[1]] = in_[p[0]]
        return in_, out_

    def block(self, name, pattern):
        in_, out_ = self.wires(self.case.n, pattern)
        return self.case.garble(self.c, in_, out_, name)


def pair_patterns(c):
    """all patterns `in[j] = in[i]` of a circuit, in a fixed shuffled order"""
    pairs = [(i, j) for i in range(c.num_inputs) for j in range(i + 1, c.num_inputs)]
    np.random.default_rng(5).shuffle(pairs)
    return [("p%d_%d" % p, [tuple(int(x) for x in p)]) for p in pairs]


@functools.lru_cache(None)
def case_mates():
    """1. mates of one shape, wrong guesses in both directions: the patterns differ only in which ids repeat"""
    case = Case("evdev/mates", SmallBinder.PRIM)
    sb = SmallBinder(case)
    order = first_use_order(sb.c)
    pats = {"distinct": [],
            "adjacent": [(order[0], order[1])],   # the two inputs named first: neighbours among the first occurrences
            "far": [(order[0], order[-1])],       # the input named first and the one named last
            "several": [(order[2], order[5]), (order[3], order[7]), (order[4], order[9])],
            "outin": ["outin"]}
    for name, p in pats.items():
        case.one(sb.block(name, p), "first sight")
    mixes = [("distinct", "adjacent far several outin adjacent distinct far outin several distinct adjacent several far outin distinct far"),
             ("adjacent", "distinct far distinct several outin distinct adjacent distinct outin far several adjacent distinct several far outin"),
             ("outin", "far adjacent several distinct outin adjacent far several distinct far outin several adjacent distinct several outin distinct")]
    for front, mix in mixes:
        # the pattern the next buffer's blocks are guessed to have: the one the host matched last
        case.one(sb.block(front, pats[front]), "to the front: the guess of the buffer behind it")
        case.buf([sb.block(n, pats[n]) for n in mix.split()])
    return case


def _variants_intro(case, sb, n):
    pats = pair_patterns(sb.c)
    assert len(pats) >= n + 3
    for name, p in pats[:n]:
        case.one(sb.block(name, p), "first sight")
    return pats


@functools.lru_cache(None)
def case_full_table():
    """2. exactly kSkelVariants patterns of one shape: forward, reverse, shuffled"""
    cap = source_constants()["kSkelVariants"]
    case = Case("evdev/full", SmallBinder.PRIM)
    sb = SmallBinder(case)
    pats = _variants_intro(case, sb, cap)[:cap]
    shuffled = list(pats)
    np.random.default_rng(11).shuffle(shuffled)
    for order in (pats, pats[::-1], shuffled):
        case.buf([sb.block(n, p) for n, p in order])
    return case


@functools.lru_cache(None)
def case_eviction():
    """3. one pattern more than the table holds, and patterns that arrive inside a buffer"""
    cap = source_constants()["kSkelVariants"]
    case = Case("evdev/evict", SmallBinder.PRIM)
    sb = SmallBinder(case)
    pats = _variants_intro(case, sb, cap)
    by_name = dict(pats)
    case.one(sb.block(*pats[cap]), "one more than the table holds: the least recently used variant goes")
    # every pattern once: the evicted one in the middle of live ones, then the ones ITS parse evicts in turn
    order = [5, 0, 1, 2, cap, cap - 1] + [k for k in range(3, cap - 1) if k != 5]
    assert sorted(order) == list(range(cap + 1))
    case.buf([sb.block(*pats[k]) for k in order], note="all of them once")
    # every live variant but the guess is adopted in turn, which leaves the guess at the back; the new pattern that follows
    # evicts it while the verdicts on the blocks behind are pending; then another new one
    live = [inst.name for inst in case.model.lists[sb.c.NumGates, sb.c.NumWires]]
    seq = live[:0:-1] + [pats[cap + 1][0]] + live[1:4] + [pats[cap + 2][0]] + live[4:6]
    case.buf([sb.block(n, by_name[n]) for n in seq], note="new patterns inside the buffer")
    live = [inst.name for inst in case.model.lists[sb.c.NumGates, sb.c.NumWires]]
    case.buf([sb.block(n, by_name[n]) for n in live[::-1]], note="the live ones")
    return case


@functools.lru_cache(None)
def case_widths():
    """4. ids on both sides of 0xffff inside one block: 16-bit and 32-bit records, both with global ids"""
    low, high = [0x100 + i for i in range(32)], [0x10000 + i for i in range(32)]
    case = Case("evdev/widths", low + high)
    c = small_circuit()
    order = [w for w in first_use_order(c) if w < 6]

    def block(name, pattern):
        k = case.n
        in_ = [(low if i < 6 else high)[(5 * k + i) % 32] for i in range(c.num_inputs)]
        half = c.num_outputs // 2
        out_ = [0xf000 + 24 * k + i for i in range(half)] + [0x18000 + 24 * k + i for i in range(c.num_outputs - half)]
        for i, j in pattern:
            in_[j] = in_[i]
        return case.garble(c, in_, out_, name)

    pats = {"distinct": [], "repeat": [(order[0], order[1])]}  # (both 16-bit: the layout stays)
    for name, p in pats.items():
        case.one(block(name, p), "first sight")
    case.buf([block(n, pats[n]) for n in ("distinct repeat " * 8).split()])
    case.buf([block(n, pats[n]) for n in ("repeat distinct " * 8).split()])
    return case


# ---- one-level circuits that name kUniqLds wires, give or take one -----------------------------------------------------------


def ring_circuit(nin, nout):
    """out_j = in_j OP in_(j + 1 mod nin): every input is read, every 97th gate is an AND (the blocks carry rows)"""
    g = np.zeros(nout, GATE)
    j = np.arange(nout)
    g["in0"], g["in1"], g["out"] = j % nin, (j + 1) % nin, nin + j
    g["op"] = np.where(j % 97 == 0, AND, XOR)
    return Circuit(nin + nout, [nin // 2, nin - nin // 2], [nout], g, "ring_%d_%d" % (nin, nout))


class RingBinder:
    """32-bit ids throughout (13 bytes per record: a block of 4 096 gates is 54 KB) — or, with `tail`, the LAST gate's three
    wires below 0x10000: its record is the 7-byte form, the block's length no multiple of 16, and that record's op byte lies in
    the bytes behind the last whole 16"""
    LOW = [0x10 + i for i in range(8)]

    def __init__(self, case, nout):
        self.case, self.nout = case, nout
        self.pool = [0x20000 + i for i in range(nout + 40)]

    def block(self, c, name, tail=False, last_on_first=False, out0_on_in2=False):
        k = self.case.n
        in_ = [self.pool[(3 * k + i) % len(self.pool)] for i in range(c.num_inputs)]
        out_ = [0x40000 + self.nout * k + j for j in range(self.nout)]
        if tail:
            in_[-1], in_[0], out_[-1] = self.LOW[(2 * k) % 8], self.LOW[(2 * k + 1) % 8], 0x1000 + k
        if last_on_first:
            out_[-1] = in_[0]  # the id named last for the first time equals the one named first
        if out0_on_in2:
            # first occurrences come in the order in_0 in_1 out_0 in_2 out_1 ...: NEIGHBOURS name one wire, and gates 1 and 2
            # read what gate 0 wrote — under the skeleton of the all-distinct binding they would read the old label
            out_[0] = in_[2]
        watch = out_[:4] + out_[4::127] + out_[-2:]
        return self.case.garble(c, in_, out_, name, watch)


@functools.lru_cache(None)
def case_uniq_edge():
    """5. blocks that name kUniqLds - 1, kUniqLds, kUniqLds + 1 distinct wires; with them the 4-block threshold (8.)"""
    k = source_constants()
    nout = k["kUniqLds"] // 2
    rb = RingBinder(None, nout)
    case = rb.case = Case("evdev/uniq", rb.pool)
    few = k["min_items"]
    circs = {d: ring_circuit(nout + d, nout) for d in (-1, 0, 1)}
    for d, c in circs.items():
        case.one(rb.block(c, "uniq%+d" % d), "first sight")
        case.buf([rb.block(c, "uniq%+d" % d) for _ in range(few)], note="the fewest blocks of a device turn")
    case.buf([rb.block(circs[0], "uniq+0") for _ in range(few - 1)], note="one block fewer: the host's")
    blocks = [rb.block(circs[0], "uniq+0") for _ in range(few + 1)]
    blocks[2] = rb.block(circs[0], "last on first", last_on_first=True)
    case.buf(blocks, note="the longest reach of the all-pairs loop")
    case.buf([rb.block(circs[0], n, last_on_first=n != "uniq+0") for n in ("last on first", "uniq+0", "last on first", "uniq+0", "uniq+0")],
             note="both are known now")
    blocks = [rb.block(circs[0], "uniq+0") for _ in range(few + 1)]
    blocks[1] = rb.block(circs[0], "out0 on in2", out0_on_in2=True)
    case.buf(blocks, note="the shortest reach of the all-pairs loop")
    return case


def xor_positions(b):
    return [p0 for p0, op, _, _, _ in records(b.clean, b.c.NumGates) if op == XOR]


@functools.lru_cache(None)
def case_compare_regions():
    """6. one XOR made XNOR in every region of the masked compare; one row byte changed"""
    k = source_constants()
    nout = k["kUniqLds"] // 2
    rb = RingBinder(None, nout)
    case = rb.case = Case("evdev/regions", rb.pool + RingBinder.LOW)
    c = ring_circuit(nout, nout)
    case.one(rb.block(c, "clean", tail=True), "first sight")
    lane16 = 16 * 512  # bytes one trip of the 512 lanes covers per unrolled load (k_eval_verify)
    targets = [("first", 0)]
    for u in (1, 2, 3):
        targets += [("below", lane16 * u), ("from", lane16 * u)]
    targets += [("below", 4 * lane16 + 16), ("from", 4 * lane16 + 16), ("tail", None)]
    nblocks = k["min_items"] + 1
    for n, (side, at) in enumerate(targets):
        if n:
            case.one(rb.block(c, "clean", tail=True), "to the front again: the parsed mutant is the newest variant of the key")
        blocks = [rb.block(c, "clean", tail=True) for _ in range(nblocks)]
        b = blocks[n % nblocks]
        xs = xor_positions(b)
        pos = {"first": xs[0], "tail": xs[-1]}.get(side)
        if side == "below":
            pos = max(p for p in xs if p < at)
        elif side == "from":
            pos = min(p for p in xs if p >= at)
        gate = [p0 for p0, _, _, _, _ in records(b.clean, c.NumGates)].index(pos)
        raw = bytearray(b.clean)
        raw[pos] |= 1  # XOR -> XNOR: the same lengths, another circuit
        b.changed(raw, ("xor", pos, (side, at)), [b.out_[gate]])
        b.name = "xnor@%d" % pos
        case.buf(blocks, note="%s %s" % (side, at))
    case.one(rb.block(c, "clean", tail=True), "to the front again")
    blocks = [rb.block(c, "clean", tail=True) for _ in range(nblocks)]
    b = blocks[1]
    p0, gate = next((rec[3], g) for g, rec in enumerate(records(b.clean, c.NumGates)) if rec[4] and g > nout // 2)
    raw = bytearray(b.clean)
    raw[p0 + 21] ^= 0x40  # a byte of the gate's second row: masked out of the compare
    b.changed(raw, ("row", p0 + 21, None), [b.out_[gate]])
    case.buf(blocks, note="a row byte")
    return case


def _replace_wire(b, wire, new, only_first=False):
    raw = bytearray(b.raw)
    hits = [(p, sz) for p, sz, v in global_fields(b.raw, b.c.NumGates) if v == wire]
    assert hits
    for p, sz in hits[:1] if only_first else hits:
        raw[p:p + sz] = new.to_bytes(sz, "big")
    return raw


@functools.lru_cache(None)
def case_untrusted_ids():
    """7. ids the device reads and the host must check"""
    case = Case("evdev/ids", SmallBinder.PRIM)
    sb = SmallBinder(case)
    case.one(sb.block("distinct", []), "first sight")
    n = 16
    # a fresh wire of the header's range in place of an input / of an output: the same pattern, another binding
    blocks = [sb.block("distinct", []) for _ in range(n)]
    b = blocks[5]
    spare = next(w for w in SmallBinder.PRIM if w not in b.in_)
    b.changed(_replace_wire(b, b.in_[3], spare), ("wire", None, (b.in_[3], spare)))
    b = blocks[9]
    spare = b.out_[0] - 4  # (one of the free wires behind the outputs of the block before)
    b.changed(_replace_wire(b, b.out_[7], spare), ("wire", None, (b.out_[7], spare)), [spare])
    case.buf(blocks, note="fresh wires in range")
    # an id beyond the header's numWires: in every field of that wire (the pattern holds: the verdict names a skeleton, the
    # host's range check must stop it), then in one field only (the pattern breaks as well)
    for only_first in (False, True):
        blocks = [sb.block("distinct", []) for _ in range(n)]
        b = blocks[6]
        assert b.nwires <= 0xfff0
        b.changed(_replace_wire(b, b.in_[2], 0xfff0, only_first), ("beyond", None, (b.in_[2], 0xfff0)))
        b.name = "beyond"
        case.buf(blocks, note="an id beyond numWires")
        case.buf([sb.block("distinct", []) for _ in range(n)], note="the stream goes on")
    return case


@functools.lru_cache(None)
def case_thresholds():
    """8. kMinDevBuffer to the byte, and runs of known blocks around a block met for the first time"""
    k = source_constants()
    case = Case("evdev/thresholds", SmallBinder.PRIM)
    sb = SmallBinder(case)
    case.one(sb.block("distinct", []), "first sight")
    n = 16
    for total in (k["kMinDevBuffer"] - 1, k["kMinDevBuffer"]):
        case.buf([sb.block("distinct", []) for _ in range(n)], total=total, note="%d bytes" % total)
        case.rest("what the cut left")
    run = -(-k["kMinDevBuffer"] // (20 + len(case.steps[0].blocks[0].raw)))  # blocks that make a device-size buffer
    for levels, before, after in ((5, run, run), (4, run, run // 2), (3, k["min_items"] - 1, run)):
        new = SmallBinder(case, synthetic_levelised(levels, 40, 0.4, seed=78, ninputs=12, inv_frac=0.1, xnor_frac=0.1))
        blocks = [sb.block("distinct", []) for _ in range(before)] + [new.block("new%d" % levels, [])] + \
                 [sb.block("distinct", []) for _ in range(after)]
        case.buf(blocks, note="%d known, one new, %d known" % (before, after))
    return case


CASES = {"mates": case_mates, "full_table": case_full_table, "eviction": case_eviction, "widths": case_widths,
         "uniq_edge": case_uniq_edge, "compare_regions": case_compare_regions, "untrusted_ids": case_untrusted_ids,
         "thresholds": case_thresholds}
