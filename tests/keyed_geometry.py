"""What tile and LDS image a batch of the flattened kernels gets, restated in plain Python, and the circuits, keys and
instance samples that the keyed-kernel tests share (tests/test_keyed_geometry.py on the host, tests/test_gpu_batch_keyed*.py on
the device).

The restatement is written from DESIGN.md (sections 9 and 15) and the LDS map at the head of fused_flat_keyed_kernels.hip, not
by calling the engine's own size functions:

    64 KiB AES table | 256 B column keys | 2 stage buffers of `ustride` uint4 | R[TI] | wires [nls][TI] | keys [TI][15] uint4

    one key per batch:     (4112 + 2 ustride + (nls + 1) TI) * 16 bytes
    one key per instance:  that + 240 TI bytes (15 round keys of AES-256, whatever the key length)
    limit:                 160 KiB

Tile rule (make_geom, schedule 1, flattened kernels): TI = 2^t; t grows while batch >> (t + 1) >= 256 — at least 256 tiles —
up to 6, to 3 when some XOR list of the plan is spread over two lanes, to 2 when over four (parts * TI <= 16, one DPP row);
then, when ONE instance fits (the wires are in LDS at all), t shrinks until the one-key image fits.  The keyed calls take the
tile as it is and refuse the batch when their image does not fit.

The engine supplies only the three figures of a plan that the rule needs: n_flat_slots (gc_plan_info) and the stage stride and
part count (gc_plan_flat_geometry)."""
import numpy as np

from mpc_amd import circuit, engine
from mpc_amd.circuit import AND, GATE, INV, OR, XNOR, XOR, Circuit

LDS_LIMIT = 160 * 1024
FRONT16 = 4112  # uint4 in front of the stage buffers: 64 KiB of AES table + 256 B
KEY_TABLE_BYTES = 240  # per instance of a tile: 15 round keys


def one_key_bytes(nls, ustride, ti):
    return (FRONT16 + 2 * ustride + (nls + 1) * ti) * 16


def keyed_bytes(nls, ustride, ti):
    return one_key_bytes(nls, ustride, ti) + KEY_TABLE_BYTES * ti


def tile_log2(batch, nls, ustride, parts):
    cap = 2 if parts >= 4 else 3 if parts == 2 else 6
    t = 0
    while t < cap and (batch >> (t + 1)) >= 256:
        t += 1
    if one_key_bytes(nls, ustride, 1) <= LDS_LIMIT:
        while t > 0 and one_key_bytes(nls, ustride, 1 << t) > LDS_LIMIT:
            t -= 1
    return t


class Shape:
    """prediction for one (circuit, batch): .ti, .parts, .wires_in_lds, .keyed, .lds (one-key bytes), .keyed_lds"""

    def __init__(self, nls, ustride, parts, batch):
        self.nls, self.ustride, self.parts, self.batch = nls, ustride, parts, batch
        self.ti = 1 << tile_log2(batch, nls, ustride, parts)
        self.lds = one_key_bytes(nls, ustride, self.ti)
        self.keyed_lds = keyed_bytes(nls, ustride, self.ti)
        self.wires_in_lds = self.lds <= LDS_LIMIT
        self.keyed = self.wires_in_lds and self.keyed_lds <= LDS_LIMIT

    def as_tuple(self):
        return self.ti, self.parts, self.keyed


def plan_figures(c):
    """(n_flat_slots, stage stride in uint4, largest part count) of the circuit's plan; host only"""
    p = engine.Plan(c.Gates, c.NumWires, c.num_inputs, c.num_outputs)
    assert p.info.n_flat_slots != 0xFFFFFFFF, "no flattened plan"
    ustride, parts = p.flat_geometry()
    return int(p.info.n_flat_slots), ustride, parts


_figures = {}


def predict(name, batch):
    """Shape of circuit CIRCUITS[name] at `batch` (the plan is built once per name)"""
    if name not in _figures:
        _figures[name] = plan_figures(build(name))
    return Shape(*_figures[name], batch)


def check_batch(b, shape):
    """a device batch got the predicted tile, wire placement and keyed scope"""
    assert b.tile_instances == shape.ti, "tile of %d instances, predicted %d" % (b.tile_instances, shape.ti)
    assert b.lds_wires == shape.wires_in_lds
    assert b.keyed_supported() == shape.keyed


# ---- circuits ---------------------------------------------------------------------------------------------------------


class _Gates:
    def __init__(self, ninputs):
        self.g, self.nw = [], ninputs

    def gate(self, a, b, op):
        self.g.append((int(a), 0 if op == INV else int(b), self.nw, op, 0))
        self.nw += 1
        return self.nw - 1

    def chain(self, terms, xnor=False):
        """XOR of the terms as a chain of gates (the last one an XNOR on request): ONE list of len(terms) terms in the plan"""
        acc = terms[0]
        for i, t in enumerate(terms[1:]):
            acc = self.gate(acc, t, XNOR if xnor and i == len(terms) - 2 else XOR)
        return acc

    def circuit(self, ninputs, noutputs, name):
        return Circuit(self.nw, [ninputs // 2, ninputs - ninputs // 2], [noutputs], np.array(self.g, GATE), name)


def parity_lists(name, ninputs, lens1, lens2, lens_out, seed):
    """XOR lists between hash phases.  Round 1: a list of lens1[j] input wires each (every third ends in an XNOR: kXoRpar),
    feeding AND / OR / INV gates.  Round 2: lists of lens2[j] terms over inputs and those gates' outputs, feeding AND / OR
    gates that are circuit outputs.  Lists of lens_out[j] terms over the same pool are circuit outputs themselves (kXoStore;
    every second an XNOR).  The terms of a list are distinct, so its length in the plan is the length given here."""
    rng = np.random.default_rng(seed)
    b = _Gates(ninputs)
    ops = (AND, OR, INV, AND)
    p = [b.chain(rng.choice(ninputs, k, replace=False), xnor=j % 3 == 1) for j, k in enumerate(lens1)]
    h = [b.gate(p[j], p[(j + 1) % len(p)], ops[j % 4]) for j in range(len(p))]
    pool = np.array(list(range(ninputs)) + h)
    q = [b.chain(rng.choice(pool, k, replace=False), xnor=j % 2 == 1) for j, k in enumerate(lens2)]
    # an output list: all but its last gate now, the last gate among the circuit's last wires
    tails = []
    for j, k in enumerate(lens_out):
        terms = rng.choice(pool, k, replace=False)
        tails.append((b.chain(terms[:-1]), terms[-1], XNOR if j % 2 else XOR))
    for j in range(len(q)):
        b.gate(q[j], q[(j + 1) % len(q)], (AND, OR)[j % 2])
    for acc, last, op in tails:
        b.gate(acc, last, op)
    return b.circuit(ninputs, len(q) + len(tails), name)


def lds_edge(n):
    """n inputs that all stay live until a chain of n ANDs, one hash phase each, consumes them one by one behind three
    hash phases (OR, INV, AND): every unit is one gate, so the stage buffers are the smallest there are, and one more
    input is one more live label."""
    b = _Gates(n)
    acc = b.gate(0, 1, OR)
    acc = b.gate(acc, 0, INV)
    acc = b.gate(acc, 2, AND)
    for i in range(n):
        acc = b.gate(acc, i, AND)
    return b.circuit(n, 1, "lds_edge_%d" % n)


# lds_edge: n_flat_slots = n + 3 (n inputs, two labels in flight, the zero slot) and stage stride 4, so the keyed image of a
# tile of one instance is (4112 + 8 + n + 4) * 16 + 240 bytes: exactly the limit for n = 6 101
N_FIT = 6101

CIRCUITS = {
    "adder8": lambda: circuit.adder(8),  # narrow units only
    # 320 ANDs per level: 1 280 garbler blocks per instance, several passes of 1 024 column lanes per unit
    "wide": lambda: circuit.synthetic_levelised(levels=3, width=320, and_frac=1.0, seed=11),
    # every gate kind: the HAS_OR build; odd gate counts leave the last pass of a unit partial
    "mixed": lambda: circuit.synthetic_levelised(levels=3, width=320, and_frac=0.45, seed=12, or_frac=0.2, inv_frac=0.15,
                                                 xnor_frac=0.1),
    # every gate kind with a live set small enough for tiles of 64
    "mixed_small": lambda: circuit.synthetic_levelised(levels=3, width=32, and_frac=0.4, seed=21, ninputs=40, or_frac=0.2,
                                                       inv_frac=0.15, xnor_frac=0.1),
    # lists of 9..16 terms -> two parts: tiles of at most 8, the join_parts<8> branch
    "parity2": lambda: parity_lists("parity2", 40, [12, 9, 16, 3, 10, 5, 13, 2, 11, 16, 9, 7], [9, 4, 14, 16, 2, 12],
                                    [10, 3, 16, 9, 6], seed=31),
    # lists of 17..32 terms -> four parts: tiles of at most 4.  More than 111 of them in round 1, so the lists do not fit
    # one unit (448 items) and a unit breaks between two four-part lists
    "parity4": lambda: parity_lists("parity4", 64, [17 + (5 * j) % 16 for j in range(116)] + [12, 9, 4, 2],
                                    [32, 17, 9, 25, 3, 20], [24, 5, 32, 17, 12, 18], seed=32),
    "edge_fit": lambda: lds_edge(N_FIT),
    "edge_over": lambda: lds_edge(N_FIT + 7),  # one-key fits (up to N_FIT + 15), the key table does not
}


def build(name):
    return CIRCUITS[name]()


# ---- keys -------------------------------------------------------------------------------------------------------------


def edge_keys(tag, batch, keylen):
    """seeded, distinct keys [batch][keylen]: instance 0 all zero, instance 1 all 0xFF; 3 = 2 but for the last byte, 5 = 4 but
    for the first byte (a truncated or mis-strided key read changes an instance that is compared with the oracle: 0..5 are in
    tile 0 or in the sample of every batch that has them)"""
    seed = int.from_bytes(("keyed/" + tag).encode(), "big") % (1 << 63)
    keys = np.random.default_rng(seed).integers(0, 256, (batch, keylen), dtype=np.uint8)
    keys[0] = 0
    if batch > 1:
        keys[1] = 0xFF
    if batch > 3:
        keys[3] = keys[2]
        keys[3, -1] ^= 0x01
    if batch > 5:
        keys[5] = keys[4]
        keys[5, 0] ^= 0x80
    assert len({k.tobytes() for k in keys}) == batch
    return keys


def pool_keys(tag, batch, keylen):
    """(pool [3][keylen], keys [batch][keylen]) with key i = pool[i % 3]: 3 is coprime to every tile width, so the lanes of
    neighbouring instances always hold different keys, and three one-key passes give every instance's expected bytes"""
    pool = edge_keys("pool/" + tag, 3, keylen)
    return pool, pool[np.arange(batch) % 3]


def sample(batch, ti):
    """instances compared with the oracle: tile 0, the last two tiles, every 37th in between, and 0..5 (edge_keys)"""
    ntiles = (batch + ti - 1) // ti
    s = set(range(min(ti, batch))) | set(range(max(0, (ntiles - 2) * ti), batch)) | set(range(0, batch, 37))
    return sorted(s | set(range(min(6, batch))))
