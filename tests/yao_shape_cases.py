"""The circuits, sessions and field-edge predicates of the gc_yao_* shape tests — TEST INFRASTRUCTURE, shared by
tests/test_yao_shape_cases_host.py (which asserts that the chosen inputs hit the edges claimed here, without a GPU),
tests/test_gpu_yao_shapes.py and tests/test_gpu_yao_hostile_shapes.py.

The predicates are pure Python over tests/py_yao_reference.py's geometry: where the 16-byte fields of M1 (table rows, the
garbler's own labels) and the row words of its gates lie against the pieces the M1 kernels cut the message into, and how many
words the message's last line holds.  A session's random bytes depend on the circuit, the key length and the session's index
alone, so session s is the same in every case and its reference is computed once per process."""
import functools

from mpc_amd import circuit as mc
from tests import py_yao_reference as ref
from tests import sha2pc_cases
from tests import yao_cases as cases

DEFAULT_SHAPE = (4, 4096)  # yao.h: kYaoTile, kYaoPieceBytes


@functools.lru_cache(maxsize=None)
def circuit(name):
    """-> (circuit, ng, ne)"""
    if name == "small":
        return sha2pc_cases.small_circuit(3, 9)[0], 3, 9
    if name == "wide":  # the several-piece circuit of tests/test_gpu_yao.py and tests/test_gpu_yao_hostile.py
        return mc.synthetic_levelised(8, 96, 0.5, 21, ninputs=14, or_frac=0.1, inv_frac=0.1), 5, 9
    if name.startswith("and"):  # bits independent ANDs: ngates = nout = ng = ne = bits, two rows a gate
        bits = int(name[3:])
        return mc.bitwise(bits, mc.AND), bits, bits
    raise KeyError(name)


def geometry(name, keylen):
    circ, ng, ne = circuit(name)
    return ref.geometry(circ, ng, ne, keylen)


@functools.lru_cache(maxsize=None)
def session(name, keylen, s):
    return cases.session(geometry(name, keylen), "shapes/%s/%d/%d" % (name, keylen, s))


def sessions(name, keylen, S):
    return [session(name, keylen, s) for s in range(S)]


@functools.lru_cache(maxsize=None)
def reference(name, keylen, s):
    """cases.reference of session s, computed once and shared; nobody writes into it"""
    return cases.reference(circuit(name)[0], geometry(name, keylen), session(name, keylen, s))


# ---- where the fields of M1 lie against pieces of `piece` bytes -----------------------------------------------------------

def row_offsets(g):
    """byte offset in M1 of every table row"""
    return [o + 4 + 16 * r for o, n in zip(ref.gate_offsets(g), g.rows) for r in range(n)]


def label_offsets(g):
    """byte offset in M1 of the garbler's own labels"""
    at_labels = ref.len1(g) - 16 * g.ng
    return [at_labels + 16 * i for i in range(g.ng)]


def crossings(offsets, piece):
    """the 16-byte fields at `offsets` that lie across a piece boundary -> the set of byte counts in the earlier piece"""
    return {piece - o % piece for o in offsets if o // piece != (o + 15) // piece}


def begin_at_a_piece(offsets, piece):
    """the fields that begin exactly where a piece behind the first begins"""
    return [o for o in offsets if o and o % piece == 0]


def gates_first_word(g, piece):
    """gates whose row word is the first word of a piece"""
    return [i for i, o in enumerate(ref.gate_offsets(g)) if o and o % piece == 0]


def gates_last_word(g, piece):
    """gates whose row word is the last word of a piece"""
    return [i for i, o in enumerate(ref.gate_offsets(g)) if o % piece == piece - 4]


def npieces(g, piece):
    return -(-ref.len1(g) // piece)


def tail_words(g):
    """words of the message behind its last whole 16-byte line: what the M1 kernels move as words"""
    return ref.len1(g) % 16 // 4


def last_piece_full(g, piece):
    return ref.len1(g) % piece == 0


def piece_of_gate(g, piece, gate):
    return ref.gate_offsets(g)[gate] // piece


def hostile_gates(g, piece):
    """the gates the hostile M1 test spoils: the last one, a (lower, higher) pair in different pieces, and one whose row
    word is the first word of a piece"""
    first = gates_first_word(g, piece)
    last = len(g.rows) - 1
    return {"last": last, "pair": (first[0] - 1, last - 3), "first_of_piece": first[-1]}


# ---- the directed results of the decode kernels ----------------------------------------------------------------------------

DIRECTED_NOUT = (64, 65, 130)


def directed_values(nout):
    """results that put the highest set bit at the edges of k_yao_m2_decode's 64-output ballots and of M3's length: each
    value once, in the order given"""
    vs = [0, 1, 1 << 7, 1 << 8, (1 << 64) - 1, 1 << 63, 1 << 64, (1 << 64) | 1, 1 << (nout - 1), (1 << nout) - 1]
    out = []
    for v in vs:
        if v < 1 << nout and v not in out:
            out.append(v)
    return out


def directed_sessions(nout):
    """one session per value of an AND of nout bits: the garbler's bits all one, the evaluator's the value's"""
    name, out = "and%d" % nout, []
    for s, v in enumerate(directed_values(nout)):
        ses = dict(session(name, 32, s))
        ses["gbits"], ses["ebits"] = [1] * nout, [v >> i & 1 for i in range(nout)]
        out.append(ses)
    return out


def directed_expectation(nout, v):
    """M3, len3 and the bits of result v straight from Python's integers"""
    n = (v.bit_length() + 7) // 8
    return {"m3": ref.be32(n) + v.to_bytes(n, "big"), "len3": 4 + n, "bits": v.to_bytes((nout + 7) // 8, "little")}
