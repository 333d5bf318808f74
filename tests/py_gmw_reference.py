"""Plain-Python restatement of the reference's GMW party, written from the Go (line numbers of markkurossi/mpc):

* assign_levels_gmw   — (*Circuit).AssignLevels(TargetGMW), circuit/circuit.go:206-254
* run_parties         — (*Network).run's level loop (gmw/network.go:563-624) and andBatchFlush (:660-757) for n parties in
                        one process, broadcastXORs (:790-823) as a plain XOR over the parties' d / e
* triple_batch        — the local arithmetic of tripleBatch (gmw/triples.go:287-466) given the parties' a, b and the
                        bit-COT outputs of every ordered (sender, receiver) pair

Vectors are the Go bit vectors ([]uint64, bit k of word w = element 64 w + k) with a batch axis added as the last numpy axis:
every instance is one independent run of the reference, so the arrays are [words][n].  The engine's layouts are the same.
"""
import numpy as np

from mpc_amd.circuit import AND, INV, XNOR, XOR

U64 = np.uint64
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def assign_levels_gmw(c):
    """circuit.go:206-254 with TargetGMW: a gate's level is the max of its inputs' levels; an AND's output wire is one
    level up, every other output keeps it.  Returns (level of every gate, Stats[NumLevels])."""
    levels = [0] * c.NumWires
    out = []
    mx = 0
    for i0, i1, o, op in zip(c.Gates["in0"].tolist(), c.Gates["in1"].tolist(), c.Gates["out"].tolist(), c.Gates["op"].tolist()):
        level = levels[i0]
        if op != INV:
            level = max(level, levels[i1])
        out.append(level)
        if op == AND:  # circuit.go:228-231
            level += 1
        levels[o] = level
        mx = max(mx, level)
    return out, mx


def buckets(c):
    """network.go:563-576: (ands[level], rest[level]) gate indices in circuit order; numLevels = Stats[NumLevels] + 1"""
    lv, mx = assign_levels_gmw(c)
    n = mx + 1
    ands, rest = [[] for _ in range(n)], [[] for _ in range(n)]
    for g, op in enumerate(c.Gates["op"].tolist()):
        (ands if op == AND else rest)[lv[g]].append(g)
    return ands, rest


def triple_words(c):
    """words per level and first word of every level: TriplePool.Get takes whole words (triples.go:60-90, 130-142)"""
    ands, _ = buckets(c)
    w = [(len(a) + 63) // 64 for a in ands]
    W = [0]
    for x in w:
        W.append(W[-1] + x)
    return w, W[:-1], W[-1]


def pack(bits):
    """[m][n] 0/1 -> [ceil(m/64)][n] u64 (big.Int / []uint64 word order)"""
    bits = np.asarray(bits, np.uint8)
    m, n = bits.shape
    words = (m + 63) // 64
    padded = np.zeros((words * 64, n), U64)
    padded[:m] = bits
    sh = np.arange(64, dtype=U64)[None, :, None]
    return np.bitwise_or.reduce(padded.reshape(words, 64, n) << sh, axis=1)


def unpack(words, m):
    """[words][n] u64 -> [m][n] 0/1"""
    words = np.asarray(words, U64)
    sh = np.arange(64, dtype=U64)[None, :, None]
    bits = ((words[:, None, :] >> sh) & U64(1)).astype(np.uint8).reshape(-1, words.shape[1])
    return bits[:m]


def run_parties(c, input_shares, triples):
    """the online phase of every party.  input_shares[p]: [ceil(ninputs/64)][n] u64 (nw.wires after setWires,
    network.go:560-561); triples[p] = (a, b, c) each [TW][n] u64, level l using words [W_l, W_l + w_l).
    Returns (msgs, outs): msgs[p] = [(level, [2][w][n] d then e)] per AND level (SendBitvec2, peer.go:131-163),
    outs[p] = [ceil(noutputs/64)][n] output shares (network.go:622-624)."""
    P = len(input_shares)
    n = np.asarray(input_shares[0]).shape[1]
    ands, rest = buckets(c)
    w_of, W_of, _ = triple_words(c)
    gin0, gin1, gout, gop = (c.Gates[k].tolist() for k in ("in0", "in1", "out", "op"))
    wires = []
    for p in range(P):
        wv = np.zeros((c.NumWires, n), np.uint8)
        wv[: c.num_inputs] = unpack(input_shares[p], c.num_inputs)
        wires.append(wv)
    msgs = [[] for _ in range(P)]
    for i in range(len(ands)):
        for p in range(P):  # network.go:580-612
            wv = wires[p]
            for g in rest[i]:
                a = wv[gin0[g]]
                b = wv[gin1[g]] if gop[g] != INV else 0
                if gop[g] == XOR:
                    bit = a ^ b
                elif gop[g] == XNOR:
                    bit = a ^ b ^ (1 if p == 0 else 0)
                elif gop[g] == INV:
                    bit = a ^ 1 if p == 0 else a
                else:
                    raise ValueError("gate %d not supported" % gop[g])
                wv[gout[g]] = bit
        batch = ands[i]
        if not batch:  # andBatchFlush: len(batch) == 0 -> nothing is sent
            continue
        words, W = w_of[i], W_of[i]
        ds, es = [], []
        for p in range(P):  # step 1: d = x ^ a, e = y ^ b; bits past len(batch) stay 0 before the XOR (network.go:695-721)
            ta, tb, _ = triples[p]
            x = pack(np.stack([wires[p][gin0[g]] for g in batch]))
            y = pack(np.stack([wires[p][gin1[g]] for g in batch]))
            d = x ^ np.asarray(ta, U64)[W:W + words]
            e = y ^ np.asarray(tb, U64)[W:W + words]
            ds.append(d)
            es.append(e)
            msgs[p].append((i, np.stack([d, e])))
        d_open = np.bitwise_xor.reduce(np.stack(ds), axis=0)  # broadcastXORs: own XOR every peer's (:790-823)
        e_open = np.bitwise_xor.reduce(np.stack(es), axis=0)
        for p in range(P):  # step 3 (:735-756)
            ta, tb, tc = (np.asarray(t, U64)[W:W + words] for t in triples[p])
            z = tc ^ (d_open & tb) ^ (e_open & ta)
            if p == 0:
                z ^= d_open & e_open
            zb = unpack(z, len(batch))
            for k, g in enumerate(batch):  # every AND has read its inputs above; now the outputs
                wires[p][gout[g]] = zb[k]
    outs = [pack(wires[p][c.NumWires - c.num_outputs:]) for p in range(P)]
    return msgs, outs


def plain_bucketed(c, input_bits):
    """plaintext evaluation in the bucketed order (what the XOR of the parties' outputs equals; with wire reuse it can differ
    from circuit order, the order of Circuit.compute_bits)"""
    ands, rest = buckets(c)
    gin0, gin1, gout, gop = (c.Gates[k].tolist() for k in ("in0", "in1", "out", "op"))
    wv = np.zeros(c.NumWires, np.uint8)
    wv[: c.num_inputs] = np.asarray(input_bits, np.uint8) & 1
    for i in range(len(ands)):
        for g in rest[i]:
            a, b = wv[gin0[g]], wv[gin1[g]]
            wv[gout[g]] = a ^ 1 if gop[g] == INV else a ^ b ^ (1 if gop[g] == XNOR else 0)
        vals = [wv[gin0[g]] & wv[gin1[g]] for g in ands[i]]
        for g, v in zip(ands[i], vals):
            wv[gout[g]] = v
    return wv[c.NumWires - c.num_outputs:]


def triple_batch(a, b, cot):
    """tripleBatch's local arithmetic (triples.go:287-466) for every party at once.  a[p], b[p]: [words] u64 (or [words][n]);
    cot[(s, r)] = (delta_bit, s_bits, r_bits): the bit-COT of sender s (peer.iknpS.SendBits) with receiver r
    (peer.iknpR.ReceiveBits, choices b[r]).  Returns (c, sent): c[p] the triple words, sent[(s, r)] = (u, v), the vectors
    the sender sends (u = a ^ Delta, :340-352) and receives (v = b of the receiver, :355-359, :392-399)."""
    P = len(a)
    a = [np.asarray(x, U64) for x in a]
    b = [np.asarray(x, U64) for x in b]
    c = [a[p] & b[p] for p in range(P)]  # local term (:312-315)
    sent = {}
    for p in range(P):
        for q in range(P):
            if q == p:
                continue
            # self = p as sender to q (term "a_self & b_peer"), and as receiver from q; the Go orders the two by id
            # (:333-455) but the XOR folds commute
            delta, s_bits, _ = cot[(p, q)]
            u = a[p] ^ (ONES if delta else U64(0))  # :340-349
            v = b[q]
            c[p] = c[p] ^ np.asarray(s_bits, U64) ^ (u & v)  # :362-364
            sent[(p, q)] = (u, v)
            _, _, r_bits = cot[(q, p)]
            c[p] = c[p] ^ np.asarray(r_bits, U64)  # :387-389
    return c, sent


def ideal_cot(rng, b, P, shape):
    """an ideal bit-COT for every ordered pair: s random, r = s ^ (choice & Delta0) (bitcot_test.go's correlation)"""
    cot = {}
    for s in range(P):
        for r in range(P):
            if s == r:
                continue
            delta = int(rng.integers(0, 2))
            sb = rng.integers(0, 2 ** 63, shape, dtype=np.int64).astype(U64) ^ (rng.integers(0, 2, shape).astype(U64) << U64(63))
            rb = sb ^ (np.asarray(b[r], U64) & (ONES if delta else U64(0)))
            cot[(s, r)] = (delta, sb, rb)
    return cot


def beaver_triples(rng, P, tw, n):
    """random valid triples for P parties: (+)c = ((+)a) & ((+)b), shares uniform"""
    def r():
        return rng.integers(0, 2 ** 63, (tw, n), dtype=np.int64).astype(U64) ^ (rng.integers(0, 2, (tw, n)).astype(U64) << U64(63))
    a = [r() for _ in range(P)]
    b = [r() for _ in range(P)]
    c = [r() for _ in range(P)]
    xa = np.bitwise_xor.reduce(np.stack(a), axis=0) if tw else np.zeros((0, n), U64)
    xb = np.bitwise_xor.reduce(np.stack(b), axis=0) if tw else np.zeros((0, n), U64)
    rest = np.bitwise_xor.reduce(np.stack(c[1:]), axis=0) if tw else np.zeros((0, n), U64)
    c[0] = (xa & xb) ^ rest
    return list(zip(a, b, c))


def share_inputs(rng, c, bits, P):
    """XOR shares of the input bits [n][ninputs] for P parties: [ceil(ninputs/64)][n] u64 each"""
    bits = np.asarray(bits, np.uint8)
    n = bits.shape[0]
    shares = [rng.integers(0, 2, (n, c.num_inputs)).astype(np.uint8) for _ in range(P - 1)]
    last = bits.copy()
    for s in shares:
        last ^= s
    shares.append(last)
    return [pack(s.T) if c.num_inputs else np.zeros((0, n), U64) for s in shares]


def fuzz_circuit(rng, ninputs, ngates, reuse, nargs=2, p_and=0.3):
    """random XOR / XNOR / AND / INV circuit (no OR: GMW has none) whose gates may overwrite earlier wires (the parsers allow
    it, parser.go:38-44); inputs split over `nargs` arguments"""
    from mpc_amd.circuit import GATE, Circuit
    gates = np.zeros(ngates, GATE)
    nw = ninputs
    live = list(range(ninputs))
    for i in range(ngates):
        a = live[int(rng.integers(max(0, len(live) - 16), len(live)))] if rng.random() < 0.7 else live[int(rng.integers(0, len(live)))]
        b = live[int(rng.integers(0, len(live)))]
        r = rng.random()
        op = AND if r < p_and else INV if r < p_and + 0.1 else XNOR if r < p_and + 0.2 else XOR
        if nw > ninputs and rng.random() < reuse:
            out = int(rng.integers(ninputs, nw))
        else:
            out = nw
            nw += 1
            live.append(out)
        gates[i] = (a, 0 if op == INV else b, out, op, 0)
    nout = min(int(rng.integers(1, 80)), nw)
    sizes = [ninputs // nargs] * (nargs - 1)
    sizes.append(ninputs - sum(sizes))
    return Circuit(nw, sizes, [nout], gates)
