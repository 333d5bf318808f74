"""The generators of tests/stream_eval_dev_cases.py against the oracle alone (no GPU): every script is what it claims to be —
the oracle's evaluator takes every block the GPU test expects to be taken, refuses (or the reference would index beyond its
store at) exactly the ones it expects to be refused, the buffers and counts sit on the intended side of every limit, every
changed byte is where it was meant to be — so that tests/test_gpu_stream_eval_device.py cannot pass vacuously."""
import pytest

import oracle
from mpc_amd.circuit import AND, XOR
from tests import stream_eval_dev_cases as cases

K = cases.source_constants()


def _walks(case):
    return [w for s in case.steps if s.kind == "buf" for w in s.expect["walk"]]


def _bufs(case):
    return [s for s in case.steps if s.kind == "buf"]


def test_constants_are_the_sources():
    assert K["kUniqLds"] >= 2 and K["kUniqLds"] % 2 == 0
    assert K["kMinDevBuffer"] > 0 and K["min_items"] >= 2 and K["kSkelVariants"] >= 2


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_script_against_the_oracle(name):
    case = cases.CASES[name]()
    oe = oracle.StreamEval(case.key)
    for w, lab in case.first.items():
        oe.set(w, lab)
    seen = set()
    for s in case.steps:
        for b in s.blocks:
            assert all(w < b.nwires for w in b.in_ + b.out_ + b.watch)
            if b.tamper is None:
                assert b.raw == b.clean
            else:
                assert b.raw != b.clean and len(b.raw) == len(b.clean)
        for b in s.blocks[:s.taken]:
            assert not b.ident().beyond
            assert oe.circuit(b.c.NumGates, b.c.NumWires, b.nwires, b.raw) == len(b.raw), (s.note, b.name)
        if s.kind == "one":
            # handed over alone: first sight of a pattern, or a known one brought to the front
            assert (s.expect["parsed"], s.expect["matched"]) == ((1, 0) if s.expect["how"] == "parse" else (0, 1))
            assert (s.expect["how"] == "parse") == (not any(b.ident().same(o) for b in s.blocks for o in seen))
        else:
            e = s.expect
            assert e["dev"] + e["fallbacks"] == e["guessed"] or e["error"]
            assert e["error"] == (s.taken < len(s.blocks) and not e["more"])
            if e["error"]:
                # the block the call stops at: the oracle's loop does not take it as it stands — it names a wire beyond the
                # numWires of its header, where the reference indexes beyond its store (tests/hostile_fuzz.py: stricter)
                bad = s.blocks[s.taken]
                assert bad.tamper[0] == "beyond" and bad.ident().beyond
                assert any(v >= bad.nwires for _, _, v in cases.global_fields(bad.raw, bad.c.NumGates))
            if e["more"]:
                cut = s.blocks[s.taken]
                assert len(s.data) < sum(20 + len(b.raw) for b in s.blocks[:s.taken + 1])
                assert not cut.ident().beyond
            # nothing else of the buffer is refused
            assert all(not b.ident().beyond for b in s.blocks if b.tamper is None or b.tamper[0] != "beyond")
        seen.update(b.ident() for b in s.blocks[:s.taken])
    for s in _bufs(case):  # the framing: headers where the lengths say, the next operation's code behind the last block
        if not s.expect["more"]:
            assert len(s.data) == sum(20 + len(b.raw) for b in s.blocks) + 4 and s.data[-4:] == b"\0\0\0\2"


def _patterns(case, upto):
    out = {}
    for s in case.steps[:upto]:
        assert s.kind == "one" and s.expect["how"] == "parse"
        out[s.blocks[0].name] = s.blocks[0].ident()
    return out


@pytest.mark.parametrize("name,count", [("mates", 5), ("full_table", K["kSkelVariants"]), ("eviction", K["kSkelVariants"] + 1),
                                        ("widths", 2)])
def test_patterns_are_mates_of_one_shape(name, count):
    """the same key, length and bytes outside ids and rows; pairwise different repeat patterns"""
    case = cases.CASES[name]()
    pats = _patterns(case, count)
    assert len(pats) == count
    ids = list(pats.values())
    assert len({(i.key, i.nbytes, i.shape) for i in ids}) == 1
    assert len({i.canon for i in ids}) == count
    for s in case.steps:
        for b in s.blocks:
            assert (b.ident().key, b.ident().nbytes, b.ident().shape) == (ids[0].key, ids[0].nbytes, ids[0].shape)
    if name != "widths":
        assert ids[0].id_widths == {2}
    else:
        assert ids[0].id_widths == {2, 4}  # 16-bit and 32-bit records in one block, global ids in both
        b = case.steps[0].blocks[0]
        assert min(b.in_) <= 0xffff < max(b.in_) and min(b.out_) <= 0xffff < max(b.out_)


def test_mates_buffers_guess_wrong_both_ways():
    case = cases.case_mates()
    walks = _walks(case)
    pats = _patterns(case, 5)
    nu = {n: i.nuniq for n, i in pats.items()}
    assert nu["adjacent"] == nu["far"] == nu["distinct"] - 1 and nu["several"] == nu["distinct"] - 3
    # the finer pattern guessed for a coarser block (only the distinctness loop refuses the guess): with the two equal ids
    # next to each other among the first occurrences, and as far apart as the inputs get
    for coarse in ("adjacent", "far", "several", "outin"):
        assert ("distinct", coarse, "adopted mate") in walks
    # ... and a coarser one guessed for the finer block (only the gf_canon compare refuses the guess)
    assert ("adjacent", "distinct", "adopted mate") in walks and ("outin", "distinct", "adopted mate") in walks
    for s in _bufs(case):
        names = [b.name for b in s.blocks]
        assert all(a != b for a, b in zip(names, names[1:]))
        assert len(s.data) >= K["kMinDevBuffer"] and len(s.blocks) >= 16
        e = s.expect
        assert (e["dev"], e["fallbacks"], e["parsed"]) == (len(s.blocks), 0, 0)


def test_first_occurrences_of_the_adjacent_pattern():
    """in the `adjacent` pattern the two inputs a block names first are one wire: in the all-distinct skeleton's list of first
    occurrences they are entries 0 and 1"""
    case = cases.case_mates()
    d, a = case.steps[0].blocks[0], case.steps[1].blocks[0]
    fd = [v for _, _, v in cases.global_fields(d.raw, 240)]
    fa = [v for _, _, v in cases.global_fields(a.raw, 240)]
    firsts = list(dict.fromkeys(fd))
    n1 = fd.index(firsts[1])
    assert fa[n1] == fa[0] and fd[n1] != fd[0]


def test_full_table_and_eviction_scripts():
    cap = K["kSkelVariants"]
    full = cases.case_full_table()
    assert [s.kind for s in full.steps] == ["one"] * cap + ["buf"] * 3
    for s in _bufs(full):
        assert sorted(b.name for b in s.blocks) == sorted(st.blocks[0].name for st in full.steps[:cap])
        e = s.expect
        assert (e["dev"], e["fallbacks"], e["parsed"], e["guessed"]) == (cap, 0, 0, cap) and len(s.data) >= K["kMinDevBuffer"]
    orders = [[b.name for b in s.blocks] for s in _bufs(full)]
    assert orders[1] == orders[0][::-1] and orders[2] not in (orders[0], orders[1])
    ev = cases.case_eviction()
    a, b, c = _bufs(ev)
    assert len({x.name for x in a.blocks}) == len(a.blocks) == cap + 1
    hows = [w[2] for w in a.expect["walk"]]
    assert "mate gone" in hows and "refused" in hows and a.expect["parsed"] >= 1
    hows = [w[2] for w in b.expect["walk"]]
    assert hows[:cap - 1] == ["adopted mate"] * (cap - 1) and hows[cap - 1] == "refused" and "guess gone" in hows[cap:]
    assert b.expect["parsed"] == 2  # the two patterns that were never live
    for s in (a, b, c):
        assert s.expect["dev"] + s.expect["fallbacks"] == s.expect["guessed"] == len(s.blocks)
    assert (c.expect["dev"], c.expect["fallbacks"]) == (cap, 0)


def test_uniq_edge_script():
    case = cases.case_uniq_edge()
    ones = [s for s in case.steps if s.kind == "one"]
    assert [s.blocks[0].ident().nuniq for s in ones] == [K["kUniqLds"] - 1, K["kUniqLds"], K["kUniqLds"] + 1]
    for s in ones:
        b = s.blocks[0]
        assert len(b.raw) > 32 << 10 and b.ident().id_widths == {4}
        ops = [op for _, op, _, _, _ in cases.records(b.raw, b.c.NumGates)]
        assert ops.count(AND) >= 40 and ops.count(XOR) == len(ops) - ops.count(AND)
        used = {v for _, _, v in cases.global_fields(b.raw, b.c.NumGates)}
        assert used == set(b.in_) | set(b.out_)  # every input is read
    bufs = _bufs(case)
    few = K["min_items"]
    for s, (dev, fb) in zip(bufs[:3], [(few, 0), (few, 0), (0, few)]):
        e = s.expect
        assert len(s.blocks) == few and (e["dev"], e["fallbacks"], e["parsed"], e["matched"]) == (dev, fb, 0, few)
    assert len(bufs[3].blocks) == few - 1 and len(bufs[3].data) >= K["kMinDevBuffer"]
    e = bufs[3].expect
    assert (e["dev"], e["fallbacks"], e["guessed"], e["matched"]) == (0, 0, 0, few - 1)
    # the last id named for the first time is the id named first
    s = bufs[4]
    b = s.blocks[2]
    f = [v for _, _, v in cases.global_fields(b.raw, b.c.NumGates)]
    assert f[-1] == f[0] and f.count(f[-1]) == 3 and b.ident().nuniq == K["kUniqLds"] - 1
    clean = [v for _, _, v in cases.global_fields(s.blocks[0].raw, b.c.NumGates)]
    assert clean.count(clean[-1]) == 1 and len(set(clean)) == K["kUniqLds"]
    e = s.expect
    assert (e["dev"], e["fallbacks"], e["parsed"]) == (len(s.blocks) - 1, 1, 1)
    e = bufs[5].expect
    assert (e["dev"], e["fallbacks"], e["parsed"]) == (len(bufs[5].blocks), 0, 0)
    # two NEIGHBOURS among the first occurrences name one wire, the all-distinct pattern is the guess, and the block means
    # something else under it: gates 1 and 2 read what gate 0 wrote
    s = bufs[6]
    b = s.blocks[1]
    f = [v for _, _, v in cases.global_fields(b.raw, b.c.NumGates)]
    firsts = list(dict.fromkeys(clean))
    assert clean.index(firsts[3]) == 4 and f[4] == f[2] == b.out_[0] and clean[2] == firsts[2] and f[6] == f[2]
    assert ("uniq+0", "out0 on in2", "refused") in s.expect["walk"] and b.out_[1] in b.watch and b.out_[2] in b.watch
    e = s.expect
    assert (e["dev"], e["fallbacks"], e["parsed"]) == (len(s.blocks) - 1, 1, 1)


def test_compare_regions_script():
    case = cases.case_compare_regions()
    bufs = _bufs(case)
    lane16 = 16 * 512
    sides = []
    for s in bufs[:-1]:
        t = [b for b in s.blocks if b.tamper]
        assert len(t) == 1 and len(s.blocks) > K["min_items"]
        b = t[0]
        kind, pos, (side, at) = b.tamper
        nbytes = len(b.clean)
        assert nbytes > 2 * 4 * lane16 // 2 and nbytes > (32 << 10) + 32  # the 16-byte loop makes a second trip
        recs = cases.records(b.clean, b.c.NumGates)
        xs = [p0 for p0, op, _, _, _ in recs if op == XOR]
        assert kind == "xor" and pos in xs and b.raw[pos] == b.clean[pos] | 1
        assert [i for i in range(nbytes) if b.raw[i] != b.clean[i]] == [pos]
        if side == "first":
            assert pos == xs[0] and pos < 64
        elif side == "below":  # the last XOR in front of the boundary ...
            assert pos < at and not [p for p in xs if pos < p < at] and at - pos <= 64
        elif side == "from":   # ... and the first one at or behind it
            assert pos >= at and not [p for p in xs if at <= p < pos] and pos - at <= 64
        else:
            assert nbytes & 15 and pos >= (nbytes & ~15)  # in the bytes behind the last whole 16
        sides.append((side, at))
        e = s.expect
        assert (e["dev"], e["fallbacks"], e["parsed"], e["guessed"]) == (len(s.blocks) - 1, 1, 1, len(s.blocks))
    assert sides == [("first", 0)] + [(sd, lane16 * u) for u in (1, 2, 3) for sd in ("below", "from")] + \
        [("below", (32 << 10) + 16), ("from", (32 << 10) + 16), ("tail", None)]
    s = bufs[-1]
    (b,) = [x for x in s.blocks if x.tamper]
    rows = [(rp, n) for _, _, _, rp, n in cases.records(b.clean, b.c.NumGates) if n]
    assert b.tamper[0] == "row" and any(rp <= b.tamper[1] < rp + 16 * n for rp, n in rows)
    assert b.ident().same(s.blocks[0].ident())
    e = s.expect
    assert (e["dev"], e["fallbacks"], e["parsed"]) == (len(s.blocks), 0, 0)


def test_untrusted_ids_script():
    case = cases.case_untrusted_ids()
    bufs = _bufs(case)
    e = bufs[0].expect
    assert (e["dev"], e["fallbacks"], e["parsed"]) == (len(bufs[0].blocks), 0, 0)
    for b in bufs[0].blocks:
        if b.tamper:
            old, new = b.tamper[2]
            ids = {v for _, _, v in cases.global_fields(b.raw, 240)}
            assert new in ids and old not in ids and new < b.nwires and b.ident().same(bufs[0].blocks[0].ident())
            assert new in case.first or new in b.watch
    assert sum(1 for b in bufs[0].blocks if b.tamper) == 2
    for s, hows in ((bufs[1], "beyond"), (bufs[3], "refused")):
        e = s.expect
        assert e["error"] and s.taken == 6 and (e["dev"], e["fallbacks"], e["parsed"]) == (6, 1, 0)
        assert e["walk"][-1][2] == hows
    for s in (bufs[2], bufs[4]):
        e = s.expect
        assert (e["dev"], e["fallbacks"], e["parsed"]) == (len(s.blocks), 0, 0)


def test_thresholds_script():
    case = cases.case_thresholds()
    bufs = _bufs(case)
    kmin, few = K["kMinDevBuffer"], K["min_items"]
    one = 20 + len(case.steps[0].blocks[0].raw)
    short, rest1, exact, rest2 = bufs[:4]
    assert len(short.data) == kmin - 1 and len(exact.data) == kmin
    for s in (short, exact):
        assert s.taken == kmin // one >= few and s.expect["more"] and kmin % one and (kmin - 1) % one
    e = short.expect
    assert (e["dev"], e["fallbacks"], e["guessed"], e["matched"]) == (0, 0, 0, short.taken)
    e = exact.expect
    assert (e["dev"], e["fallbacks"], e["guessed"]) == (exact.taken, 0, exact.taken)
    for s, cut in ((rest1, short), (rest2, exact)):
        assert s.blocks == cut.blocks[cut.taken:] and s.taken == len(s.blocks) and s.expect["dev"] == 0
    a, b, c = bufs[4:]
    run = -(-kmin // one)
    # the device takes the run before the new block; the run behind it only while that is a device-size buffer of its own
    assert [x.name for x in a.blocks] == ["distinct"] * run + ["new5"] + ["distinct"] * run
    e = a.expect
    assert (e["dev"], e["fallbacks"], e["parsed"], e["taken"]) == (2 * run, 0, 1, 2 * run + 1)
    assert run * one + 4 >= kmin > (run // 2) * one + 4
    e = b.expect
    assert (e["dev"], e["fallbacks"], e["parsed"], e["matched"], e["taken"]) == (run, 0, 1, run + run // 2, run + run // 2 + 1)
    e = c.expect
    assert len(c.data) >= kmin
    assert (e["dev"], e["fallbacks"], e["parsed"], e["matched"], e["taken"]) == (run, 0, 1, run + few - 1, run + few)
