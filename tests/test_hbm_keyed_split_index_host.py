"""CPU walk of the index arithmetic of the split form of the keyed HBM-wire kernels (mpc_amd/csrc/hbm_keyed_split.h: which
levels split the workgroup, how many hash waves a level gets, which column lane or free lane a (wave, pass, lane) handles).
The header is compiled into a stand-alone C++ program with the host compiler under AddressSanitizer and UBSan; the program
walks every level of a list of Step shapes the way k_garble_hbm_keyed_split / k_eval_hbm_keyed_split do (wave, role, pass,
lane) and writes one record per lane visited, the one pass past the end that the pipeline's loads run ahead included.  The
records are compared with a model written from col_classify's definition (mpc_amd/csrc/col_lanes.h):

  * every column lane and every free lane of the level is visited exactly once;
  * all lanes of a gate-instance row share wave and pass (the DPP partners of a lane are in its pass);
  * the per-role pass counts match;
  * every idle lane classifies as K_NONE of gate 0: the address it re-reads is the level's first descriptor;
  * H obeys the caps: 16 without free gates, 0 without hashed gates, never more waves than the level has lanes for, at least
    one and at most eight free waves under the rule, the fixed value otherwise.

Shapes: TI 1, 2, 4, 64; both roles; with and without OR; levels of 1 024 lanes and of the next width above; free gates only;
hashed gates only; fewer hash lanes than one wave beside many free lanes; a last partial pass in each role; every fixed H."""
import os
import subprocess

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpc_amd", "csrc")
THREADS, WAVES, IDLE = 1024, 16, 0xFFFFFFFF
SINGLE, HASH, FREE = 0, 1, 2

PROGRAM = r"""
#include <cstdio>
#include <vector>

#include "hbm_keyed_split.h"

using namespace gc;

// argv[1]: output file.  "ti_log2 eval tune first count nonfree n_and n_or n_inv" on stdin, one level per line -> a header record
// {wide, H, e_hash, n_free, hash passes, free passes} and one record {role, wave, pass, lane, J or u, 0} per lane visited
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "wb");
    if (!f) return 2;
    unsigned ti_log2, eval, tune;
    Step st;
    static_assert(kHksThreads == 1024 && kHksWaves == 16 && kHksFreeGroup == 4 && kHksIdle == 0xffffffffu, "the walk's constants");
    while (std::scanf("%u %u %u %u %u %u %u %u %u", &ti_log2, &eval, &tune, &st.first, &st.count, &st.nonfree, &st.n_and, &st.n_or,
                      &st.n_inv) == 9) {
        std::vector<uint32_t> rec;
        auto put = [&](uint32_t role, uint32_t wave, uint32_t pass, uint32_t lane, uint32_t v) {
            const uint32_t r[6] = {role, wave, pass, lane, v, 0};
            rec.insert(rec.end(), r, r + 6);
        };
        const uint32_t e_hash = hks_hash_lanes(st, ti_log2, eval), n_free = hks_free_lanes(st, ti_log2);
        const bool wide = hks_level_wide(st, ti_log2, eval);
        const uint32_t H = wide ? hks_hash_waves(e_hash, n_free, eval, tune) : 0u;
        const uint32_t nph = wide ? hks_hash_passes(e_hash, H) : 0u, npf = wide ? hks_free_passes(n_free, H) : 0u;
        for (uint32_t wave = 0; wave < kHksWaves; wave++)
            for (uint32_t lane = 0; lane < 64; lane++) {
                if (!wide) {  // the single pass: lane threadIdx.x of the column form
                    put(0, wave, 0, lane, wave * 64 + lane);
                } else if (wave < H) {  // passes 0 and 1 prefetched, then p + 2 under pass p: nph + 2 descriptors, nph + 1 of them loaded from
                    for (uint32_t p = 0; p < nph + 2; p++) put(1, wave, p, lane, hks_hash_lane(e_hash, H, wave, p, lane));
                } else {  // groups of kHksFreeGroup passes
                    for (uint32_t p0 = 0; p0 < npf; p0 += kHksFreeGroup)
                        for (uint32_t p = p0; p < p0 + kHksFreeGroup; p++) put(2, wave, p, lane, hks_free_lane(n_free, H, wave, p, lane));
                }
            }
        const uint32_t head[6] = {wide, H, e_hash, n_free, nph, npf};
        const uint32_t n = (uint32_t)(rec.size() / 6);
        std::fwrite(head, sizeof head, 1, f);
        std::fwrite(&n, 4, 1, f);
        if (n) std::fwrite(rec.data(), 4, rec.size(), f);
    }
    return std::fclose(f) == 0 ? 0 : 2;
}
"""


def lq(ev):
    """log2 of the wide lanes per AND / OR / INV gate-instance (col_classify<2, 1, HAS_OR, 2> / <1, 0, HAS_OR, 0>)"""
    return (1, 0, 0) if ev else (2, 2, 1)


def lanes_of(ev, ti, n_and, n_or, n_inv, n_free):
    a, o, i = lq(ev)
    return 4 * ti * ((n_and << a) + (n_or << o) + (n_inv << i)), n_free * ti


def shapes():
    """[(name, ti_log2, eval, tune, (first, count, nonfree, n_and, n_or, n_inv))]"""
    out = []

    def add(name, t, ev, tune, n_and, n_or, n_inv, n_free, first=7):
        nonfree = n_and + n_or + n_inv
        out.append(("%s-ti%d-%s%s-h%d" % (name, 1 << t, "eval" if ev else "garble", "-or" if n_or else "", tune), t, ev, tune,
                    (first, nonfree + n_free, nonfree, n_and, n_or, n_inv)))

    for t in (0, 1, 2, 6):
        ti = 1 << t
        for ev in (0, 1):
            a, _, _ = lq(ev)
            full = 1024 // (4 * ti << a)  # AND gates that fill 1 024 column lanes
            for n_or in (0, 3):
                # hashed lanes short of 1 024 by 16 free gates' worth where OR gates are in (their rows shift the AND count)
                n_and = full if not n_or else max(full - 3, 0)
                eh, _ = lanes_of(ev, ti, n_and, n_or, 0, 0)
                fill = (1024 - eh) // ti if eh <= 1024 else 0
                if eh <= 1024:
                    add("edge1024", t, ev, 0, n_and, n_or, 0, fill)       # the single pass, full
                    add("edge-above", t, ev, 0, n_and, n_or, 0, fill + 1)  # the narrowest split level: 1 024 + TI lanes
                add("mixed", t, ev, 0, 37 if t < 6 else 3, n_or, 11 if t < 6 else 2, 333 if t < 6 else 41, first=0)
                add("hashonly", t, ev, 0, 3 * full + 1, n_or, 5, 0)
                add("one-and", t, ev, 0, 1, 0, 0, max(400, 1100 // ti + 1))
            add("freeonly", t, ev, 0, 0, 0, 0, 1024 // ti + 3)
            add("narrow-freeonly", t, ev, 0, 0, 0, 0, 5 if t < 6 else 1)
            add("narrow-mixed", t, ev, 0, 1, 1 if t < 6 else 0, 1, 2)
            for tune in range(1, 16):
                add("mixed", t, ev, tune, 37 if t < 6 else 3, 2, 11 if t < 6 else 2, 333 if t < 6 else 41)
            for tune in (1, 8, 15):
                add("one-and", t, ev, tune, 1, 0, 0, max(400, 1100 // ti + 1))
                add("hashonly", t, ev, tune, 3 * full + 1, 0, 5, 0)
                add("freeonly", t, ev, tune, 0, 0, 0, 1024 // ti + 3)
    return out


SHAPES = shapes()


@pytest.fixture(scope="module")
def walks(tmp_path_factory):
    d = tmp_path_factory.mktemp("hbm_keyed_split_index")
    src, exe, out = d / "hks_walk.cpp", d / "hks_walk", d / "walk.bin"
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(out)], input="".join("%d %d %d %d %d %d %d %d %d\n" % ((t, ev, tune) + st)
                                                            for _, t, ev, tune, st in SHAPES),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    raw = np.fromfile(str(out), np.uint32)
    res, k = {}, 0
    for name, *_ in SHAPES:
        head, n = [int(v) for v in raw[k:k + 6]], int(raw[k + 6])
        res[name] = (head, raw[k + 7:k + 7 + 6 * n].reshape(n, 6))
        k += 7 + 6 * n
    assert k == len(raw)
    return res


def classify(ev, st, t, J):
    """col_classify<.., HAS_OR = true, ..> in 32-bit arithmetic -> (kind, g, inst, q, c) per lane; kind 0 none, 1 AND, 2 OR, 3 INV,
    4 free"""
    first, count, nonfree, n_and, n_or, n_inv = st
    a, o, i = lq(ev)
    J = np.asarray(J, np.uint64)
    M = np.uint64(0xFFFFFFFF)
    ti, tim = 1 << t, np.uint64((1 << t) - 1)
    e_and = 4 * ti * (n_and << a)
    e_or = e_and + 4 * ti * (n_or << o)
    ncol = e_or + 4 * ti * (n_inv << i)
    kind = np.zeros(len(J), np.int64)
    g, inst, q = np.zeros(len(J), np.int64), np.zeros(len(J), np.int64), np.zeros(len(J), np.int64)
    c = (J & np.uint64(3)).astype(np.int64)
    for k, lo, hi, l, g0 in ((1, 0, e_and, a, 0), (2, e_and, e_or, o, n_and), (3, e_or, ncol, i, n_and + n_or)):
        m = (J >= lo) & (J < hi)
        w = (J[m] - np.uint64(lo)) >> np.uint64(2)
        kind[m] = k
        q[m] = (w & np.uint64((1 << l) - 1)).astype(np.int64)
        inst[m] = ((w >> np.uint64(l)) & tim).astype(np.int64)
        g[m] = g0 + (w >> np.uint64(t + l)).astype(np.int64)
    u = (J - np.uint64(ncol)) & M  # (unsigned wrap, as in the kernel)
    m = (J >= ncol) & (u < (count - nonfree) * ti)
    kind[m] = 4
    inst[m] = (u[m] & tim).astype(np.int64)
    g[m] = nonfree + (u[m] >> np.uint64(t)).astype(np.int64)
    c[kind == 0] = 0
    c[kind == 4] = 0
    return kind, g, inst, q, c


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s[0])
def test_every_lane_of_a_level_is_visited_once_in_whole_rows(walks, shape):
    name, t, ev, tune, st = shape
    first, count, nonfree, n_and, n_or, n_inv = st
    (wide, H, e_hash, n_free, nph, npf), rec = walks[name]
    ti = 1 << t
    want_h, want_f = lanes_of(ev, ti, n_and, n_or, n_inv, count - nonfree)
    assert (e_hash, n_free) == (want_h, want_f) and wide == (want_h + want_f > THREADS)
    role, wave, pas, lane, val = (rec[:, k].astype(np.int64) for k in range(5))
    if not wide:
        assert H == 0 and (role == SINGLE).all() and len(rec) == THREADS
        assert (val == wave * 64 + lane).all() and sorted(val.tolist()) == list(range(THREADS))
        kind = classify(ev, st, t, val)[0]
        assert (kind[val < e_hash] > 0).all() and (kind[val < e_hash] < 4).all()
        assert (kind[(val >= e_hash) & (val < e_hash + n_free)] == 4).all() and (kind[val >= e_hash + n_free] == 0).all()
        return
    # the caps on H
    need = -(-e_hash // 64)
    if n_free == 0:
        assert H == WAVES
    elif e_hash == 0:
        assert H == 0
    elif tune:
        assert H == min(need, tune)
    else:
        assert 1 <= H <= WAVES - 1 and H <= need and (H >= 8 or H == need)
    assert (wave[role == HASH] < H).all() and (wave[role == FREE] >= H).all() and not (role == SINGLE).any()
    assert sorted(set(wave.tolist())) == [w for w in range(WAVES) if w < H or npf > 0]
    # pass counts
    assert nph == (-(-e_hash // (64 * H)) if H else 0) and npf == (-(-n_free // (64 * (WAVES - H))) if H < WAVES else 0)
    hm, fm = role == HASH, role == FREE
    if H:
        assert pas[hm].max() == nph + 1  # (the descriptor two passes ahead)
    if npf:
        assert pas[fm].max() == -(-npf // 4) * 4 - 1  # whole groups of four passes
    # every column lane and every free lane exactly once
    hv, fv = val[hm & (val != IDLE)], val[fm & (val != IDLE)]
    assert sorted(hv.tolist()) == list(range(e_hash)) and sorted(fv.tolist()) == list(range(n_free))
    assert (val[hm & (pas >= nph)] == IDLE).all() and (val[fm & (pas >= npf)] == IDLE).all()
    # whole rows: all lanes of a gate-instance share wave and pass, and sit in one aligned run of lanes of the wave
    if e_hash:
        sel = hm & (val != IDLE)
        kind, g, inst, q, c = classify(ev, st, t, val[sel])
        assert (kind >= 1).all() and (kind <= 3).all()
        key = g * 64 + inst
        order = np.argsort(key, kind="stable")
        ks, ws, ps, ls, qs, cs = key[order], wave[sel][order], pas[sel][order], lane[sel][order], q[order], c[order]
        starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
        sizes = np.diff(np.r_[starts, len(ks)])
        a, o, i = lq(ev)
        size_of = {1: 4 << a, 2: 4 << o, 3: 4 << i}
        assert (sizes == np.array([size_of[int(k)] for k in kind[order][starts]])).all()
        assert (np.maximum.reduceat(ws, starts) == np.minimum.reduceat(ws, starts)).all(), "a row spans two waves"
        assert (np.maximum.reduceat(ps, starts) == np.minimum.reduceat(ps, starts)).all(), "a row spans two passes"
        lo = np.minimum.reduceat(ls, starts)
        assert (lo % sizes == 0).all() and (np.maximum.reduceat(ls, starts) - lo == sizes - 1).all()
        assert (ls - np.repeat(lo, sizes) == 4 * qs + cs).all()  # lane of the row = 4 q + c: what the DPP controls assume
    # an idle lane of a hash wave classifies as K_NONE of gate 0: it re-reads descs[st.first], whatever the level holds
    kind, g, inst, q, c = classify(ev, st, t, np.array([IDLE], np.uint64))
    assert (kind[0], g[0], inst[0], q[0], c[0]) == (0, 0, 0, 0, 0)


def test_the_shapes_cover_what_they_claim(walks):
    """both sides of the form boundary, H = 0, H = 16, fewer hash lanes than a wave, partial last passes, every fixed H"""
    heads = {n: walks[n][0] for n, *_ in SHAPES}
    assert any(h[0] == 0 and h[2] + h[3] == 1024 for h in heads.values())
    assert any(h[0] == 1 and h[2] + h[3] == 1025 for h in heads.values())
    assert any(h[0] == 1 and h[1] == 0 for h in heads.values()) and any(h[0] == 1 and h[1] == 16 for h in heads.values())
    assert any(h[0] == 1 and 0 < h[2] < 64 and h[1] == 1 for h in heads.values())
    assert any(h[0] == 1 and h[1] and h[2] % (64 * h[1]) for h in heads.values())
    assert any(h[0] == 1 and h[1] < 16 and h[3] % (64 * (16 - h[1])) for h in heads.values())
    for tune in range(1, 16):
        assert any(n.endswith("-h%d" % tune) and h[1] == tune for n, h in heads.items())
