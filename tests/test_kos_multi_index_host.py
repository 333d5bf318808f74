"""CPU walk of the index arithmetic of the multi-session KOS kernel (mpc_amd/csrc/kos_multi.h: which session a team of lanes
owns, where label i of a session lies, which chi counter it has and where its choice bit is).  The header is compiled into a
stand-alone C++ program with the host compiler under AddressSanitizer and UBSan; the program walks a launch the way
k_kos_multi does (workgroup, team, trip, lane, label) and writes one record per label it visits.  The records are compared
with a model written from the reference's two loops (ot/iknp.go:422-454: chi labels 0 .. n-1 over result and b, then 256
more over the choice vector and bcv), run once per session:

  * every label of every session is visited exactly once, with the chi counter restarting at 0 in every session and going on
    at per behind the result labels;
  * every choice bit is read from the right byte and bit of the packed buffers (64 * ceil(per / 512) bytes per session for b,
    64 for bcv, LSB first);
  * no address lies outside the arrays of the call.

(S, per) covers every per that changes a byte or chunk count, per + 256 at the team threshold and one either side, and S one
below, on and one above a sweep of the capped grid for both team sizes."""
import os
import subprocess

import numpy as np
import pytest

from tests.util import kernel_constants

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpc_amd", "csrc")
THREADS, GRID, WAVE_MAX = kernel_constants("kKosMultiThreads", "kKosMultiGrid", "kKosMultiWaveMax")
T = WAVE_MAX - 256  # the largest per that runs a wave per session

PERS = sorted({0, 1, 7, 8, 9, 127, 128, 129, 511, 512, 513, T - 1, T, T + 1})
CASES = [(S, per) for S in (1, 3, 18) for per in PERS]
WAVE_SWEEP, WG_SWEEP = GRID * (THREADS // 64), GRID
CASES += [(S, 1) for S in (WAVE_SWEEP - 1, WAVE_SWEEP, WAVE_SWEEP + 1)]
CASES += [(S, T + 1) for S in (WG_SWEEP - 1, WG_SWEEP, WG_SWEEP + 1)]
CASES += [(GRID + 1, T)]  # more sessions than workgroups: workgroup 0 holds two wave teams

PROGRAM = r"""
#include <cstdio>
#include <vector>

#include "kos_multi.h"

using namespace gc;

// argv[1]: output file.  "S per grid threads wave_max" on stdin, one launch per line -> a header record
// {S, per, workgroups, team, labels visited, 0} and one record {session, label, in_cv, off, bit_byte, bit} per visit
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "wb");
    if (!f) return 2;
    unsigned long long S, per, cap, threads, wave_max;
    while (std::scanf("%llu %llu %llu %llu %llu", &S, &per, &cap, &threads, &wave_max) == 5) {
        const bool wave = kos_multi_wave_team(per, (uint32_t)wave_max);
        const uint32_t team = wave ? 64u : (uint32_t)threads, tpw = (uint32_t)threads / team;
        const uint32_t grid = kos_multi_grid(S, (uint32_t)cap);
        const uint64_t n = kos_multi_labels(per);
        std::vector<uint64_t> rec;
        for (uint32_t b = 0; b < grid; b++)
            for (uint32_t t = 0; t < tpw; t++)
                for (uint64_t trip = 0;; trip++) {
                    const uint64_t s = kos_multi_session(b, t, trip, grid, tpw);
                    if (s >= S) break;
                    for (uint32_t tl = 0; tl < team; tl++)
                        for (uint64_t i = tl; i < n; i += team) {
                            const KosMultiLabel m = kos_multi_label(s, i, per);
                            if (m.ctr != i) return 3;
                            const uint64_t r[6] = {s, m.ctr, m.in_cv, m.off, m.bit_byte, m.bit};
                            rec.insert(rec.end(), r, r + 6);
                        }
                }
        const uint64_t head[6] = {S, per, grid, team, rec.size() / 6, kos_multi_sweep((uint32_t)cap, tpw)};
        std::fwrite(head, sizeof head, 1, f);
        if (!rec.empty()) std::fwrite(rec.data(), 8, rec.size(), f);
    }
    return std::fclose(f) == 0 ? 0 : 2;
}
"""


@pytest.fixture(scope="module")
def walks(tmp_path_factory):
    d = tmp_path_factory.mktemp("kos_multi_index")
    src, exe, out = d / "kos_multi_walk.cpp", d / "kos_multi_walk", d / "walk.bin"
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(out)], input="".join("%d %d %d %d %d\n" % (S, per, GRID, THREADS, WAVE_MAX)
                                                            for S, per in CASES),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    raw = np.fromfile(str(out), np.uint64).reshape(-1, 6)
    res, k = {}, 0
    for case in CASES:
        head = [int(v) for v in raw[k]]
        assert tuple(head[:2]) == case
        res[case] = (head, raw[k + 1:k + 1 + head[4]])
        k += 1 + head[4]
    assert k == len(raw)
    return res


def go_loops(S, per):
    """both loops of Receive (iknp.go:422-454) for S sessions alone: per label (session, chi index, in the choice vector?,
    element of result / choiceVector [S][..], byte and bit of the packed b / bcv)"""
    n = per + 256
    s = np.repeat(np.arange(S, dtype=np.uint64), n)
    i = np.tile(np.arange(n, dtype=np.uint64), S)  # prgLabels hands out label 0, 1, ... of ONE stream per session
    in_cv = i >= per
    j = np.where(in_cv, i - np.uint64(per), i)  # index into choiceVector / result (and bcv / b)
    off = np.where(in_cv, s * np.uint64(256) + j, s * np.uint64(per) + j)
    row = 64 * -(-per // 512)  # bytes of one session's b as gc_iknp_multi_receive_dev takes them
    byte = np.where(in_cv, s * np.uint64(64), s * np.uint64(row)) + j // np.uint64(8)
    return np.stack([s, i, in_cv.astype(np.uint64), off, byte, j % np.uint64(8)], axis=1), row


@pytest.mark.parametrize("case", CASES, ids=lambda c: "S%d-per%d" % c)
def test_every_label_is_visited_once_at_the_right_place(walks, case):
    S, per = case
    (_, _, grid, team, visits, sweep), rec = walks[case]
    wave = per + 256 <= WAVE_MAX
    assert team == (64 if wave else THREADS) and grid == min(S, GRID)
    assert sweep == (WAVE_SWEEP if wave else WG_SWEEP)
    want, row = go_loops(S, per)
    assert visits == len(want) == S * (per + 256)
    order = np.lexsort((rec[:, 1], rec[:, 0]))  # by session, then by label
    assert (rec[order] == want).all()
    # no address outside the arrays: result [S * per], choice_vec [S * 256], b [S * row] bytes, bcv [S * 64] bytes
    res, cv = rec[rec[:, 2] == 0], rec[rec[:, 2] == 1]
    assert len(res) == S * per and len(cv) == S * 256
    if per:
        assert res[:, 3].max() < S * per and res[:, 4].max() < S * row
        assert (res[:, 4] % row < -(-per // 8)).all(), "a byte of padding was read"
    assert cv[:, 3].max() < S * 256 and cv[:, 4].max() < S * 64 and (cv[:, 4] % 64 < 32).all()
    assert rec[:, 5].max() < 8


def test_sessions_go_round_the_workgroups_first(walks):
    """S sessions short of a sweep run on min(S, grid) workgroups: the visits of a launch come workgroup by workgroup, and with
    S = grid + 1 wave teams workgroup 0 is the only one that holds two sessions (0 and grid)"""
    (_, _, grid, team, _, _), rec = walks[(GRID + 1, T)]
    assert grid == GRID and team == 64
    first = rec[::T + 256, 0].tolist()  # the session of every team's walk, in launch order
    assert first == [0, GRID] + list(range(1, GRID))
