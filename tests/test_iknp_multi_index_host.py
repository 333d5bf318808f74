"""CPU walk of the work items of the multi-session IKNP kernel (mpc_amd/csrc/iknp_multi.h: iknp_multi_item, the arithmetic
k_iknp_multi addresses its four arrays with).  The header is compiled into a small C++ program with the host compiler and
every item of every (S, per, pos) below is compared with a Python model written from the reference's receive loop
(ot/iknp.go:468-511) run once per session:

  * every byte of choice, u and labels that the loop touches is covered by exactly one item, and no item reaches outside the
    buffers of the call (the 64 choice bytes an item may load as whole quarters included): a wrong offset here is an
    out-of-bounds access on the device;
  * an item's stream position is what the session's PRGs have given out before its chunk, and its block count is
    ceil((pos % 16 + byte_rows) / 16);
  * the advance of a call equals the one-session stream_advance, and the u bytes gc_iknp_u_bytes."""
import os
import subprocess

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpc_amd", "csrc")

SS = [1, 3, 9]
PERS = [1, 7, 8, 37, 40, 127, 128, 129, 511, 512, 513, 549, 1024]
POSS = [0, 5, 16, 69]
CASES = [(S, per, pos) for S in SS for per in PERS for pos in POSS]

PROGRAM = r"""
#include <cstdio>

#include "iknp_multi.h"

using namespace gc;

// "S per pos" on stdin, one case per line -> "# items advance u_bytes choice_bytes steps8 steps4", then one line per item
int main() {
    unsigned long long S, per, pos;
    while (std::scanf("%llu %llu %llu", &S, &per, &pos) == 3) {
        const uint64_t items = iknp_multi_items(S, per);
        std::printf("# %llu %llu %llu %llu %llu %llu\n", (unsigned long long)items, (unsigned long long)iknp_multi_advance(per),
                    (unsigned long long)iknp_multi_u_bytes(per), (unsigned long long)iknp_multi_choice_bytes(per),
                    (unsigned long long)iknp_multi_steps(items, 8), (unsigned long long)iknp_multi_steps(items, 4));
        for (uint64_t it = 0; it < items; it++) {
            const IknpMultiItem m = iknp_multi_item(it, per, pos);
            std::printf("%llu %llu %u %u %u %llu %llu %llu %llu\n", (unsigned long long)m.session, (unsigned long long)m.chunk,
                        m.rows, m.byte_rows, m.blocks, (unsigned long long)m.stream_pos, (unsigned long long)m.choice_off,
                        (unsigned long long)m.u_off, (unsigned long long)m.label_off);
        }
    }
    return 0;
}
"""


def go_receive_loop(per, pos):
    """one session of receive() (iknp.go:479-505): per chunk (ofs, rows, byteRows, bytes of u sent before it, stream position)"""
    out, ofs, sent = [], 0, 0
    while ofs < per:
        rows = min(512, per - ofs)
        byte_rows = (rows + 7) // 8
        out.append((ofs, rows, byte_rows, sent, pos))
        sent += byte_rows * 128  # SendData(out[:byteRows*128])
        pos += byte_rows         # prg() draws byteRows bytes from every column stream
        ofs += rows
    return out, sent, pos


def one_session_u_bytes(n):
    """gc_iknp_u_bytes (ot_engine.cpp)"""
    return (n // 512) * 8192 + ((n % 512 + 7) // 8) * 128


def one_session_stream_advance(n):
    """stream_advance (ot_engine.cpp)"""
    return (n // 512) * 64 + (n % 512 + 7) // 8


@pytest.fixture(scope="module")
def walks(tmp_path_factory):
    d = tmp_path_factory.mktemp("iknp_multi_index")
    src, exe = d / "iknp_multi_walk.cpp", d / "iknp_multi_walk"
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], input="".join("%d %d %d\n" % c for c in CASES), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out, lines, k = {}, r.stdout.splitlines(), 0
    for case in CASES:
        head = lines[k].split()
        assert head[0] == "#"
        items = int(head[1])
        out[case] = ([int(x) for x in head[1:]], [[int(x) for x in l.split()] for l in lines[k + 1:k + 1 + items]])
        k += 1 + items
    assert k == len(lines)
    return out


@pytest.mark.parametrize("S", SS)
@pytest.mark.parametrize("per", PERS)
def test_items_cover_every_byte_once(walks, S, per):
    for pos in POSS:
        (items, advance, u_bytes, choice_bytes, steps8, steps4), rows = walks[(S, per, pos)]
        loop, sent, end = go_receive_loop(per, pos)
        assert u_bytes == sent == one_session_u_bytes(per)
        assert advance == end - pos == one_session_stream_advance(per)
        assert choice_bytes == 64 * -(-per // 512) and items == S * len(loop) == len(rows)
        assert steps8 == -(-items // 8) and steps4 == -(-items // 4)
        choice = np.zeros(S * choice_bytes, np.int32)
        u = np.zeros(S * u_bytes, np.int32)
        labels = np.zeros(S * per, np.int32)
        for it, (session, chunk, nrows, byte_rows, blocks, stream_pos, choice_off, u_off, label_off) in enumerate(rows):
            assert (session, chunk) == divmod(it, len(loop)), "session-major, a session's chunks in order"
            ofs, want_rows, want_br, sent_before, want_pos = loop[chunk]
            assert (nrows, byte_rows, stream_pos) == (want_rows, want_br, want_pos)
            assert blocks == -(-(pos % 16 + byte_rows) // 16) and 1 <= blocks <= 5
            assert blocks * 16 - stream_pos % 16 >= byte_rows and stream_pos % 16 == pos % 16
            assert choice_off == session * choice_bytes + ofs // 8
            assert u_off == session * u_bytes + sent_before
            assert label_off == session * per + ofs
            # what the kernel touches: no index below zero, none past the end (numpy would wrap or clip a slice silently)
            assert choice_off % 16 == 0 and choice_off + 64 <= len(choice), "the item's 64 choice bytes, loaded as quarters"
            assert u_off % 128 == 0 and u_off + 128 * byte_rows <= len(u)
            assert label_off + nrows <= len(labels)
            choice[choice_off:choice_off + byte_rows] += 1
            for col in range(128):
                u[u_off + col * byte_rows:u_off + (col + 1) * byte_rows] += 1
            labels[label_off:label_off + nrows] += 1
        assert (u == 1).all() and (labels == 1).all()
        used = np.zeros(S * choice_bytes, np.int32).reshape(S, choice_bytes)
        used[:, :(per + 7) // 8] = 1  # bbuf of the loop: ceil(per / 8) bytes per session, the rest of the chunk is padding
        assert (choice.reshape(S, choice_bytes) == used).all()


def test_a_session_of_128_ots_costs_one_block_per_column(walks):
    for S in SS:
        _, rows = walks[(S, 128, 0)]
        assert [r[4] for r in rows] == [1] * S
        _, rows = walks[(S, 128, 5)]  # off a block boundary (a call of 40 OTs went before): two
        assert [r[4] for r in rows] == [2] * S
        _, rows = walks[(S, 549, 5)]  # a full chunk five, the 5 bytes of the last chunk one
        assert [r[4] for r in rows] == [5, 1] * S
