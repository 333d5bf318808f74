"""CPU check of mpc_amd/csrc/host_transfer.h, the chunked transfer behind every host-buffer call of the batch engine
(DESIGN.md §17).  The header is compiled into a stand-alone program (tests/cpp/host_transfer_check.cpp) with the host compiler
under AddressSanitizer and UBSan, against the stand-in <hip/hip_runtime.h> of tests/cpp/fake_hip, whose device memory, streams
and events are host allocations, whose calls are logged with their stream and whose k-th call can be told to fail.  The kernel
of a chunk is a host transpose; 3 labels per instance and a budget of 32 * 48 bytes make every chunk 32 instances, and batches
of 1, 31, 32, 33, 64, 65 and 97 give one to four chunks, ragged last chunks and the reuse of both staging buffers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("host_transfer") / "host_transfer_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(CPP, "fake_hip"), "-I", CSRC,
                        os.path.join(CPP, "host_transfer_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def check(program, which):
    r = subprocess.run([program, which], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]


def test_chunk_rule(program):
    """max(32, min(batch, budget / per_inst)) rounded up to 32, and the staging bytes that go with it, at points worked out by
    hand: among them (300, 14887 * 16, 32 MiB) -> 160 and (300, 36663 * 16, 32 MiB) -> 64, which
    test_host_api_pinned_buffers_pipeline relies on for its two to five chunks"""
    check(program, "chunk_rule")


def test_clean_runs_data_and_order(program):
    """device -> host in label and wire mode, host -> device from dense and from strided sources (a column offset), pinned and
    pageable: the host bytes are the direct transpose, no access goes past a staging buffer of min(chunk, batch rounded up to
    32) instances, and the log holds the order — pinned: every copy behind its kernel (read) or every kernel behind its copy
    (upload), the reuse of a buffer from chunk 2 on behind its previous use, by event edges; the upload's guard at the head;
    one wait at the end, of the copy stream (read) or the work stream (upload) — pageable: everything on the work stream and
    one wait per chunk.  A second transfer on the same pipe creates and allocates nothing."""
    check(program, "clean")


def test_ensure_and_release(program):
    """creation at first use; no growth, no runtime call; a growth waits for both streams before it frees; the release frees
    every buffer, event and stream once; a failure at every call of a first ensure and of a growth"""
    check(program, "ensure")


def test_failure_at_every_call(program):
    """every case of the clean runs with each of its fallible calls failing in turn, out of memory and otherwise: GC_E_NOMEM /
    GC_E_HIP, one gc::set_error, on neither stream anything queued behind the stream's last wait, no staging buffer freed, no
    leak, and the pipe serves the next transfer"""
    check(program, "failures")
