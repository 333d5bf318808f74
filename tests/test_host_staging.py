"""CPU check of mpc_amd/csrc/host_staging.h, the staging path of every host form of the OT family.  The header
is compiled into a stand-alone program (tests/cpp/host_staging_check.cpp) with the host compiler under AddressSanitizer and
UBSan, against a stand-in <hip/hip_runtime.h> (tests/cpp/fake_hip) whose device memory is host memory, whose calls are logged
and whose k-th call can be told to fail.  The program runs a host form of five arrays: an input, an output, one updated in
place, one of zero bytes and one whose device copy is larger than the copy."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("host_staging") / "host_staging_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(CPP, "fake_hip"), "-I", CSRC,
                        os.path.join(CPP, "host_staging_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def check(program, which):
    r = subprocess.run([program, which], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]


def test_clean_run_order_and_data(program):
    """every allocation, then the inputs in array order, the operation, the outputs in array order, one wait, the frees; the
    data round-trips, the zero-byte entry has a device pointer and no copy, the over-sized one is allocated at its device size"""
    check(program, "clean")


def test_failure_at_every_call(program):
    """GC_E_NOMEM / GC_E_HIP and one gc::set_error; nothing is freed behind a queued copy without a wait in between, every
    allocation is freed once (and ASan sees no leak), and a failed allocation leaves no copy behind"""
    check(program, "failures")


def test_pack_rows(program):
    """per in {0, 1, 7, 8, 9, 511, 512, 513}, S in {1, 3}, rows of ceil(per / 8) bytes and wider"""
    check(program, "pack_rows")
