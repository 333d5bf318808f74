"""CPU check of mpc_amd/csrc/launch_dispatch.h: the one place where a key length (10 / 12 / 14 AES rounds) and a flag become
template arguments of a kernel build ("Shared device code").  The dispatch helpers are plain C++17, so they are compiled into a
stand-alone program (tests/cpp/launch_dispatch_check.cpp) with the host compiler under AddressSanitizer and UBSan, against the
stand-in <hip/hip_runtime.h> of tests/cpp/fake_hip.  And the structure the header exists for: no other file of mpc_amd/csrc
dispatches over the round count or sets a kernel's dynamic LDS size by hand."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("launch_dispatch") / "launch_dispatch_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(CPP, "fake_hip"), "-I", CSRC,
                        os.path.join(CPP, "launch_dispatch_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def test_dispatch_helpers(program):
    """with_rounds hands 10, 12 and 14 to the callback as compile-time constants (a static_assert and a template argument
    inside the callback) and returns its result; 0, 11, 13, 15 and -1 give hipErrorInvalidValue without a call; with_flag
    forwards both values; a nested use returns the innermost result, for the build the run-time values name"""
    r = subprocess.run([program], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "launch_dispatch: ok" in r.stdout


def sources():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h", ".cpp")):
            with open(os.path.join(CSRC, name)) as f:
                yield name, f.read()


def test_the_header_is_the_only_dispatch():
    """no ladder over the round count and no hand-set dynamic LDS size outside launch_dispatch.h"""
    for name, text in sources():
        if name == "launch_dispatch.h":
            assert text.count("hipFuncSetAttribute") == 1
            continue
        for word in ("rounds == 10", "case 10:", "hipFuncSetAttribute"):
            assert word not in text, "%s: %s" % (name, word)


def test_no_launch_macros_behind_the_kernels():
    """the macros of a .hip file are kernel-body macros: none is defined behind its last __global__"""
    for name, text in sources():
        if name.endswith(".hip") and "__global__" in text:
            tail = text[text.rindex("__global__"):]
            assert not re.search(r"#\s*define\s+GC_", tail), name
