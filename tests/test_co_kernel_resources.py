"""The Chou-Orlandi kernels (mpc_amd/csrc/co_kernels.hip) compile for gfx950 without scratch and without spills: the point,
the accumulator, the field temporaries and the 18 words of the hash message all stay in registers (nothing in p256.h or
co_sha256.h is indexed by a register).  Cross-compiles here; no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("k_co_encrypt", "k_co_choices", "k_co_decrypt")


def test_co_kernels_use_no_scratch(tmp_path):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.fail("hipcc is missing: the product is built with it")
    src = os.path.join(ROOT, "mpc_amd", "csrc", "co_kernels.hip")
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                        "--cuda-device-only", "-c", src, "-o", str(tmp_path / "co.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vspill = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    sspill = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    for k in KERNELS:
        assert any(k in n for n in names), (k, names)
    assert len(names) == len(KERNELS), names  # everything is inlined: no device function is left to call
    assert len(scratch) == len(names) and all(s == 0 for s in scratch), list(zip(names, scratch))
    assert len(vspill) == len(names) and all(v == 0 for v in vspill), list(zip(names, vspill))
    assert len(sspill) == len(names) and all(v == 0 for v in sspill), list(zip(names, sspill))
    # an array the compiler could not keep in registers may also be moved to LDS instead of scratch: none is
    assert len(lds) == len(names) and all(v == 0 for v in lds), list(zip(names, lds))
