"""The VOLE kernels (mpc_amd/csrc/vole_kernels.hip) compile for gfx950 without scratch and without spills: the sender keeps
its AES state, key schedule and 256-bit operands in registers.  Cross-compiles here; no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_vole_kernels_use_no_scratch(tmp_path):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.fail("hipcc is missing: the product is built with it")
    src = os.path.join(ROOT, "mpc_amd", "csrc", "vole_kernels.hip")
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                        "--cuda-device-only", "-c", src, "-o", str(tmp_path / "vole.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vspill = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    sspill = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", r.stderr)]
    assert any("k_vole_sender" in n for n in names) and any("k_vole_receiver" in n for n in names), names
    assert len(scratch) == len(names) and all(s == 0 for s in scratch), list(zip(names, scratch))
    assert len(vspill) == len(names) and all(v == 0 for v in vspill), list(zip(names, vspill))
    assert all(v == 0 for v in sspill), list(zip(names, sspill))
