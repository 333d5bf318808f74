"""The table-driven Chou-Orlandi receiver kernels (mpc_amd/csrc/co_base_kernels.hip) compile for gfx950 without scratch and
without spills: the accumulator, the entry in use, the entry in flight and the scalar all stay in registers (pt_mul_tab takes
its digit from a scalar shifted as a whole, so nothing is indexed by the loop counter).  The register counts themselves are
recorded in profiles/co_base_kernels_resources.txt, not pinned here.  Cross-compiles; no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("k_co_choices_tab", "k_co_decrypt_tab")


def test_co_base_kernels_use_no_scratch(tmp_path):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.fail("hipcc is missing: the product is built with it")
    src = os.path.join(ROOT, "mpc_amd", "csrc", "co_base_kernels.hip")
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                        "--cuda-device-only", "-c", src, "-o", str(tmp_path / "co_base.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vspill = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    sspill = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", r.stderr)]
    for k in KERNELS:
        assert sum(1 for n in names if k in n) == 1, (k, names)
    assert len(names) == len(KERNELS), names  # everything is inlined: no device function is left to call
    assert len(scratch) == len(names) and all(s == 0 for s in scratch), list(zip(names, scratch))
    assert len(vspill) == len(names) and all(v == 0 for v in vspill), list(zip(names, vspill))
    assert len(sspill) == len(names) and all(v == 0 for v in sspill), list(zip(names, sspill))
