"""The kernels of the multi-session Chou-Orlandi receiver handle (mpc_amd/csrc/co_multi_base_kernels.hip: the two that build
the per-session window tables on the device and the decrypt that reads them) compile for gfx950 without scratch, without
spills and without LDS, as the other Chou-Orlandi kernels do (tests/test_co_multi_kernel_resources.py): the base, the current
entry and the running product of a table row stay in registers, the Z and prefix products go through global memory, and
nothing of p256.h, co_sha256.h, co_table.h or co_multi_table.h is left as a call.  Cross-compiles here; no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("k_co_multi_tab_bases", "k_co_multi_tab_rows", "k_co_multi_decrypt_tab")


def test_co_multi_base_kernels_use_no_scratch(tmp_path):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.fail("hipcc is missing: the product is built with it")
    src = os.path.join(ROOT, "mpc_amd", "csrc", "co_multi_base_kernels.hip")
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                        "--cuda-device-only", "-c", src, "-o", str(tmp_path / "co_multi_base.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vspill = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    sspill = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    for k in KERNELS:
        assert sum(1 for n in names if k in n) == 1, (k, names)
    assert len(names) == len(KERNELS), names  # everything is inlined: no device function is left to call
    assert len(scratch) == len(names) and all(s == 0 for s in scratch), list(zip(names, scratch))
    assert len(vspill) == len(names) and all(v == 0 for v in vspill), list(zip(names, vspill))
    assert len(sspill) == len(names) and all(v == 0 for v in sspill), list(zip(names, sspill))
    # an array the compiler could not keep in registers may also be moved to LDS instead of scratch: none is
    assert len(lds) == len(names) and all(v == 0 for v in lds), list(zip(names, lds))
