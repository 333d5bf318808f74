"""The sha2pc kernels (mpc_amd/csrc/sha2pc_kernels.hip) compile for gfx950 without scratch, without spills and without LDS:
the square root of the Round 2 decode keeps its field elements in registers, and nothing of p256.h or p256_sqrt.h is left as
a call.  Cross-compiles here; no GPU needed.  profiles/sha2pc_kernels_resources.txt holds the figures of this compile."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("k_s2_r1_encode", "k_s2_r2_take", "k_s2_r2_encode", "k_s2_r3_decode", "k_s2_r3_header", "k_s2_r3_assemble",
           "k_s2_zero_bad", "k_s2_r4_take", "k_s2_r4_decode", "k_s2_r4_verdict", "k_s2_repack")


def test_sha2pc_kernels_use_no_scratch(tmp_path):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.fail("hipcc is missing: the product is built with it")
    src = os.path.join(ROOT, "mpc_amd", "csrc", "sha2pc_kernels.hip")
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                        "--cuda-device-only", "-c", src, "-o", str(tmp_path / "sha2pc.o"),
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
    assert len(lds) == len(names) and all(v == 0 for v in lds), list(zip(names, lds))
