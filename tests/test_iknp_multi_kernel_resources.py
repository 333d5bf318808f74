"""The multi-session IKNP and COT kernels (mpc_amd/csrc/iknp_multi_kernels.hip) compile for gfx950 without scratch and without
spills: a 1024-lane workgroup leaves a lane 128 VGPRs, and k_iknp_multi keeps the column key, the finished stream words, one
AES block and the item's offsets in them where k_iknp_fused reads its round keys from LDS.  Every instantiation the launcher
can pick is there (receiver / sender x off a block boundary or on it x the two counter forms) and nothing is left as a call.
The VGPR counts are recorded in profiles/iknp_multi_kernels_resources.txt.  Cross-compiles here; no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = {"k_iknp_multi": 8, "k_cot_multi": 2}  # name -> instantiations


def test_iknp_multi_kernels_use_no_scratch(tmp_path):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.fail("hipcc is missing: the product is built with it")
    src = os.path.join(ROOT, "mpc_amd", "csrc", "iknp_multi_kernels.hip")
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                        "--cuda-device-only", "-c", src, "-o", str(tmp_path / "iknp_multi.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)]
    vspill = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    sspill = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", r.stderr)]
    for k, count in KERNELS.items():
        assert sum(1 for n in names if k in n) == count, (k, names)
    assert len(names) == sum(KERNELS.values()), names  # everything is inlined: no device function is left to call
    assert len(scratch) == len(names) and all(s == 0 for s in scratch), list(zip(names, scratch))
    assert len(vspill) == len(names) and all(v == 0 for v in vspill), list(zip(names, vspill))
    assert len(sspill) == len(names) and all(v == 0 for v in sspill), list(zip(names, sspill))
    # 1024 lanes = 16 waves on 4 SIMDs of 512 registers per lane: 128 each
    assert len(vgprs) == len(names) and all(v <= 128 for v in vgprs), list(zip(names, vgprs))


def test_the_recorded_vgpr_counts_are_the_compiler_s(tmp_path):
    """profiles/iknp_multi_kernels_resources.txt holds the remark lines of this file's kernels as the compiler prints them"""
    src = os.path.join(ROOT, "mpc_amd", "csrc", "iknp_multi_kernels.hip")
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                        "--cuda-device-only", "-c", src, "-o", str(tmp_path / "iknp_multi.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    now = dict(zip(re.findall(r"Function Name: (\S+)", r.stderr), re.findall(r" VGPRs: (\d+)", r.stderr)))
    text = open(os.path.join(ROOT, "profiles", "iknp_multi_kernels_resources.txt")).read()
    new = text[text.index("== iknp_multi_kernels.hip"):]
    new = new[:new.index("\n== ", 4)] if "\n== " in new[4:] else new
    rec = dict(zip(re.findall(r"Function Name: (\S+)", new), re.findall(r" VGPRs: (\d+)", new)))
    assert rec == now and len(rec) == sum(KERNELS.values())
