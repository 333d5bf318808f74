"""The multi-session KOS kernel (mpc_amd/csrc/kos_multi_kernels.hip) compiles for gfx950 without scratch and without spills:
a 1024-lane workgroup leaves a lane 128 VGPRs, and k_kos_multi keeps its 256-bit product sum, its x sum, the chi key, one
AES block with its on-the-fly key schedule and the multiply in them.  Every instantiation the launchers can pick is there
(receiver / sender x a wave or a workgroup per session) and nothing is left as a call.  The VGPR counts are recorded in
profiles/kos_multi_kernels_resources.txt.  Cross-compiles here; no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = {"k_kos_multi": 4}  # name -> instantiations


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.fail("hipcc is missing: the product is built with it")
    src = os.path.join(ROOT, "mpc_amd", "csrc", "kos_multi_kernels.hip")
    out = tmp_path_factory.mktemp("kos_multi_resources") / "kos_multi.o"
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                        "--cuda-device-only", "-c", src, "-o", str(out), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return r.stderr


def test_kos_multi_kernels_use_no_scratch(remarks):
    names = re.findall(r"Function Name: (\S+)", remarks)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", remarks)]
    vspill = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", remarks)]
    sspill = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", remarks)]
    for k, count in KERNELS.items():
        assert sum(1 for n in names if k in n) == count, (k, names)
    assert len(names) == sum(KERNELS.values()), names  # everything is inlined: no device function is left to call
    assert len(scratch) == len(names) and all(s == 0 for s in scratch), list(zip(names, scratch))
    assert len(vspill) == len(names) and all(v == 0 for v in vspill), list(zip(names, vspill))
    assert len(sspill) == len(names) and all(v == 0 for v in sspill), list(zip(names, sspill))
    # 1024 lanes = 16 waves on 4 SIMDs of 512 registers per lane: 128 each
    assert len(vgprs) == len(names) and all(v <= 128 for v in vgprs), list(zip(names, vgprs))


def test_the_recorded_vgpr_counts_are_the_compiler_s(remarks):
    """profiles/kos_multi_kernels_resources.txt holds the remark lines of this file's kernels as the compiler prints them"""
    now = dict(zip(re.findall(r"Function Name: (\S+)", remarks), re.findall(r" VGPRs: (\d+)", remarks)))
    text = open(os.path.join(ROOT, "profiles", "kos_multi_kernels_resources.txt")).read()
    new = text[text.index("== kos_multi_kernels.hip"):]
    new = new[:new.index("\n== ", 4)] if "\n== " in new[4:] else new
    rec = dict(zip(re.findall(r"Function Name: (\S+)", new), re.findall(r" VGPRs: (\d+)", new)))
    assert rec == now and len(rec) == sum(KERNELS.values())
