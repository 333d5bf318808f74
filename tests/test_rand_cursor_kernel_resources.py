"""The kernels of the per-session cursors of the device random streams (mpc_amd/csrc/rand_cursor_kernels.hip) compile for
gfx950 without scratch and without spills for every key length: the cursor fill as k_rand_fill does, the scalar draw with
its candidate's eight limbs, the modulus and all but five rounds' keys in vector registers.  Cross-compiles here; no GPU
needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_rand_cursor_kernels_use_no_scratch(tmp_path):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.fail("hipcc is missing: the product is built with it")
    src = os.path.join(ROOT, "mpc_amd", "csrc", "rand_cursor_kernels.hip")
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                        "--cuda-device-only", "-c", src, "-o", str(tmp_path / "rand_cursor.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vspill = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    sspill = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)]
    # three key lengths of the fill and of the scalar draw; the advance, the set and the status reset once each
    for kernel, n in (("k_rand_cur_fill", 3), ("k_rand_cur_scalars", 3), ("k_rand_cur_advance", 1), ("k_rand_cur_set", 1),
                      ("k_rand_status_reset", 1)):
        assert sum(kernel in x for x in names) == n, names
    assert len(names) == 9
    assert len(scratch) == len(names) and all(s == 0 for s in scratch), list(zip(names, scratch))
    assert len(vspill) == len(names) and all(v == 0 for v in vspill), list(zip(names, vspill))
    assert len(sspill) == len(names) and all(v == 0 for v in sspill), list(zip(names, sspill))
    # a 1024-lane workgroup needs its 16 waves resident at once: at most 128 VGPRs
    assert len(vgprs) == len(names) and all(v <= 128 for v in vgprs), list(zip(names, vgprs))
