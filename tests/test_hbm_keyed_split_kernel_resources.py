"""The split form of the keyed HBM-wire kernels (mpc_amd/csrc/fused_hbm_keyed_split_kernels.hip: hash waves and free waves on
wide levels) compiles for gfx950 without scratch or spills in at most 128 VGPRs, its LDS image at the widest tile fits a CU, and
the figures are the ones recorded in profiles/hbm_keyed_split_kernels_resources.txt.  The plain form and the one-key kernels
keep theirs: tests/test_hbm_keyed_kernel_resources.py.  Cross-compiles here; no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

from tests.test_flat_kernel_resources import resource_blocks
from tests.test_hbm_keyed_kernel_resources import FIELDS, HIPCC, LDS_LIMIT, dynamic_lds, one

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "hbm_keyed_split_kernels_resources.txt")
KERNELS = ["k_%s_hbm_keyed_splitILi%dELb%dE" % (role, nr, has_or) for role in ("garble", "eval") for nr in (10, 12, 14)
           for has_or in (0, 1)]


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.fail("hipcc is missing: the product is built with it")
    tmp = tmp_path_factory.mktemp("hbm_keyed_split")
    src = os.path.join(ROOT, "mpc_amd", "csrc", "fused_hbm_keyed_split_kernels.hip")
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                        "--cuda-device-only", "-S", src, "-o", str(tmp / "split.s"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return resource_blocks(r.stderr)


def recorded():
    out = {}
    for line in open(RECORD):
        m = re.match(r"split\s+(\S+)\s+([\d ]+)$", line)
        if m:
            out[m.group(1)] = [int(x) for x in m.group(2).split()]
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_split_kernels_fit_128_vgprs_and_the_lds_of_a_cu(remarks, kernel):
    name, r = one(remarks, kernel)
    print(name, r)
    assert r["ScratchSize [bytes/lane]"] == 0
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0
    assert r["VGPRs"] <= 128
    nr = int(re.search(r"ILi(\d+)E", kernel).group(1))
    assert r["LDS Size [bytes/block]"] + dynamic_lds(nr, 64) <= LDS_LIMIT
    assert recorded()[name] == [r[f] for f in FIELDS], "profiles/hbm_keyed_split_kernels_resources.txt is stale for %s" % name


def test_the_record_lists_the_twelve_instantiations():
    assert len(recorded()) == len(KERNELS) == 12 and all("hbm_keyed_split" in k for k in recorded())
