"""The keyed HBM-wire kernels (mpc_amd/csrc/fused_hbm_keyed_kernels.hip: one AES key per instance, wires in HBM, round keys in
LDS) compile for gfx950 without scratch or spills in at most 128 VGPRs, their LDS image at the widest tile fits a CU, and the
one-key kernels of fused_kernels.hip, which now share their column lane map with them (col_lanes.h), keep the registers and
LDS they had before: the figures of the parent commit are the `before` lines of profiles/hbm_keyed_kernels_resources.txt.
Cross-compiles here; no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

from tests.test_flat_kernel_resources import resource_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
RECORD = os.path.join(ROOT, "profiles", "hbm_keyed_kernels_resources.txt")
FIELDS = ["VGPRs", "TotalSGPRs", "LDS Size [bytes/block]", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill",
          "Occupancy [waves/SIMD]"]
KEYED_KERNELS = ["k_%s_hbm_keyedILi%dELb%dE" % (role, nr, has_or) for role in ("garble", "eval") for nr in (10, 12, 14)
                 for has_or in (0, 1)]
ONE_KEY_KERNELS = ["k_%s_%sILi%dE" % (role, form, nr) for role in ("garble", "eval") for form in ("col", "fused")
                   for nr in (10, 12, 14)]
LDS_LIMIT = 160 * 1024


def dynamic_lds(nr, ti):
    """the LDS map at the head of the file: 64 KiB AES table | R[64] | keys [TI][NR + 1] uint4"""
    return 65536 + 64 * 16 + ti * (nr + 1) * 16


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    """{file: kernel-resource-usage remarks}, the two translation units compiled side by side"""
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.fail("hipcc is missing: the product is built with it")
    tmp = tmp_path_factory.mktemp("hbm_keyed")
    procs = {}
    for name in ("fused_hbm_keyed_kernels", "fused_kernels"):
        src = os.path.join(ROOT, "mpc_amd", "csrc", name + ".hip")
        procs[name] = subprocess.Popen([HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                                        "--cuda-device-only", "-S", src, "-o", str(tmp / (name + ".s")),
                                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out = {}
    for name, p in procs.items():
        _, err = p.communicate()
        assert p.returncode == 0, err[-4000:]
        out[name] = resource_blocks(err)
    return out


def one(res, kernel):
    names = [n for n in res if kernel in n]
    assert len(names) == 1, (kernel, names)
    return names[0], res[names[0]]


def recorded(tag):
    """{mangled name: [figures]} of the record's lines that start with `tag`"""
    out = {}
    for line in open(RECORD):
        m = re.match(r"%s\s+(\S+)\s+([\d ]+)$" % tag, line)
        if m:
            out[m.group(1)] = [int(x) for x in m.group(2).split()]
    return out


@pytest.mark.parametrize("kernel", KEYED_KERNELS)
def test_keyed_hbm_kernels_fit_128_vgprs_and_the_lds_of_a_cu(remarks, kernel):
    name, r = one(remarks["fused_hbm_keyed_kernels"], kernel)
    print(name, r)
    assert r["ScratchSize [bytes/lane]"] == 0
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0
    assert r["VGPRs"] <= 128
    nr = int(re.search(r"ILi(\d+)E", kernel).group(1))
    assert r["LDS Size [bytes/block]"] + dynamic_lds(nr, 64) <= LDS_LIMIT
    assert recorded("keyed")[name] == [r[f] for f in FIELDS], "profiles/hbm_keyed_kernels_resources.txt is stale for %s" % name


def test_the_record_lists_the_twelve_instantiations():
    assert len(recorded("keyed")) == len(KEYED_KERNELS)


@pytest.mark.parametrize("kernel", ONE_KEY_KERNELS)
def test_one_key_kernels_keep_the_parents_figures(remarks, kernel):
    """k_garble_col / k_eval_col (all builds) and the production builds of k_garble_fused / k_eval_fused"""
    if "fused" in kernel:
        kernel += "Lb0E"
    name, r = one(remarks["fused_kernels"], kernel)
    before, after = recorded("before"), recorded("after")
    now = [r[f] for f in FIELDS]
    print(name, dict(zip(FIELDS, now)), "parent:", before[name])
    assert now == before[name], "registers / LDS of %s moved against the parent commit" % name
    assert after[name] == before[name]
