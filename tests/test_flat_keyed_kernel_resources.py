"""The keyed flat kernels (mpc_amd/csrc/fused_flat_keyed_kernels.hip: one AES key per instance, round keys in LDS) compile for
gfx950 without scratch or spills in at most 128 VGPRs, and the one-key batch kernels of fused_flat_kernels.hip, which now share
their lane helpers with them (flat_lanes.h), keep the registers and LDS they had before: the figures of the parent commit are
the `before` lines of profiles/flat_keyed_kernels_resources.txt.  Cross-compiles here; no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

from tests.test_flat_kernel_resources import BATCH_KERNELS, resource_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
RECORD = os.path.join(ROOT, "profiles", "flat_keyed_kernels_resources.txt")
FIELDS = ["VGPRs", "TotalSGPRs", "LDS Size [bytes/block]", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill",
          "Occupancy [waves/SIMD]"]
KEYED_KERNELS = ["k_%s_flat_keyedILi%dELb%dE" % (role, nr, has_or) for role in ("garble", "eval") for nr in (10, 12, 14)
                 for has_or in (0, 1)]


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    """{file: kernel-resource-usage remarks}, the two translation units compiled side by side"""
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.fail("hipcc is missing: the product is built with it")
    tmp = tmp_path_factory.mktemp("keyed")
    procs = {}
    for name in ("fused_flat_keyed_kernels", "fused_flat_kernels"):
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


@pytest.mark.parametrize("kernel", KEYED_KERNELS)
def test_keyed_kernels_fit_128_vgprs_without_scratch(remarks, kernel):
    name, r = one(remarks["fused_flat_keyed_kernels"], kernel)
    print(name, r)
    assert r["ScratchSize [bytes/lane]"] == 0
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0
    assert r["VGPRs"] <= 128


@pytest.mark.parametrize("nr", [10, 12, 14])
def test_key_expansion_kernel_has_no_scratch(remarks, nr):
    """its schedule words are indexed by constants only: registers, not a stack array"""
    name, r = one(remarks["fused_flat_keyed_kernels"], "k_expand_keysILi%dE" % nr)
    print(name, r)
    assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0


def recorded(tag):
    """{mangled name: [figures]} of the record's `before` / `after` lines"""
    out = {}
    for line in open(RECORD):
        m = re.match(r"%s\s+(\S+)\s+([\d ]+)$" % tag, line)
        if m:
            out[m.group(1)] = [int(x) for x in m.group(2).split()]
    return out


@pytest.mark.parametrize("kernel", BATCH_KERNELS)
def test_one_key_batch_kernels_keep_the_parents_figures(remarks, kernel):
    name, r = one(remarks["fused_flat_kernels"], kernel)
    before, after = recorded("before"), recorded("after")
    assert len(before) == len(BATCH_KERNELS) == len(after)
    now = [r[f] for f in FIELDS]
    print(name, dict(zip(FIELDS, now)), "parent:", before[name])
    assert now == before[name], "registers / LDS of %s moved against the parent commit" % name
    assert after[name] == before[name]
