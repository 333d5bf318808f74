"""The flat batch kernels (mpc_amd/csrc/fused_flat_kernels.hip) compile for gfx950 without scratch or spills in at most 128
VGPRs, and their AES block — the largest basic block of the kernel: 14 rounds of sixteen look-ups — spends fewer than two
VALU instructions per ds_read_b32 (the fused address form of aes_device.h: 24 VALU per round instead of 32).
Cross-compiles here; no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

BATCH_KERNELS = ["k_%s_flatILi%dELb0ELb0E" % (role, nr) for role in ("garble", "eval") for nr in (10, 12, 14)]


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.fail("hipcc is missing: the product is built with it")
    out = tmp_path_factory.mktemp("flat") / "flat.s"
    src = os.path.join(ROOT, "mpc_amd", "csrc", "fused_flat_kernels.hip")
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                        "--cuda-device-only", "-S", src, "-o", str(out), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return r.stderr, out.read_text()


def resource_blocks(remarks):
    """{mangled name: {field: int}} from the kernel-resource-usage remarks"""
    res = {}
    for blk in re.split(r"(?=remark: Function Name: )", remarks):
        m = re.match(r"remark: Function Name: (\S+)", blk)
        if m:
            res[m.group(1)] = {k.strip(): int(v) for k, v in re.findall(r"remark:\s+([A-Za-z][A-Za-z /\[\]]*?): (\d+) \[-Rpass", blk)}
    return res


def largest_block(asm, kernel):
    """mnemonics of the largest basic block of the kernel whose mangled name contains `kernel`"""
    m = re.search(r"^(\S*%s\S*):\s*; @\S+\n(.*?)^\s*s_endpgm" % re.escape(kernel), asm, re.M | re.S)
    assert m, "kernel %s not found in the assembly" % kernel
    best = []
    for bb in re.split(r"^\.LBB\S+:.*$", m.group(2), flags=re.M):
        ins = [l.split()[0] for l in bb.split("\n") if l.startswith("\t") and l.strip() and l.strip()[0] not in ";."]
        if len(ins) > len(best):
            best = ins
    return best


@pytest.mark.parametrize("kernel", BATCH_KERNELS)
def test_flat_batch_kernels_fit_128_vgprs_without_scratch(compiled, kernel):
    res = resource_blocks(compiled[0])
    names = [n for n in res if kernel in n]
    assert len(names) == 1, names
    r = res[names[0]]
    print(names[0], r)
    assert r["ScratchSize [bytes/lane]"] == 0
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0
    assert r["VGPRs"] <= 128


@pytest.mark.parametrize("kernel", ["k_eval_flatILi14ELb0ELb0E", "k_garble_flatILi14ELb0ELb0E"])
def test_aes_block_has_under_two_valu_per_lookup(compiled, kernel):
    ins = largest_block(compiled[1], kernel)
    valu = sum(1 for i in ins if i.startswith("v_"))
    reads = sum(1 for i in ins if i == "ds_read_b32")
    print(kernel, "largest block: %d instructions, %d VALU, %d ds_read_b32, %.2f VALU per look-up" % (len(ins), valu, reads, valu / max(reads, 1)))
    assert reads == 14 * 16, "the largest block is not the whole AES-256 hash (%d ds_read_b32)" % reads
    assert valu / reads < 2.0
