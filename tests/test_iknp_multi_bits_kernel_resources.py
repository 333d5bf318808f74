"""The bit-COT kernels of the multi-session IKNP handle and the triple folds over S peers
(mpc_amd/csrc/iknp_multi_bits_kernels.hip) compile for gfx950 without scratch and without spills, the 1 024-lane receiver
within the 128 VGPRs such a workgroup leaves a lane, and every instantiation the launchers can pick is there with nothing
left as a call.  Moving the lane's keystream helpers into iknp_multi_stream.h has not touched the kernels that were there
before: the resource lines of k_iknp_multi / k_cot_multi are the ones profiles/iknp_multi_kernels_resources.txt has held
since they were written.  The new kernels' lines are recorded in profiles/iknp_multi_bits_kernels_resources.txt.
Cross-compiles here; no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# name -> instantiations: receiver (off a block boundary or on it) x (the two counter forms); sender x the counter forms
KERNELS = {"k_iknp_multi_recv_bits": 4, "k_iknp_multi_send_bits": 2, "k_gmw_multi_sender_u": 1, "k_gmw_multi_fold": 2}
FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]")


def remarks(name, tmp_path):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.fail("hipcc is missing: the product is built with it")
    src = os.path.join(ROOT, "mpc_amd", "csrc", name)
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                        "--cuda-device-only", "-c", src, "-o", str(tmp_path / (name + ".o")),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return r.stderr


def resource_lines(text):
    """function name -> {field: value} from the compiler's remarks, or from a file that holds them"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: (?:\S+: )?\s*Function Name: (\S+)", line) or re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for f in FIELDS:
            m = re.search(r"\s%s: (\d+)" % re.escape(f), line)
            if m and cur is not None:
                cur[f] = int(m.group(1))
    return out


@pytest.fixture(scope="module")
def bits(tmp_path_factory):
    return resource_lines(remarks("iknp_multi_bits_kernels.hip", tmp_path_factory.mktemp("bits_res")))


def test_the_new_kernels_use_no_scratch_and_do_not_spill(bits):
    for k, count in KERNELS.items():
        assert sum(1 for n in bits if k in n) == count, (k, sorted(bits))
    assert len(bits) == sum(KERNELS.values()), sorted(bits)  # everything is inlined: no device function is left to call
    for n, r in bits.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (n, r)


def test_the_1024_lane_receiver_fits_its_registers(bits):
    """1024 lanes = 16 waves on 4 SIMDs of 512 registers per lane: 128 each"""
    recv = {n: r for n, r in bits.items() if "k_iknp_multi_recv_bits" in n}
    assert len(recv) == 4 and all(r["VGPRs"] + r.get("AGPRs", 0) <= 128 for r in recv.values()), recv


def test_the_recorded_lines_of_the_new_kernels_are_the_compiler_s(bits):
    text = open(os.path.join(ROOT, "profiles", "iknp_multi_bits_kernels_resources.txt")).read()
    sec = text[text.index("== iknp_multi_bits_kernels.hip"):]
    rec = resource_lines(sec[:sec.index("\n== ", 4)])
    assert rec == bits


def test_the_kernels_that_were_there_keep_their_resource_lines(tmp_path):
    """every field of every k_iknp_multi / k_cot_multi instantiation, against the section of
    profiles/iknp_multi_kernels_resources.txt written when those kernels were added"""
    now = resource_lines(remarks("iknp_multi_kernels.hip", tmp_path))
    text = open(os.path.join(ROOT, "profiles", "iknp_multi_kernels_resources.txt")).read()
    sec = text[text.index("== iknp_multi_kernels.hip"):]
    sec = sec[:sec.index("\n== ", 4)] if "\n== " in sec[4:] else sec
    rec = resource_lines(sec)
    assert len(rec) == 10 and all("k_iknp_multi" in n or "k_cot_multi" in n for n in rec), sorted(rec)
    assert rec == now
