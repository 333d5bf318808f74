"""k_sb_serialise_range (mpc_amd/csrc/stream_batch_kernels.hip), the byte-range form of the stream-batch serialiser, compiles
for gfx950 once, without scratch and without spills, and stages a piece in no more LDS than k_sb_serialise does.  Cross-compiles
here; no GPU needed.  profiles/stream_batch_split_kernels_resources.txt holds the figures of this compile."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_the_range_serialiser_uses_no_scratch_and_no_more_lds(tmp_path):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.fail("hipcc is missing: the product is built with it")
    src = os.path.join(ROOT, "mpc_amd", "csrc", "stream_batch_kernels.hip")
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                        "--cuda-device-only", "-c", src, "-o", str(tmp_path / "stream_batch_kernels.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vspill = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    sspill = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vspill) == len(sspill) == len(lds)
    # (the mangled name of k_sb_serialise is followed by its parameter list, that of the range form by "_range")
    ranged = [i for i, n in enumerate(names) if "k_sb_serialise_range" in n]
    whole = [i for i, n in enumerate(names) if "k_sb_serialise" in n and "k_sb_serialise_range" not in n]
    assert len(ranged) == 1 and len(whole) == 1, names
    for i in ranged + whole:
        assert scratch[i] == 0 and vspill[i] == 0 and sspill[i] == 0, (names[i], scratch[i], vspill[i], sspill[i])
    assert 0 < lds[ranged[0]] <= lds[whole[0]], (lds[ranged[0]], lds[whole[0]])
    # the shared row loop and piece_out are inlined into both: no device function is left to call
    assert not [n for n in names if "piece_rows" in n or "piece_out" in n], names
