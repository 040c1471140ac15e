"""The compile-time resources of csrc/sample_scores_groups.hip, as the shipped flags build it: both instantiations of the
tile kernel (without / with the inner-dimension tail) keep two workgroups of four waves on a CU (at most 256 VGPRs,
occupancy >= 2, 2 x 76 KiB of LDS inside the 160 KiB of a CU) and no kernel of the file uses scratch memory - two label
registers and a fourth column array must not cost registers the accumulator tile needs.  The file has ONE __global__
kernel: the column pre-kernel and the merge are those of sample_scores.hip."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-metrics_amd", "csrc")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_grouped_tile_kernels_keep_two_workgroups_per_cu_and_use_no_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    spec = importlib.util.spec_from_file_location("am_build", os.path.join(ROOT, "audio-metrics_amd", "_build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)                                         # the flags the shipped library is built with
    r = subprocess.run([hipcc, *build.HIPCC_FLAGS, "--cuda-device-only", "-c", "sample_scores_groups.hip", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        for key, short in (("ScratchSize \\[bytes/lane\\]", "scratch"), ("VGPRs", "vgprs"), ("Occupancy \\[waves/SIMD\\]", "occupancy")):
            m = re.search(r"remark:\s+%s: (\d+)" % key, line)
            if m and name:
                usage[name][short] = int(m.group(1))
    with open(os.path.join(CSRC, "sample_scores_groups.hip")) as f:
        source = f.read()
    assert re.findall(r"\b(\w+_kernel)\(const", source) == ["sample_scores_groups_kernel"]
    assert source.count("__global__") == 1 and "launch_merge(" in source and "launch_columns(" in source and "asm" not in source
    assert "__launch_bounds__(ENGINE_THREADS, 2)" in source
    assert "(ENGINE_LDS_FLOATS + 2 * 4 * TB) * sizeof(float)" in source      # 72 KiB of staging slabs + 4 KiB: two fit in 160 KiB
    # the tile kernel without / with the inner-dimension tail, and nothing else
    assert len(usage) == 2 and all("sample_scores_groups_kernel" in n for n in usage), sorted(usage)
    assert sum("ILb0E" in n for n in usage) == 1 and sum("ILb1E" in n for n in usage) == 1, sorted(usage)
    for n, u in usage.items():
        print(n, u)
        assert u["scratch"] == 0, (n, u)
        assert u["vgprs"] <= 256 and u["occupancy"] >= 2, (n, u)
