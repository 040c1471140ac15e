"""The compile-time resources of csrc/frechet_influence.hip, as the shipped flags build it: both instantiations of the row
kernel (float32 / float64 rows) keep at least two workgroups of four waves on a CU - at most 256 VGPRs, occupancy >= 2 and a
static LDS footprint of at most half the CU's 160 KiB - and no kernel of the file uses scratch memory: the per-row partial
sums and the operands prefetched for the next slab must not cost registers the accumulator tiles need."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-metrics_amd", "csrc")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_row_kernels_keep_two_workgroups_per_cu_and_use_no_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    spec = importlib.util.spec_from_file_location("am_build", os.path.join(ROOT, "audio-metrics_amd", "_build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)                                         # the flags the shipped library is built with
    r = subprocess.run([hipcc, *build.HIPCC_FLAGS, "--cuda-device-only", "-c", "frechet_influence.hip", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        for key, short in (("ScratchSize \\[bytes/lane\\]", "scratch"), ("VGPRs", "vgprs"), ("Occupancy \\[waves/SIMD\\]", "occupancy"),
                           ("LDS Size \\[bytes/block\\]", "lds")):
            m = re.search(r"remark:\s+%s: (\d+)" % key, line)
            if m and name:
                usage[name][short] = int(m.group(1))
    with open(os.path.join(CSRC, "frechet_influence.hip")) as f:
        source = f.read()
    declared = set(re.findall(r"\b(fi_\w*_kernel)\b", source))
    assert declared == {"fi_rows_kernel", "fi_sums_kernel"}, declared
    assert "__launch_bounds__(256, 2)" in source
    rows = {n: u for n, u in usage.items() if re.search(r"fi_rows_kernelI[fd]E", n)}
    assert len(rows) == 2 and sum("kernelIfE" in n for n in rows) == 1 and sum("kernelIdE" in n for n in rows) == 1, sorted(rows)
    assert len(usage) == 3 and all(any(k in n for n in usage) for k in declared), sorted(usage)      # every __global__ kernel of the file
    for n, u in usage.items():
        print(n, u)
        assert u["scratch"] == 0, (n, u)
    for n, u in rows.items():
        assert u["vgprs"] <= 256 and u["occupancy"] >= 2 and u["lds"] <= 80 * 1024, (n, u)
