"""The compile-time resources of csrc/kmeans.hip, as the shipped flags build it: both instantiations of the assign's tile
kernel (without / with the inner-dimension tail) keep two workgroups of four waves on a CU (at most 256 VGPRs, occupancy >= 2)
and no kernel of the file - the assign, its merge, the inertia sum, the update and its finish - uses scratch memory."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-metrics_amd", "csrc")


def resource_usage(source):
    """{mangled kernel name: {scratch, vgprs, occupancy}} of one file of csrc, compiled with the flags of the shipped library."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    spec = importlib.util.spec_from_file_location("am_build", os.path.join(ROOT, "audio-metrics_amd", "_build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)                                         # the flags the shipped library is built with
    r = subprocess.run([hipcc, *build.HIPCC_FLAGS, "--cuda-device-only", "-c", source, "-o", os.devnull,
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
    return usage


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_assign_kernels_keep_two_workgroups_per_cu_and_use_no_scratch():
    usage = resource_usage("kmeans.hip")
    with open(os.path.join(CSRC, "kmeans.hip")) as f:
        source = f.read()
    declared = set(re.findall(r"\b(kmeans\w*_kernel)\(", source))
    assert declared == {"kmeans_assign_kernel", "kmeans_assign_merge_kernel", "kmeans_inertia_kernel", "kmeans_update_kernel",
                        "kmeans_update_finish_kernel"}, declared
    assert "__launch_bounds__(ENGINE_THREADS, 2)" in source
    tile = {n: u for n, u in usage.items() if re.search(r"kmeans_assign_kernelILb[01]E", n)}
    # the tile kernel without / with the inner-dimension tail
    assert len(tile) == 2 and sum("ILb0E" in n for n in tile) == 1 and sum("ILb1E" in n for n in tile) == 1, sorted(tile)
    assert len(usage) == 2 + 4 and all(any(k in n for n in usage) for k in declared), sorted(usage)  # every __global__ kernel of the file
    for n, u in usage.items():
        print(n, u)
        assert u["scratch"] == 0, (n, u)
    for n, u in tile.items():
        assert u["vgprs"] <= 256 and u["occupancy"] >= 2, (n, u)
