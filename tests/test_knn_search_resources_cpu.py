"""The compile-time resources of csrc/knn_search.hip, as the shipped flags build it: the six instantiations of the tile kernel
(list lengths 8, 16 and 32, each without / with the inner-dimension tail) stay inside 256 VGPRs - two workgroups of four
waves per CU for the lists of 8 and 16 keys, one for the 32-key lists, which alone take half of a wave's registers - and no
kernel of the file uses scratch memory.  The 16-key form sits at 256 VGPRs exactly: one more live value costs it its second
workgroup."""
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
def test_search_kernels_keep_their_workgroups_per_cu_and_use_no_scratch():
    usage = resource_usage("knn_search.hip")
    with open(os.path.join(CSRC, "knn_search.hip")) as f:
        source = f.read()
    declared = set(re.findall(r"\b(knn_search\w*_kernel)\(", source))
    assert declared == {"knn_search_kernel", "knn_search_merge_kernel"}, declared
    assert "__launch_bounds__(ENGINE_THREADS, KCAP <= 16 ? 2 : 1)" in source
    tile = {n: u for n, u in usage.items() if re.search(r"knn_search_kernelILi(8|16|32)ELb[01]E", n)}
    merge = {n: u for n, u in usage.items() if re.search(r"knn_search_merge_kernelILi(8|16|32)E", n)}
    # every list length without / with the inner-dimension tail, and one merge kernel per list length
    assert sorted(re.search(r"ILi(\d+)ELb([01])E", n).groups() for n in tile) == \
        sorted((str(k), t) for k in (8, 16, 32) for t in "01"), sorted(tile)
    assert sorted(re.search(r"ILi(\d+)E", n).group(1) for n in merge) == ["16", "32", "8"], sorted(merge)
    assert len(usage) == 6 + 3, sorted(usage)                                  # every __global__ kernel of the file
    for n, u in usage.items():
        print(n, u)
        assert u["scratch"] == 0, (n, u)
    for n, u in tile.items():
        kcap = int(re.search(r"ILi(\d+)E", n).group(1))
        assert u["vgprs"] <= 256 and u["occupancy"] >= (2 if kcap <= 16 else 1), (n, u)
