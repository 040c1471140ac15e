"""The compile-time resources of csrc/fld.hip, as the shipped flags build it: both tile kernels (the loglik sweep and the
gradient sweep), each without and with the inner-dimension tail, keep two workgroups of four waves on a CU (at most 256
VGPRs, occupancy >= 2) and no kernel of the file uses scratch memory - the f64 exp chains and the two f64 sums per row of
the gradient epilogue must not cost registers the accumulator tile needs."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-metrics_amd", "csrc")
KERNELS = {"fld_columns_kernel", "fld_lse_columns_kernel", "fld_loglik_kernel", "fld_grad_kernel", "fld_loglik_merge_kernel",
           "fld_stats_kernel", "fld_grad_merge_kernel"}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_tile_kernels_keep_two_workgroups_per_cu_and_use_no_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    spec = importlib.util.spec_from_file_location("am_build", os.path.join(ROOT, "audio-metrics_amd", "_build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)                                         # the flags the shipped library is built with
    r = subprocess.run([hipcc, *build.HIPCC_FLAGS, "--cuda-device-only", "-c", "fld.hip", "-o", os.devnull,
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
    with open(os.path.join(CSRC, "fld.hip")) as f:
        source = f.read()
    declared = set(re.findall(r"\b(fld\w*_kernel)\(", source))
    assert declared == KERNELS, declared
    assert source.count("__launch_bounds__(ENGINE_THREADS, 2)") == 2
    for tile_name in ("fld_loglik_kernel", "fld_grad_kernel"):
        tile = {n: u for n, u in usage.items() if tile_name + "I" in n}
        # the tile kernel without / with the inner-dimension tail
        assert len(tile) == 2 and sum("ILb0E" in n for n in tile) == 1 and sum("ILb1E" in n for n in tile) == 1, sorted(tile)
        for n, u in tile.items():
            assert u["vgprs"] <= 256 and u["occupancy"] >= 2, (n, u)
    assert len(usage) == 9 and all(any(k in n for n in usage) for k in declared), sorted(usage)      # every __global__ kernel of the file
    for n, u in usage.items():
        print(n, u)
        assert u["scratch"] == 0, (n, u)
