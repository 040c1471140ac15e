"""The compile-time resources of csrc/class_scores.hip, as the shipped flags build it: the file declares the five kernels it
says it does, no kernel of it uses scratch memory (the row kernel keeps a row in registers behind a compile-time chunk
count, never a register array under a runtime index), and every instantiation of the class-groups row kernel keeps two
workgroups of four waves on a CU (at most 256 VGPRs, occupancy >= 2; its LDS is dynamic, 64 KiB at the column cap)."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-metrics_amd", "csrc")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_row_kernel_keeps_two_workgroups_per_cu_and_no_kernel_uses_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    spec = importlib.util.spec_from_file_location("am_build", os.path.join(ROOT, "audio-metrics_amd", "_build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)                                         # the flags the shipped library is built with
    r = subprocess.run([hipcc, *build.HIPCC_FLAGS, "--cuda-device-only", "-c", "class_scores.hip", "-o", os.devnull,
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
    with open(os.path.join(CSRC, "class_scores.hip")) as f:
        source = f.read()
    declared = set(re.findall(r"^(cs_\w+_kernel)\(", source, flags=re.M))
    assert declared == {"cs_plan_kernel", "cs_rows_kernel", "cs_groups_kernel", "cs_pairs_kernel", "cs_sums_kernel"}, declared
    assert source.count("__global__") == len(declared)
    assert "__launch_bounds__(256, 2)\ncs_rows_kernel" in source
    rows = {n: u for n, u in usage.items() if "cs_rows_kernel" in n}
    pairs = {n: u for n, u in usage.items() if "cs_pairs_kernel" in n}
    # two row types x six chunk counts (256, 512, 768, 1024, 1536, 2048 columns); two row types x four modes; the other three
    assert len(rows) == 12 and len(pairs) == 8 and len(usage) == 23, sorted(usage)
    assert all(any(k in n for n in usage) for k in declared)
    for n, u in usage.items():
        print(n, u)
        assert u["scratch"] == 0, (n, u)
    for n, u in rows.items():
        assert u["vgprs"] <= 256 and u["occupancy"] >= 2 and u["lds"] == 0, (n, u)          # (static LDS: none; dynamic: (4 C + 8) doubles)
    assert "CS_LDS_MAX = (4 * CS_MAX_C + 8) * 8" in source and "CS_MAX_C = 2048" in source     # 65 600 bytes: two fit the CU's 160 KiB
