"""The compile-time resources of csrc/logit.hip, as the shipped flags build it: the file holds exactly the row kernel (for
float32 and for float64 rows) and the kernel that adds the workgroups' partials, none of them uses scratch memory - the f64
exp / log1p chains of the residual must not spill beside the staged slab - and the row kernel's LDS stays within the 64 KiB a
workgroup may declare statically."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-metrics_amd", "csrc")
KERNELS = {"logit_rows_kernel", "logit_sums_kernel"}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_logit_kernels_use_no_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    spec = importlib.util.spec_from_file_location("am_build", os.path.join(ROOT, "audio-metrics_amd", "_build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)                                         # the flags the shipped library is built with
    r = subprocess.run([hipcc, *build.HIPCC_FLAGS, "--cuda-device-only", "-c", "logit.hip", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        for key, short in (("ScratchSize \\[bytes/lane\\]", "scratch"), ("VGPRs", "vgprs"), ("LDS Size \\[bytes/block\\]", "lds")):
            m = re.search(r"remark:\s+%s: (\d+)" % key, line)
            if m and name:
                usage[name][short] = int(m.group(1))
    with open(os.path.join(CSRC, "logit.hip")) as f:
        source = f.read()
    declared = set(re.findall(r"\b(logit\w*_kernel)\(", source))
    assert declared == KERNELS, declared
    assert source.count("__global__") == 2
    rows = {n: u for n, u in usage.items() if "logit_rows_kernelI" in n}
    assert len(rows) == 2 and sum("IfE" in n for n in rows) == 1 and sum("IdE" in n for n in rows) == 1, sorted(rows)
    assert len(usage) == 3 and any("logit_sums_kernel" in n for n in usage), sorted(usage)      # every __global__ kernel of the file
    for n, u in usage.items():
        print(n, u)
        assert u["scratch"] == 0, (n, u)
        assert u["vgprs"] <= 256 and u["lds"] <= 65536, (n, u)
