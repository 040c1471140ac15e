"""The compile-time resources of csrc/vendi.hip, as the shipped flags build it: no kernel touches scratch memory, the per-group
kernel exists in its three sizes (up to 32, 64 and 128 rows) for both row types, and the 128-row one - a 128 x 129 f64 matrix
plus the Jacobi's side arrays - stays within the CU's 160 KiB of LDS."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-metrics_amd", "csrc")
CU_LDS_BYTES = 160 * 1024


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_vendi_kernels_use_no_scratch_and_the_group_kernel_fits_in_lds():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    spec = importlib.util.spec_from_file_location("am_build", os.path.join(ROOT, "audio-metrics_amd", "_build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)                                         # the flags the shipped library is built with
    r = subprocess.run([hipcc, *build.HIPCC_FLAGS, "--cuda-device-only", "-c", "vendi.hip", "-o", os.devnull,
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
    with open(os.path.join(CSRC, "vendi.hip")) as f:
        declared = set(re.findall(r"\b(vg_\w+_kernel)\(", f.read()))
    assert declared == {"vg_group_kernel", "vg_prep_kernel", "vg_gram_kernel", "vg_moment_kernel", "vg_fold_kernel"}, declared
    assert all(any(k in n for n in usage) for k in declared), sorted(usage)
    for n, u in usage.items():
        print(n, u)
        assert u["scratch"] == 0, (n, u)
        assert u["vgprs"] <= 256, (n, u)
    group = {n: u for n, u in usage.items() if "vg_group_kernel" in n}
    assert len(group) == 6, sorted(group)
    lds = {}
    for row_type in ("f", "d"):                                            # vg_group_kernel<float / double, 32 / 64 / 128>
        for cap in (32, 64, 128):
            hits = [u for n, u in group.items() if "vg_group_kernelI%sLi%dEE" % (row_type, cap) in n]
            assert len(hits) == 1, (row_type, cap, sorted(group))
            lds[row_type, cap] = hits[0]["lds"]
    for row_type in ("f", "d"):
        assert lds[row_type, 32] < lds[row_type, 64] < lds[row_type, 128]
        assert 128 * 129 * 8 <= lds[row_type, 128] <= CU_LDS_BYTES, lds
        assert lds[row_type, 32] * 8 <= CU_LDS_BYTES                       # eight small groups share a CU
    assert lds["f", 128] == lds["d", 128]
