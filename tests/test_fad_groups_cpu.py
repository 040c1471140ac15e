"""Per-group Frechet distance, the part that needs no GPU: the host oracle, the error paths of the new entry points
(validated before the first HIP call, so fake pointers do), the workspace query, validation of the front end before any
device call, the export, the untouched AudioMetrics tables and the compile-time resources of csrc/frechet_groups.hip."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import fad_groups_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-metrics_amd", "csrc")
BAD_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -4
FAKE = ctypes.c_void_p(0x10000)                       # 16-byte aligned, never dereferenced: the calls stop at validation
ENTRY_POINTS = ("am_frechet_groups_max_rows", "am_frechet_groups_workspace_bytes", "am_frechet_groups_f32", "am_frechet_groups_f64")


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    return audio_metrics_amd


@pytest.fixture(scope="module")
def lib(am):
    return am._lib.load()


# ---------------------------------------------------------------------------------------------------- oracle
def test_oracle_against_the_textbook_formula_at_full_rank():
    """n > D and a full-rank reference: tr sqrt(cov_x cov_y) = sum sqrt(eig(cov_x cov_y)) is well conditioned, so the
    textbook eigenvalue route and the SVD oracle agree to rounding."""
    rng = np.random.default_rng(3)
    y, x = rng.standard_normal((300, 6)), rng.standard_normal((40, 6)) * 1.2 + 0.3
    mu_y, cov_y = fr.reference_stats(y)
    o = fr.group_oracle(x, mu_y, cov_y)
    cov_x = np.cov(x, rowvar=False)
    tr = np.sqrt(np.clip(np.linalg.eigvals(cov_x @ cov_y).real, 0, None)).sum()
    fd = ((x.mean(0) - mu_y) ** 2).sum() + np.trace(cov_x) + np.trace(cov_y) - 2 * tr
    assert abs(o["tr_sqrt"] - tr) <= 1e-13 * o["scale"] and abs(o["fd"] - fd) <= 1e-13 * o["scale"]
    assert fr.group_oracle(x[:1], mu_y, cov_y)["tr_sqrt"] == 0.0
    two = fr.group_oracle(np.stack([x[0], x[0]]), mu_y, cov_y)
    assert two["tr_sqrt"] == 0.0 and two["fd"] == two["scale"]
    both = fr.groups_oracle(x, [0, 10, 40], mu_y, cov_y)
    assert both["fd"][1] == fr.group_oracle(x[10:], mu_y, cov_y)["fd"]


# ---------------------------------------------------------------------------------------------------- C ABI without a device
def test_header_exports_and_signature_table_agree(am, lib):
    with open(os.path.join(ROOT, "include", "audio_metrics_hip.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in am._lib.SIGNATURES and hasattr(lib, name), name
    assert lib.am_frechet_groups_max_rows() == 128
    assert am.hip_ops.frechet_groups_max_rows() == 128


@pytest.mark.parametrize("entry", ["am_frechet_groups_f32", "am_frechet_groups_f64"])
def test_error_paths(lib, entry):
    n, d, sizes = 1000, 64, [5, 128, 1, 50]
    f64 = entry.endswith("f64")

    def offsets(sizes):
        return (ctypes.c_int64 * (len(sizes) + 1))(*np.concatenate([[0], np.cumsum(sizes)]).tolist())
    nb = lib.am_frechet_groups_workspace_bytes(sum(sizes), len(sizes), d)
    assert nb > 0

    def call(x=FAKE, n=n, ld=d, d=d, idx=FAKE, sizes=sizes, b=None, mu=FAKE, cov=FAKE, out=FAKE, ws=FAKE, nb=nb):
        offs = offsets(sizes)
        return getattr(lib, entry)(x, n, ld, d, idx, ctypes.cast(offs, ctypes.c_void_p), len(sizes) if b is None else b, mu, cov, out,
                                   ws, nb, None)
    for kw in ("x", "out", "mu", "cov"):
        assert call(**{kw: None}) == BAD_ARG, kw
        assert "null" in lib.am_last_error().decode()
    assert call(b=0) == BAD_SHAPE and call(d=0, ld=4) == BAD_SHAPE and call(n=0) == BAD_SHAPE
    assert call(sizes=[5, 7, 0, 3]) == BAD_SHAPE and "group 2 " in lib.am_last_error().decode()
    assert call(sizes=[5, 128, 3, 129]) == BAD_SHAPE
    msg = lib.am_last_error().decode()
    assert "group 3 " in msg and "129" in msg and "128" in msg
    assert call(ld=d - 4) == BAD_ARG
    if f64:
        assert call(d=8196, ld=8196) == BAD_ARG                      # (any ld >= D is legal for float64 rows)
    else:
        assert call(ld=d + 1) == BAD_ARG and call(x=ctypes.c_void_p(0x10004)) == BAD_ARG
        assert call(n=1 << 24) == BAD_SHAPE and "4 GiB" in lib.am_last_error().decode()
    # without an index list the groups are stored rows: they must exist
    assert call(idx=None, n=sum(sizes) - 1) == BAD_SHAPE
    assert call(nb=nb - 1) == WORKSPACE and str(nb) in lib.am_last_error().decode()
    assert call(ws=None) == WORKSPACE and call(nb=0) == WORKSPACE


def test_workspace_query(lib):
    q = lib.am_frechet_groups_workspace_bytes
    for d in (16, 20, 64, 132, 512):
        prev = 0
        for b in (1, 9, 300, 2000):
            for per in (1, 5, 50, 128):
                nt = b * per
                w = q(nt, b, d)
                assert w >= 2 * nt * d * 8                              # the centred rows and Z
                assert w < nt * d * 8 * 2 + b * d * 64, (nt, b, d, w)   # ... and nothing of the order D x D per group
        for nt in (2000, 2001, 50_000, 100_000):
            w = q(nt, 2000, d)
            assert w > prev
            prev = w
        by_b = [q(100_000, b, d) for b in (1, 10, 1000, 2000, 100_000)]
        assert by_b == sorted(by_b) and by_b[0] < by_b[-1]
    by_d = [q(100_000, 2000, d) for d in (1, 20, 64, 132, 512, 513)]
    assert by_d == sorted(set(by_d))
    assert q(0, 1, 64) == 0 and q(10, 0, 64) == 0 and q(10, 1, 0) == 0
    # 100 000 x 512 rows in 2 000 groups: 0.8 GB, against 4 GB of covariances + ~25 GB of solver state on the batched route
    assert q(100_000, 2000, 512) < (1 << 30) < 2000 * 512 * 512 * 8


# ---------------------------------------------------------------------------------------------------- front end
def _sets(am, n=10, d=8, dy=8, dtype=torch.float32):
    x = am.AudioMetricsData(True)
    x._embeddings = torch.zeros((n, d), dtype=dtype)
    y = am.AudioMetricsData(False)
    y.n, y.mean, y.cov = 100, torch.zeros(dy, dtype=torch.float64), torch.eye(dy, dtype=torch.float64)
    return x, y


def test_validation_happens_before_any_device_call(am, monkeypatch):
    from audio_metrics_amd import hip_ops

    def forbidden(*a, **k):
        raise AssertionError("device call before validation")
    for name in ("frechet_groups", "stats_gather", "frechet_batch", "as_rows", "as_matrix", "as_matrix64", "frechet_groups_max_rows"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    x, y = _sets(am)
    with pytest.raises(ValueError, match="store"):
        am.frechet_distance_per_group(am.AudioMetricsData(False), y, [0] * 10)
    with pytest.raises(ValueError, match="store"):
        am.frechet_distance_per_group(_sets(am, n=0)[0], y, [])
    with pytest.raises(ValueError, match="empty"):
        am.frechet_distance_per_group(x, y, [])
    with pytest.raises(ValueError, match="9 labels for 10 stored rows"):
        am.frechet_distance_per_group(x, y, np.arange(9))
    with pytest.raises(ValueError, match="11 labels for 10 stored rows"):
        am.frechet_distance_per_group(x, y, torch.arange(11))
    for bad in (np.zeros(10), torch.zeros(10), np.zeros(10, dtype=bool), torch.zeros(10, dtype=torch.bool), ["a"] * 10):
        with pytest.raises(ValueError, match="integer"):
            am.frechet_distance_per_group(x, y, bad)
    with pytest.raises(ValueError, match="1-D"):
        am.frechet_distance_per_group(x, y, np.zeros((10, 1), dtype=np.int64))
    with pytest.raises(ValueError, match="widths differ.*8 columns.*12"):
        am.frechet_distance_per_group(x, _sets(am, dy=12)[1], np.arange(10))
    with pytest.raises(AssertionError, match="device call"):                 # valid arguments do reach the device layer
        am.frechet_distance_per_group(x, y, np.arange(10) // 3, device="cpu")


def test_export_and_untouched_tables(am):
    from audio_metrics_amd import audio_metrics as front
    from audio_metrics_amd.metrics import fad
    assert am.frechet_distance_per_group is fad.frechet_distance_per_group
    assert [k for k, _ in front.METRIC_TABLE] == ["fad", "fad_inf", "kd", "prdc", "apa"]
    assert [k for k, _ in front.EVALUATION_TABLE] == ["fad", "fad_inf", "kd", "kad", "prdc", "apa"]
    assert front.FUSED_METRICS == ("fad", "kd", "prdc")
    assert not any("group" in k for k in front.ROW_METRICS)


# ---------------------------------------------------------------------------------------------------- compile-time resources
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_kernels_use_no_scratch_memory_and_fit_the_lds():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    import importlib.util
    spec = importlib.util.spec_from_file_location("am_build", os.path.join(ROOT, "audio-metrics_amd", "_build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)                                         # the flags the shipped library is built with
    r = subprocess.run([hipcc, *build.HIPCC_FLAGS, "--cuda-device-only", "-c", "frechet_groups.hip", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        for key, short in (("ScratchSize \\[bytes/lane\\]", "scratch"), ("VGPRs Spill", "spill"), ("LDS Size \\[bytes/block\\]", "lds")):
            m = re.search(r"remark:\s+%s: (\d+)" % key, line)
            if m and name:
                usage[name][short] = int(m.group(1))
    for kernel, count in (("fg_centre_kernel", 2), ("fg_gemm_kernel", 1), ("fg_solve_kernel", 3)):
        hits = {n: u for n, u in usage.items() if kernel in n}
        assert len(hits) == count, (kernel, sorted(usage))
        for n, u in hits.items():
            assert u["scratch"] == 0 and u["spill"] == 0, (n, u)
            assert u["lds"] <= 160 * 1024, (n, u)
    # the LDS is static, so the remark is the whole truth: the 128-row instantiation holds a 128 x 129 f64 matrix, the
    # smaller ones leave room for several workgroups per CU
    solve = sorted(u["lds"] for n, u in usage.items() if "fg_solve_kernel" in n)
    assert solve[2] >= 128 * 128 * 8 and solve[1] <= 40 * 1024 and solve[0] <= 12 * 1024, solve
