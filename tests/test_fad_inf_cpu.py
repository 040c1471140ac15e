"""FAD-infinity, the part that needs no GPU: the C ABI of the gathered statistics and the batched Frechet solve (header,
exports, signature table, workspace queries), argument validation of frechet_distance_inf before any device call, the
"fad_inf" row of AudioMetrics, and the compile-time resource check of the two new kernel files (no scratch memory)."""
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-metrics_amd", "csrc")
NEW_ENTRY_POINTS = ("am_stats_gather_workspace_bytes", "am_stats_gather_f32", "am_stats_gather_f64",
                    "am_frechet_batch_workspace_bytes", "am_frechet_batch_f64")


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    return audio_metrics_amd


def test_header_exports_and_signature_table_agree(am):
    with open(os.path.join(ROOT, "include", "audio_metrics_hip.h")) as f:
        header = f.read()
    lib = am._lib.load()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in am._lib.SIGNATURES, name
        assert hasattr(lib, name), name


def test_workspace_queries(am):
    lib = am._lib.load()
    for d in (64, 100, 512):
        prev_g = prev_f = 0
        for b in (1, 2, 7, 15, 25):
            g = lib.am_stats_gather_workspace_bytes(b * 10_000, b, d)
            f = lib.am_frechet_batch_workspace_bytes(b, d)
            assert g > 0 and f > 0
            assert g >= prev_g and f > prev_f, (d, b)
            assert f >= 6 * b * d * d * 8
            prev_g, prev_f = g, f
        fixed = [lib.am_stats_gather_workspace_bytes(100_000, b, d) for b in (1, 5, 25)]      # same rows, more subsets
        assert fixed == sorted(fixed) and fixed[0] > 0
    for b, d in ((0, 64), (-1, 64), (3, 0), (3, -2)):
        assert lib.am_frechet_batch_workspace_bytes(b, d) == 0
        assert lib.am_stats_gather_workspace_bytes(1000, b, d) == 0
    assert lib.am_stats_gather_workspace_bytes(0, 3, 64) == 0
    # B = 1 needs what one solve needs, give or take the record the single entry point keeps in its workspace
    assert abs(lib.am_frechet_batch_workspace_bytes(1, 512) - lib.am_frechet_workspace_bytes(512)) <= 4096


def _host_set(am, n, d, rows=None):
    s = am.AudioMetricsData(store_embeddings=rows is not None)
    s.n = n
    s.mean = torch.zeros(d, dtype=torch.float64)
    s.cov = torch.eye(d, dtype=torch.float64)
    return s


def test_argument_validation_happens_before_any_device_call(am, monkeypatch):
    from audio_metrics_amd import hip_ops
    from audio_metrics_amd.metrics import fad

    def forbidden(*a, **k):
        raise AssertionError("device call before validation")
    for name in ("stats_gather", "frechet_batch", "as_rows"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    monkeypatch.setattr(fad, "fad_inf_subset_indices", forbidden)
    x, y = _host_set(am, 10_000, 16), _host_set(am, 10_000, 16)
    with pytest.raises(ValueError, match="store"):
        am.frechet_distance_inf(x, y)                                   # no stored rows
    x._embeddings = torch.zeros((10_000, 16))                           # host rows: enough to get past that check
    with pytest.raises(ValueError, match="steps=1"):
        am.frechet_distance_inf(x, y, steps=1)
    with pytest.raises(ValueError, match="min_n=1 "):
        am.frechet_distance_inf(x, y, min_n=1)
    with pytest.raises(ValueError, match="min_n=10001 .*10000"):
        am.frechet_distance_inf(x, y, min_n=10_001)
    with pytest.raises(ValueError, match="min_n=5000 .*4000"):
        x._embeddings = torch.zeros((4000, 16))
        am.frechet_distance_inf(x, y)                                   # the default min_n on a set of 4000 rows


def test_fit_is_ordinary_least_squares_in_one_over_n(am):
    import numpy as np
    from audio_metrics_amd.metrics.fad import fit_inverse_n
    sizes = np.linspace(5000, 100_000, 15).round()
    exact = 0.25 + 37.0 / sizes
    icpt, slope, r2 = fit_inverse_n(sizes, exact)
    assert icpt == pytest.approx(0.25, abs=1e-12) and slope == pytest.approx(37.0, rel=1e-10) and r2 == pytest.approx(1.0, abs=1e-12)
    noisy = exact + 1e-3 * np.cos(np.arange(15))
    icpt, slope, r2 = fit_inverse_n(sizes, noisy)
    design = np.stack([1.0 / sizes, np.ones(15)], axis=1)
    (s_ref, i_ref), *_ = np.linalg.lstsq(design, noisy, rcond=None)
    assert icpt == pytest.approx(i_ref, rel=1e-12) and slope == pytest.approx(s_ref, rel=1e-12) and 0.0 < r2 < 1.0


class _Embedder:
    sr = 16000

    def get_device(self):
        return torch.device("cpu")                 # a host-side embedder: no replica is moved anywhere


def _fake_one_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)


def test_audio_metrics_row(am, monkeypatch):
    from audio_metrics_amd import audio_metrics as front
    _fake_one_gpu(monkeypatch)
    keys = [k for k, _ in front.METRIC_TABLE]
    assert keys.index("fad_inf") == keys.index("fad") + 1
    m = am.AudioMetrics(metrics=["fad_inf"], embedder=_Embedder(), mix_function=lambda *a: None, device_indices=[0])
    assert m.store_stem_embeddings and m.stems_mode and not m.need_apa
    assert m.stem_reference.store_embeddings
    assert (m.fad_inf_steps, m.fad_inf_min_n, m.fad_inf_seed) == (15, 5000, 0)
    m = am.AudioMetrics(metrics=["fad", "fad_inf"], embedder=_Embedder(), mix_function=lambda *a: None, device_indices=[0],
                        fad_inf_steps=8, fad_inf_min_n=100, fad_inf_seed=3)
    assert (m.fad_inf_steps, m.fad_inf_min_n, m.fad_inf_seed) == (8, 100, 3)
    with pytest.raises(NotImplementedError, match="fad_inf"):
        am.AudioMetrics(metrics=["fad", "fad_inf"], embedder=_Embedder(), mix_function=lambda *a: None, device_indices=[0],
                        process_group=object())


def test_existing_metric_names_resolve_as_before(am, monkeypatch):
    from audio_metrics_amd import audio_metrics as front
    _fake_one_gpu(monkeypatch)
    table = dict(front.METRIC_TABLE)
    assert [k for k, _ in front.METRIC_TABLE if k != "fad_inf"] == ["fad", "kd", "prdc", "apa"]
    assert table["fad"] is front.AudioMetrics._run_fad and table["kd"] is front.AudioMetrics._run_kd
    assert table["prdc"] is front.AudioMetrics._run_prdc and table["apa"] is front.AudioMetrics._run_apa
    assert front.FUSED_METRICS == ("fad", "kd", "prdc")
    m = am.AudioMetrics(embedder=_Embedder(), mix_function=lambda *a: None, device_indices=[0])       # default metrics
    assert m.metrics == ["apa", "fad"]
    assert [k for k, _ in front.METRIC_TABLE if k in m.metrics] == ["fad", "apa"]
    assert not m.store_stem_embeddings and not m.store_mix_embeddings      # statistics only, as before
    for metrics, stored in ((["fad"], False), (["kd"], True), (["prdc"], True), (["precision"], True), (["apa"], False)):
        m = am.AudioMetrics(metrics=metrics, embedder=_Embedder(), mix_function=lambda *a: None, device_indices=[0])
        assert m.store_stem_embeddings is stored, metrics


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
@pytest.mark.parametrize("source, expected", [
    ("stats_gather.hip", ("sg_colsum_kernel", "sg_mean_kernel", "sg_scatter_kernel", "sg_scatter64_kernel", "sg_reduce_kernel")),
    ("frechet_batch.hip", ("nsb_product_kernel", "nsb_init_kernel", "nsb_t_kernel", "nsb_update_kernel", "nsb_finish_kernel")),
])
def test_new_kernels_use_no_scratch_memory(source, expected):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    import importlib.util
    spec = importlib.util.spec_from_file_location("am_build", os.path.join(ROOT, "audio-metrics_amd", "_build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)                                         # the flags the shipped library is built with
    r = subprocess.run([hipcc, *build.HIPCC_FLAGS, "--cuda-device-only", "-c", source, "-o", os.devnull,
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
    for kernel in expected:
        hits = {n: u for n, u in usage.items() if kernel in n}
        assert hits, (kernel, list(usage))
        for n, u in hits.items():
            assert u["scratch"] == 0 and u["spill"] == 0, (n, u)
            assert u["lds"] <= 65536, (n, u)
