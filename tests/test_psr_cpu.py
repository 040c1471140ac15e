"""Probabilistic precision and recall, the part that needs no GPU: the numpy oracle the GPU tests lean on
(tests/psr_reference.py) against direct loops, the host functions of metrics/pprecall.py, validation before any device call,
the non-degeneracy of the test rows at every GPU test shape, and the host side of am_psr_f32 (workspace and chunk queries,
error codes from a fake pointer)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import psr_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -4
FAKE = ctypes.c_void_p(0x10000)                       # 16-byte aligned, never dereferenced: the calls stop at validation
GPU_SHAPES = [(130, 300, 40), (257, 130, 64), (130, 4000, 40), (1000, 130, 64), (300, 257, 40)]


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    return audio_metrics_amd


@pytest.fixture(scope="module")
def lib(am):
    return am._lib.load()


def host_set(am, rows):
    s = am.AudioMetricsData(True)
    s._embeddings = rows
    return s


# ---------------------------------------------------------------------------------------------------- the oracle
def test_oracle_against_a_triple_loop():
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal((7, 3)).astype(np.float32), rng.standard_normal((5, 3)).astype(np.float32)
    y[2] = x[4]                                                           # a point on a row of the set: psr 1
    x[6] += 50.0                                                          # a point far from every row: psr 0
    R = 1.5
    psr, count, d = pr.psr_f64(x, y, R)
    for i in range(7):
        prod, c = 1.0, 0
        for j in range(5):
            d2 = 0.0
            for t in range(3):
                d2 += (float(x[i, t]) - float(y[j, t])) ** 2
            dist = d2 ** 0.5
            assert abs(d[i, j] - dist) < 1e-12
            if dist < R:
                prod *= dist / R
                c += 1
        assert count[i] == c
        assert abs(psr[i] - (1.0 - prod)) < 1e-12, i
    assert psr[4] == pytest.approx(1.0, abs=1e-6) and psr[6] == 0.0 and count[6] == 0
    assert 0 < count.sum() < 35


def test_device_contract_against_the_definition():
    x, y = pr.latent_pair(60, 45, 24)
    R = 1.2 * pr.knn_radii_f64(y, 4).mean()
    psr, count, d = pr.psr_f64(x, y, R)
    got_psr, got_count, got_prod = pr.psr_from_d2((d * d).astype(np.float32), R)
    # the float32 rounding of d2 moves a pair across R only within an ulp of R^2
    r2 = R * R
    lo, hi = ((d * d) < r2 * (1 - 4 * pr.EPS32)).sum(1), ((d * d) <= r2 * (1 + 4 * pr.EPS32)).sum(1)
    assert (lo <= got_count).all() and (got_count <= hi).all() and count.sum() > 0
    # per factor: half an ulp of d2 (a quarter in the root), the root, 1 / R and the multiply
    assert (np.abs(got_psr - psr) <= 3.0 * hi * pr.EPS32 + 1e-15).all(), np.abs(got_psr - psr).max()
    assert np.array_equal(got_psr, 1.0 - got_prod)
    # NaN, +inf and the threshold itself are out of range; 0 gives psr 1
    T = pr.threshold(R)
    assert float(T) >= r2 > float(np.nextafter(T, np.float32(0)))
    edge = np.array([[np.nan, np.inf, T, np.float32(4.0) * T]], dtype=np.float32)
    p, c, _ = pr.psr_from_d2(edge, R)
    assert p.tolist() == [0.0] and c.tolist() == [0]
    below = np.array([[np.nextafter(T, np.float32(0)), np.inf], [0.0, np.nan]], dtype=np.float32)
    p, c, _ = pr.psr_from_d2(below, R)
    assert list(c) == [1, 1] and 0.0 <= p[0] < 1e-6 and p[1] == 1.0


def test_error_bound_is_finite_at_distance_zero():
    x, y = pr.latent_pair(20, 30, 16)
    x[3] = y[7]
    R = 1.2 * pr.knn_radii_f64(y, 4).mean()
    psr, count, d = pr.psr_f64(x, y, R)
    b = pr.error_bound(x, y, d, R)
    assert np.isfinite(b).all() and (b >= 0).all() and b[3] > 0 and (b[count == 0] < 1e-3).all()


# ---------------------------------------------------------------------------------------------------- host functions
def test_psr_radius(am):
    r = np.array([1.0, 2.0, np.inf, 3.0, np.nan], dtype=np.float32)
    assert am.psr_radius(r, 1.2) == (1.2 * 2.0, 2)
    assert am.psr_radius([0.5, 1.5], 2.0) == (2.0, 0)
    v, left = am.psr_radius(torch.tensor([1.0, 4.0]).numpy(), 1.0)
    assert v == 2.5 and left == 0
    with pytest.raises(ValueError, match="no finite"):
        am.psr_radius([np.inf, np.nan], 1.2)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="a="):
            am.psr_radius([1.0], bad)


def test_psr_by_group_against_a_loop(am):
    rng = np.random.default_rng(6)
    labels = np.array([7, 3, 7, -2, 3, 7, 11, 3, 7], dtype=np.int64)      # out of order, a singleton (-2, 11)
    psr = rng.random(9)
    for dtype in (np.int32, np.int64):
        got = am.psr_by_group(labels.astype(dtype), psr)
        want_labels = sorted(set(labels.tolist()))
        assert got["group_labels"].tolist() == want_labels and got["group_labels"].dtype == np.int64
        assert got["group_sizes"].tolist() == [int((labels == g).sum()) for g in want_labels]
        for g, v in zip(want_labels, got["p_precision_per_group"]):
            rows = [psr[i] for i in range(9) if labels[i] == g]
            assert v == pytest.approx(sum(rows) / len(rows), rel=1e-15)
        assert list(got) == ["group_labels", "group_sizes", "p_precision_per_group"]
    with pytest.raises(ValueError, match="1-D"):
        am.psr_by_group(labels.reshape(3, 3), psr)
    with pytest.raises(ValueError, match="1-D and not empty"):
        am.psr_by_group(np.zeros(0, dtype=np.int64), np.zeros(0))
    with pytest.raises(ValueError, match="integers"):
        am.psr_by_group(labels.astype(np.float64), psr)
    with pytest.raises(ValueError, match="one value per row"):
        am.psr_by_group(labels, psr[:8])


# ---------------------------------------------------------------------------------------------------- validation
def test_validation_happens_before_any_device_call(am, monkeypatch):
    from audio_metrics_amd import hip_ops

    def forbidden(*a, **k):
        raise AssertionError("device call before validation")
    for name in ("as_matrix", "_call", "_workspace"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    x, y = torch.zeros((10, 8)), torch.zeros((12, 8))
    for kw in (dict(x=x.double(), y=y), dict(x=x, y=y.double())):
        with pytest.raises(NotImplementedError, match="takes float32 rows"):
            hip_ops.psr_scores(radius=1.0, **kw)
    with pytest.raises(ValueError, match="feature widths"):
        hip_ops.psr_scores(x, torch.zeros((12, 12)), 1.0)
    with pytest.raises(ValueError, match="2-D"):
        hip_ops.psr_scores(torch.zeros(8), y, 1.0)
    with pytest.raises(ValueError, match="rows on both sides"):
        hip_ops.psr_scores(x, torch.zeros((0, 8)), 1.0)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e20):
        with pytest.raises(ValueError, match="radius"):
            hip_ops.psr_scores(x, y, bad)
    # the front ends: with the operations they are built from forbidden too
    for name in ("psr_scores", "knn_radii"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    ok, ref = host_set(am, x), host_set(am, y)
    wide, none = host_set(am, torch.zeros((12, 12))), am.AudioMetricsData(False)
    groups = np.zeros(10, dtype=np.int64)
    calls = [lambda c, r, **kw: am.probabilistic_precision_recall(c, r, **kw),
             lambda c, r, **kw: am.probabilistic_precision_per_group(c, r, groups[:c.embeddings.shape[0]] if c.embeddings is not None
                                                                     else groups, **kw)]
    for call in calls:
        with pytest.raises(NotImplementedError, match="float64"):
            call(host_set(am, x.double()), ref)
        with pytest.raises(NotImplementedError, match="float64"):
            call(ok, host_set(am, y.double()))
        with pytest.raises(ValueError, match="feature widths"):
            call(ok, wide)
        with pytest.raises(ValueError, match="keeps none"):
            call(none, ref)
        with pytest.raises(ValueError, match="keeps none"):
            call(ok, none)
        for bad in (0, -3):
            with pytest.raises(ValueError, match="nearest_k"):
                call(ok, ref, nearest_k=bad)
        for bad in (0.0, -1.2, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="a="):
                call(ok, ref, a=bad)
            with pytest.raises(ValueError, match="radius_reference"):
                call(ok, ref, radius_reference=bad)
        # a reference set of nearest_k rows has no k-th nearest other row
        with pytest.raises(ValueError, match="at least 5"):
            call(ok, host_set(am, torch.zeros((4, 8))))
        with pytest.raises(ValueError, match="at least 13"):
            call(ok, ref, nearest_k=12)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e20):
        with pytest.raises(ValueError, match="radius_candidate"):
            am.probabilistic_precision_recall(ok, ref, radius_candidate=bad)
    with pytest.raises(ValueError, match="candidate set holds 4 rows"):
        am.probabilistic_precision_recall(host_set(am, torch.zeros((4, 8))), ref)
    with pytest.raises(ValueError, match="labels for 10"):
        am.probabilistic_precision_per_group(ok, ref, np.zeros(9, dtype=np.int64))


def test_names(am, lib):
    with open(os.path.join(ROOT, "include", "audio_metrics_hip.h")) as f:
        header = f.read()
    for name in ("am_psr_workspace_bytes", "am_psr_chunks", "am_psr_f32"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in am._lib.SIGNATURES and hasattr(lib, name), name
    assert len(am._lib.SIGNATURES["am_psr_f32"][1]) == 14
    from audio_metrics_amd.metrics import pprecall
    assert am.metrics.pprecall is pprecall
    for name in ("probabilistic_precision_recall", "probabilistic_precision_per_group", "psr_radius", "psr_by_group"):
        assert getattr(am, name) is getattr(pprecall, name), name
    assert pprecall.SATURATION_FRACTION == 0.5
    from audio_metrics_amd import audio_metrics as front                   # not a metric name of AudioMetrics
    assert not any("p_precision" in k or "p_recall" in k for k, _ in front.EVALUATION_TABLE)


# ---------------------------------------------------------------------------------------------------- the test rows
@pytest.mark.parametrize("n,m,d", GPU_SHAPES)
def test_latent_rows_are_not_degenerate(n, m, d):
    """At every shape of tests/test_gpu_psr.py: at least 30 % of the rows have a PSR in (0.01, 0.99), 0 < mean count < 0.2 M."""
    x, y = pr.latent_pair(n, m, d)
    R = 1.2 * pr.knn_radii_f64(y, 4).mean()
    psr, count, _ = pr.psr_f64(x, y, R)
    inner = ((psr > 0.01) & (psr < 0.99)).mean()
    print(f"({n}, {m}, {d}): R {R:.3f} mean psr {psr.mean():.3f} inner {inner:.2f} mean count {count.mean():.1f} max {count.max()}")
    assert inner >= 0.30, inner
    assert 0 < count.mean() < 0.2 * m, count.mean()


def test_prototype_values():
    """300 x 257 x 40, a = 1.2, k = 4, q = 3: the orientation values the feature was specified with."""
    x, y = pr.latent_pair(300, 257, 40)
    r_ref, r_cand = 1.2 * pr.knn_radii_f64(y, 4).mean(), 1.2 * pr.knn_radii_f64(x, 4).mean()
    p, c, _ = pr.psr_f64(x, y, r_ref)
    q, _, _ = pr.psr_f64(y, x, r_cand)
    print(r_ref, r_cand, p.mean(), q.mean(), c.mean(), c.max())
    assert r_ref == pytest.approx(4.42, abs=0.01) and r_cand == pytest.approx(4.11, abs=0.01)
    assert p.mean() == pytest.approx(0.735, abs=0.001) and q.mean() == pytest.approx(0.696, abs=0.001)


# ---------------------------------------------------------------------------------------------------- entry point
def test_workspace_and_chunk_queries_are_host_functions(lib):
    full = lib.am_psr_workspace_bytes(100_000, 100_000, 512)
    assert 0 < full < 256 << 20, full
    assert lib.am_psr_chunks(100_000, 100_000, 512) > 0
    assert lib.am_psr_chunks(130, 4000, 40) == 32
    for bad in ((10, 0, 64), (0, 10, 64), (10, 10, 0)):
        assert lib.am_psr_workspace_bytes(*bad) == 0 and lib.am_psr_chunks(*bad) == 0, bad
    assert lib.am_psr_workspace_bytes(10, 1 << 32, 64) == 0


def test_error_paths(lib):
    n, m, d = 1000, 300, 64
    nb = lib.am_psr_workspace_bytes(n, m, d)
    assert nb > 0

    def call(x=FAKE, n=n, ldx=d, y=FAKE, m=m, ldy=d, d=d, radius=1.5, psr=FAKE, count=FAKE, sums=FAKE, ws=FAKE, nb=nb):
        return lib.am_psr_f32(x, n, ldx, y, m, ldy, d, radius, psr, count, sums, ws, nb, None)
    assert call(x=None) == BAD_ARG and call(y=None) == BAD_ARG and "null" in lib.am_last_error().decode()
    assert call(psr=None) == BAD_ARG and "out_psr" in lib.am_last_error().decode()
    assert call(count=None) == BAD_ARG and "out_count" in lib.am_last_error().decode()
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1.9e19, 1e200):
        assert call(radius=bad) == BAD_ARG and "radius" in lib.am_last_error().decode(), bad
    assert call(n=0) == BAD_SHAPE and call(m=0) == BAD_SHAPE and call(d=0) == BAD_SHAPE
    assert call(ldx=d - 4) == BAD_ARG and call(ldy=d + 2) == BAD_ARG and "ld" in lib.am_last_error().decode()
    assert call(x=ctypes.c_void_p(0x10004)) == BAD_ARG
    assert call(nb=nb - 1) == WORKSPACE and str(nb) in lib.am_last_error().decode() and "am_psr_workspace_bytes" in lib.am_last_error().decode()
    assert call(ws=None) == WORKSPACE and call(nb=0) == WORKSPACE
    assert call(sums=None, nb=0) == WORKSPACE                              # the sums are optional: validation goes on past them
    assert call(radius=1.8e19, nb=0) == WORKSPACE                          # radius^2 just below FLT_MAX is a valid radius
