"""The Sinkhorn divergence, the part that needs no GPU: sinkhorn_schedule, the float64 oracle's own invariants (S(x, x) = 0,
the entropic cost against the exact assignment cost), validation before any device call in both layers (hip_ops.softmin,
sinkhorn_divergence), the new names in header / signature table / package and the entry point's error paths and workspace
query."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import sinkhorn_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -4
FAKE = ctypes.c_void_p(0x10000)                       # 16-byte aligned, never dereferenced: the calls stop at validation
NAMES = ("am_softmin_workspace_bytes", "am_softmin_f32")


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


# ---------------------------------------------------------------------------------------------------- schedule
def test_schedule_values(am):
    s = am.sinkhorn_schedule(16.0, 0.5, 0.5)
    assert s == [16.0, 4.0, 1.0, 0.25]                                     # 0.25 itself is not "above blur^2": it comes once, last
    assert am.sinkhorn_schedule(16.0, 0.6, 0.5) == [16.0, 4.0, 1.0, 0.36]
    assert am.sinkhorn_schedule(0.2, 0.5, 0.5) == [0.25] and am.sinkhorn_schedule(0.0, 0.5, 0.9) == [0.25]
    assert am.sinkhorn_schedule(0.25, 0.5, 0.5) == [0.25]
    s = am.sinkhorn_schedule(1234.5, 0.37, 0.8)
    assert s == sr.schedule(1234.5, 0.37, 0.8)                             # the oracle restates it
    assert s[0] == 1234.5 and s[-1] == 0.37 * 0.37 and all(a > b for a, b in zip(s, s[1:]))
    assert all(math.isclose(b / a, 0.64, rel_tol=1e-15) for a, b in zip(s[:-2], s[1:-1])) and s[-2] * 0.64 <= s[-1] < s[-2]
    assert len(s) == 2 + math.floor(math.log(1234.5 / 0.37 ** 2) / math.log(1 / 0.64))
    assert all(isinstance(v, float) for v in s)
    for bad in ((1.0, 0.0, 0.5), (1.0, -1.0, 0.5), (1.0, math.inf, 0.5), (1.0, math.nan, 0.5), (1.0, 0.5, 0.0), (1.0, 0.5, 1.0),
                (1.0, 0.5, -0.5), (1.0, 0.5, math.nan), (math.inf, 0.5, 0.5), (math.nan, 0.5, 0.5), (-1.0, 0.5, 0.5)):
        with pytest.raises(ValueError):
            am.sinkhorn_schedule(*bad)


# ---------------------------------------------------------------------------------------------------- the oracle itself
def test_the_oracle_softmin_is_the_definition():
    rng = np.random.default_rng(3)
    cost, g = rng.gamma(2.0, 1.0, size=(7, 5)), rng.standard_normal(5)
    for eps in (10.0, 0.3):
        want = [-eps * math.log(sum(math.exp((g[j] - cost[i, j]) / eps) for j in range(5)) / 5) for i in range(7)]
        assert np.allclose(sr.softmin(cost, g, eps), want, rtol=1e-13, atol=0)
    # far below the underflow of a plain sum: the hard minimum plus eps log m
    assert np.allclose(sr.softmin(cost, np.zeros(5), 1e-4), cost.min(axis=1) + 1e-4 * math.log(5), rtol=1e-12)


def test_the_oracle_divergence_of_a_set_with_itself_is_zero():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((48, 3)).astype(np.float32)
    o = sr.divergence(x, x, blur=0.5, rtol=1e-15, max_iter=5000)
    print(o["divergence"], o["iterations"], o["converged"])
    assert abs(o["divergence"]) <= 1e-12
    # at the fixed point the alternating solve holds the averaged one's potential up to the constant the pair (f + c, g - c) is free in
    assert np.abs(0.5 * (o["xy"]["f_star"] + o["xy"]["g_star"]) - o["xx"]["star"]).max() <= 1e-12
    assert np.ptp(o["candidate_potential"]) <= 1e-12 and np.abs(o["candidate_potential"] + o["reference_potential"]).max() <= 1e-12


def test_the_oracle_against_the_exact_assignment_cost():
    scipy_optimize = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(1)
    x = rng.standard_normal((64, 4))
    y = rng.standard_normal((64, 4)) + 0.5
    cost = sr.half_sq_dists(x, y)
    rows, cols = scipy_optimize.linear_sum_assignment(cost)
    exact = cost[rows, cols].mean()
    o = sr.divergence(x, y, blur=0.05, rtol=0.0, max_iter=5000)
    print(exact, o["ot_xy"], o["divergence"])
    assert o["iterations"][0] == 5000            # (the self solves stop on a change of exactly 0: at this blur a point's own cost 0 wins)
    assert exact <= o["ot_xy"] <= 1.02 * exact                             # the entropic cost bounds the exact one from above
    assert abs(o["divergence"] - exact) <= 1e-3 * exact                    # the debiasing takes the entropic excess out


# ---------------------------------------------------------------------------------------------------- validation
def test_validation_happens_before_any_device_call(am, monkeypatch):
    from audio_metrics_amd import hip_ops

    def forbidden(*a, **k):
        raise AssertionError("device call before validation")
    for name in ("as_matrix", "_call", "_workspace"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    x, y = torch.zeros((10, 8)), torch.zeros((12, 8))
    g, prev = torch.zeros(12, dtype=torch.float64), torch.zeros(10, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match=r"softmin takes float32 rows \(the float64 matrix-core form is not implemented\)"):
        hip_ops.softmin(x.double(), y, g, eps=1.0)
    with pytest.raises(NotImplementedError, match="float32 rows"):
        hip_ops.softmin(x, y.double(), g, eps=1.0)
    with pytest.raises(ValueError, match="feature widths"):
        hip_ops.softmin(x, torch.zeros((12, 12)), g, eps=1.0)
    with pytest.raises(ValueError, match="2-D"):
        hip_ops.softmin(torch.zeros(8), y, g, eps=1.0)
    with pytest.raises(ValueError, match="rows on both sides"):
        hip_ops.softmin(x, torch.zeros((0, 8)), torch.zeros(0, dtype=torch.float64), eps=1.0)
    for bad in (None, 0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="eps"):
            hip_ops.softmin(x, y, g, eps=bad)
    for bad in (g[:11], g.float(), torch.zeros((12, 1), dtype=torch.float64), [0.0] * 12):
        with pytest.raises(ValueError, match="one potential per row of y"):
            hip_ops.softmin(x, y, bad, eps=1.0)
    for bad in (prev[:9], prev.float()):
        with pytest.raises(ValueError, match="one value per row of x"):
            hip_ops.softmin(x, y, g, eps=1.0, prev=bad)
    for bad in (-0.5, 1.0, math.nan):
        with pytest.raises(ValueError, match="damping"):
            hip_ops.softmin(x, y, g, eps=1.0, prev=prev, damping=bad)
    with pytest.raises(ValueError, match="needs prev"):
        hip_ops.softmin(x, y, g, eps=1.0, damping=0.5)
    # past the checks it reaches the device operations
    with pytest.raises(AssertionError, match="device call before validation"):
        hip_ops.softmin(x, y, g, eps=1.0, prev=prev, damping=0.5)

    # the front end: with the operations it uses forbidden too
    for name in ("softmin", "pairwise_select_sq"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    rows_x, rows_y = torch.randn((10, 8)), torch.randn((12, 8))
    ok, other = host_set(am, rows_x), host_set(am, rows_y)
    for a, b in ((host_set(am, rows_x.double()), other), (ok, host_set(am, rows_y.double()))):
        with pytest.raises(NotImplementedError, match=r"float64 rows; softmin takes float32 rows \(the float64 matrix-core form is not implemented\)"):
            am.sinkhorn_divergence(a, b, blur=1.0)
    with pytest.raises(ValueError, match="feature widths"):
        am.sinkhorn_divergence(ok, host_set(am, torch.zeros((12, 12))), blur=1.0)
    with pytest.raises(ValueError, match="keeps none"):
        am.sinkhorn_divergence(ok, am.AudioMetricsData(False), blur=1.0)
    with pytest.raises(ValueError, match="keeps none"):
        am.sinkhorn_divergence(am.AudioMetricsData(False), other, blur=1.0)
    for bad in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="blur"):
            am.sinkhorn_divergence(ok, other, blur=bad)
        with pytest.raises(ValueError, match="blur_factor"):
            am.sinkhorn_divergence(ok, other, blur_factor=bad)
    for bad in (0.0, 1.0, -0.5, 1.5, math.nan):
        with pytest.raises(ValueError, match="scaling"):
            am.sinkhorn_divergence(ok, other, blur=1.0, scaling=bad)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="max_iter"):
            am.sinkhorn_divergence(ok, other, blur=1.0, max_iter=bad)
    with pytest.raises(ValueError, match="rtol"):
        am.sinkhorn_divergence(ok, other, blur=1.0, rtol=-1e-3)
    for value in (math.nan, math.inf, -math.inf):
        poisoned = rows_x.clone()
        poisoned[3, 5] = value
        with pytest.raises(ValueError, match="non-finite"):
            am.sinkhorn_divergence(host_set(am, poisoned), other, blur=1.0)
        with pytest.raises(ValueError, match="non-finite"):
            am.sinkhorn_divergence(other, host_set(am, poisoned), blur=1.0)
    # past the checks the front end reaches the device operations: the median for the default blur, else the first step
    with pytest.raises(AssertionError, match="device call before validation"):
        am.sinkhorn_divergence(ok, other)
    with pytest.raises(AssertionError, match="device call before validation"):
        am.sinkhorn_divergence(ok, other, blur=1.0)


# ---------------------------------------------------------------------------------------------------- names
def test_header_signature_table_and_package_agree(am, lib):
    with open(os.path.join(ROOT, "include", "audio_metrics_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in am._lib.SIGNATURES and hasattr(lib, name), name
    assert len(am._lib.SIGNATURES["am_softmin_f32"][1]) == 16
    from audio_metrics_amd.metrics import sinkhorn
    assert am.sinkhorn_divergence is sinkhorn.sinkhorn_divergence and am.sinkhorn_schedule is sinkhorn.sinkhorn_schedule
    assert am.metrics.sinkhorn is sinkhorn and callable(am.hip_ops.softmin)
    # a function call, not a metric name of AudioMetrics
    import inspect
    assert "sinkhorn" not in inspect.getsource(am.audio_metrics).lower()


# ---------------------------------------------------------------------------------------------------- entry point
def test_entry_point_error_paths_and_workspace(lib):
    n, m, d, ld = 130, 300, 40, 40
    nb = lib.am_softmin_workspace_bytes(n, m, d)
    assert nb > 0

    def call(x=FAKE, n=n, ldx=ld, y=FAKE, m=m, ldy=ld, d=d, g=FAKE, eps=1.0, prev=FAKE, damping=0.0, out=FAKE, stats=FAKE, ws=FAKE,
             nb=nb):
        return lib.am_softmin_f32(x, n, ldx, y, m, ldy, d, g, eps, prev, damping, out, stats, ws, nb, None)
    for null in ("x", "y", "out"):
        assert call(**{null: None}) == BAD_ARG, null
    assert call(x=ctypes.c_void_p(0x10004)) == BAD_ARG and call(y=ctypes.c_void_p(0x10008)) == BAD_ARG      # alignment
    assert call(ldx=42) == BAD_ARG and call(ldy=36) == BAD_ARG                                              # ld % 4, ld >= D
    assert call(n=0) == BAD_SHAPE and call(m=0) == BAD_SHAPE and call(d=0, ldx=0, ldy=0) == BAD_SHAPE
    for bad in (0.0, -1.0, math.inf, -math.inf, math.nan, 1e-40, 1e40):    # 0.5 / eps has to be a normal float32 number
        assert call(eps=bad) == BAD_ARG, bad
        assert "eps" in lib.am_last_error().decode()
    for bad in (-0.5, 1.0, math.nan):
        assert call(damping=bad) == BAD_ARG, bad
    assert call(damping=0.5, prev=None) == BAD_ARG and "prev" in lib.am_last_error().decode()
    assert call(nb=nb - 1) == WORKSPACE and call(ws=None) == WORKSPACE
    for bad in ((0, 5, 8), (5, 0, 8), (5, 5, 0)):
        assert lib.am_softmin_workspace_bytes(*bad) == 0, bad
    # row norms of both sets, one float per column, (4 + 8) bytes per row and chunk - plus alignment
    for n_, m_ in ((130, 300), (1000, 100_000), (100_000, 1000)):
        need = 4 * n_ + 8 * m_ + 12 * n_ * lib.am_knn_search_chunks(n_, m_, 64, 1)
        got = lib.am_softmin_workspace_bytes(n_, m_, 64)
        assert need <= got <= need + 5 * 256, (n_, m_, need, got)
