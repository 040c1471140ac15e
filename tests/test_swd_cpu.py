"""The sliced Wasserstein distance, the part that needs no GPU: the float64 oracle of tests/swd_reference.py against
scipy.stats.wasserstein_distance and against the repeat-to-n-m-atoms form, its closed forms (a pure shift, a set against
itself), the directions, validation before any device call in both layers (hip_ops, sliced_wasserstein_distance), the host
formulas of the result dict, the reference cache with the device functions replaced by host ones, the new names in header /
signature table / package, and the entry points' error paths and workspace queries."""
import ctypes
import inspect
import math
import os
import re
import warnings

import numpy as np
import pytest
import torch

import swd_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -4
FAKE = ctypes.c_void_p(0x10000)                       # 16-byte aligned, never dereferenced: the calls stop at validation
NAMES = ("am_sliced_project_f32", "am_sort_rows_workspace_bytes", "am_sort_rows_f32", "am_sliced_w_workspace_bytes",
         "am_sliced_w_f32")
SHAPES = [(1, 1), (1, 7), (7, 1), (5, 5), (6, 4), (127, 129), (300, 257)]


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


# ---------------------------------------------------------------------------------------------------- the oracle itself
@pytest.mark.parametrize("n,m", SHAPES)
def test_the_oracle_against_scipy_and_the_repeat_form(n, m):
    scipy_stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(1000 * n + m)
    xs, ys = np.sort(rng.standard_normal(n)), np.sort(rng.standard_normal(m) * 1.3 + 0.4)
    w1, w2 = ref.wpp_merged(xs, ys, 1), ref.wpp_merged(xs, ys, 2)
    # at most n + m - 1 non-negative terms on either side, each with a few roundings: (n + m + 8) 2^-53 relative
    rel = (n + m + 8) * 2.0 ** -53
    print(n, m, abs(w1 - scipy_stats.wasserstein_distance(xs, ys)) / w1, abs(w2 - ref.wpp_repeat(xs, ys, 2)) / w2)
    assert abs(w1 - scipy_stats.wasserstein_distance(xs, ys)) <= rel * w1
    assert abs(w1 - ref.wpp_repeat(xs, ys, 1)) <= rel * w1
    assert abs(w2 - ref.wpp_repeat(xs, ys, 2)) <= rel * w2
    assert ref.wpp_merged(ys, xs, 1) == pytest.approx(w1, rel=1e-15) and ref.wpp_merged(xs, xs, 2) == 0.0


def test_the_oracle_closed_forms():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((40, 6)).astype(np.float32)
    c = np.array([0.5, -0.25, 1.0, 0.0, 2.0, -1.5])
    y = x.astype(np.float64) + c                                           # f64 rows: the shift is exact
    theta = ref.directions(6, 9, 3)
    shift = np.abs(theta.astype(np.float64) @ c)
    for p in (1, 2):
        w = ref.per_projection(x, y, theta, p)
        assert np.allclose(w ** (1.0 / p), shift, rtol=1e-13, atol=1e-15), p       # every atom moves by <theta, c>
        assert np.all(ref.per_projection(x, x, theta, p) == 0.0)
    out = ref.distance(x, y, 9, 2, 3)
    assert out["swd_pp"] == pytest.approx(float(np.mean(shift ** 2)), rel=1e-13)
    assert out["swd_max"] == pytest.approx(float(shift.max()), rel=1e-13) and out["swd_max_index"] == int(np.argmax(shift))


# ---------------------------------------------------------------------------------------------------- directions
def test_directions_are_reproducible_and_of_unit_norm(am):
    a, b = am.sliced_directions(33, 17, 7), am.sliced_directions(33, 17, 7)
    assert a.dtype == np.float32 and a.shape == (17, 33) and np.array_equal(a, b)
    assert np.array_equal(a, ref.directions(33, 17, 7)) and not np.array_equal(a, am.sliced_directions(33, 17, 8))
    g = np.random.default_rng(7).standard_normal((17, 33))
    assert np.array_equal(a, (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32))
    for d, count, seed in ((1, 4, 0), (33, 17, 7), (512, 64, 123)):
        t = am.sliced_directions(d, count, seed).astype(np.float64)
        assert np.abs(np.sqrt((t * t).sum(axis=1)) - 1.0).max() <= 2.0 ** -24, (d, count)    # each element is rounded by <= 2^-25 |t_k|
    for bad in ((0, 4), (4, 0)):
        with pytest.raises(ValueError):
            am.sliced_directions(*bad, 0)


# ---------------------------------------------------------------------------------------------------- host formulas
def test_host_formulas_of_the_result(am):
    from audio_metrics_amd.metrics.sliced import sliced_summary
    w = np.array([0.25, 4.0, 1.0, 2.25])
    got = sliced_summary(w, 2)
    assert got["swd_pp"] == 1.875 and got["swd"] == math.sqrt(1.875) and got["swd_p"] == 2 and got["swd_n_projections"] == 4
    assert got["swd_max"] == 2.0 and got["swd_max_index"] == 1
    s = math.sqrt(sum((v - 1.875) ** 2 for v in w) / 3)
    assert got["swd_std_error"] == pytest.approx(s / (2.0 * 2.0 * math.sqrt(1.875)), rel=1e-15)
    got = sliced_summary(w, 1)
    assert got["swd"] == 1.875 and got["swd_max"] == 4.0 and got["swd_std_error"] == pytest.approx(s / 2.0, rel=1e-15)
    for p in (1, 2):
        want, got = ref.summary(w, p), sliced_summary(w, p)
        assert all(got[k] == pytest.approx(want[k], rel=1e-15) for k in want), p
    assert math.isnan(sliced_summary(w[:1], 2)["swd_std_error"]) and sliced_summary(w[:1], 2)["swd"] == 0.5
    zero = sliced_summary(np.zeros(5), 2)
    assert zero["swd"] == 0.0 and zero["swd_max"] == 0.0 and math.isnan(zero["swd_std_error"])
    bad = sliced_summary(np.array([1.0, math.nan]), 2, nonfinite=3)
    assert math.isnan(bad["swd"]) and math.isnan(bad["swd_pp"]) and math.isnan(bad["swd_max"]) and bad["swd_max_index"] == -1


# ---------------------------------------------------------------------------------------------------- validation
def test_validation_happens_before_any_device_call(am, monkeypatch):
    from audio_metrics_amd import hip_ops

    def forbidden(*a, **k):
        raise AssertionError("device call before validation")
    for name in ("as_matrix", "_call", "_workspace", "_unit_columns", "upload_host_array"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    x, t = torch.zeros((10, 8)), torch.zeros((3, 8))
    for name, call in (("sliced_project", lambda: hip_ops.sliced_project(x.double(), t)),
                       ("sliced_project", lambda: hip_ops.sliced_project(x, t.double())),
                       ("sort_rows", lambda: hip_ops.sort_rows(x.double())),
                       ("sliced_w", lambda: hip_ops.sliced_w(x.double(), x, 2)),
                       ("sliced_w", lambda: hip_ops.sliced_w(x, x.double(), 2))):
        with pytest.raises(NotImplementedError, match=r"%s takes float32 rows \(the float64 matrix-core form is not implemented\)" % name):
            call()
    with pytest.raises(ValueError, match="feature widths"):
        hip_ops.sliced_project(x, torch.zeros((3, 12)))
    with pytest.raises(ValueError, match="2-D"):
        hip_ops.sliced_project(torch.zeros(8), t)
    with pytest.raises(ValueError, match="needs rows and directions"):
        hip_ops.sliced_project(x, torch.zeros((0, 8)))
    with pytest.raises(ValueError, match="rows and columns"):
        hip_ops.sort_rows(torch.zeros((3, 0)))
    for bad in (0, 3, 1.5, None):
        with pytest.raises(ValueError, match="p="):
            hip_ops.sliced_w(x, x, bad)
    with pytest.raises(ValueError, match="10 and 3 projections"):
        hip_ops.sliced_w(x, t, 2)
    for call in (lambda: hip_ops.sliced_project(x, t), lambda: hip_ops.sort_rows(x), lambda: hip_ops.sliced_w(x, x, 1)):
        with pytest.raises(AssertionError, match="device call before validation"):       # past the checks: the device operations
            call()

    # the front end: with the operations it uses forbidden too
    for name in ("sliced_project", "sort_rows", "sliced_w"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    rows_x, rows_y = torch.randn((10, 8)), torch.randn((12, 8))
    ok, other = host_set(am, rows_x), host_set(am, rows_y)
    for a, b in ((host_set(am, rows_x.double()), other), (ok, host_set(am, rows_y.double()))):
        with pytest.raises(NotImplementedError, match=r"float64 rows; sliced_project takes float32 rows \(the float64 matrix-core form is not implemented\)"):
            am.sliced_wasserstein_distance(a, b)
    with pytest.raises(ValueError, match="feature widths"):
        am.sliced_wasserstein_distance(ok, host_set(am, torch.zeros((12, 12))))
    for empty in (am.AudioMetricsData(False), host_set(am, torch.zeros((0, 8)))):
        with pytest.raises(ValueError, match="keeps none"):
            am.sliced_wasserstein_distance(ok, empty)
        with pytest.raises(ValueError, match="keeps none"):
            am.sliced_wasserstein_distance(empty, other)
    for bad in (0, 3, 1.5, None):
        with pytest.raises(ValueError, match="p="):
            am.sliced_wasserstein_distance(ok, other, p=bad)
    for bad in (0, -4):
        with pytest.raises(ValueError, match="n_projections"):
            am.sliced_wasserstein_distance(ok, other, n_projections=bad)
        with pytest.raises(ValueError, match="chunk_projections"):
            am.sliced_wasserstein_distance(ok, other, chunk_projections=bad)
    with pytest.raises(AssertionError, match="device call before validation"):
        am.sliced_wasserstein_distance(ok, other)


# ---------------------------------------------------------------------------------------------------- the front end on host stand-ins
class HostOps:
    """Host stand-ins of the device functions of the front end, counting calls."""

    def __init__(self):
        self.projected, self.sorted, self.merged = [], 0, 0

    def install(self, monkeypatch, hip_ops):
        monkeypatch.setattr(hip_ops, "as_matrix", lambda e, name="": e)
        monkeypatch.setattr(hip_ops, "upload_host_array", lambda a, device: torch.as_tensor(np.ascontiguousarray(a)))
        monkeypatch.setattr(hip_ops, "sliced_project", self.project)
        monkeypatch.setattr(hip_ops, "sort_rows", self.sort)
        monkeypatch.setattr(hip_ops, "sliced_w", self.w)

    def project(self, x, theta):
        self.projected.append((int(x.shape[0]), int(theta.shape[0])))
        return (theta.double() @ x.double().T).float()

    def sort(self, z, out=None):
        self.sorted += 1
        return torch.sort(z, dim=1).values

    def w(self, zx, zy, p):
        self.merged += 1
        vals = [ref.wpp_merged(a.numpy(), b.numpy(), p) for a, b in zip(zx, zy)]
        bad = [int((~torch.isfinite(a)).sum() + (~torch.isfinite(b)).sum()) for a, b in zip(zx, zy)]
        return (torch.tensor([math.nan if c else v for v, c in zip(vals, bad)], dtype=torch.float64),
                torch.tensor(bad, dtype=torch.int32))


def test_front_end_values_chunks_and_reference_cache(am, monkeypatch):
    from audio_metrics_amd import hip_ops
    from audio_metrics_amd.metrics.kad import reference_cache
    host = HostOps()
    host.install(monkeypatch, hip_ops)
    rng = np.random.default_rng(2)
    x, y = rng.standard_normal((30, 5)).astype(np.float32), (rng.standard_normal((41, 5)) + 0.5).astype(np.float32)
    sx, sy = host_set(am, torch.as_tensor(x)), host_set(am, torch.as_tensor(y))
    got = am.sliced_wasserstein_distance(sx, sy, n_projections=7, p=2, seed=11, cache_reference=False, return_projections=True)
    want = ref.distance(x, y, 7, 2, 11)
    assert np.array_equal(got["swd_directions"], want["swd_directions"]) and got["swd_seed"] == 11
    assert np.allclose(got["swd_per_projection"], want["swd_per_projection"], rtol=1e-5)     # the stand-in projects to float32
    assert got["swd"] == pytest.approx(want["swd"], rel=1e-5) and got["swd_max_index"] == want["swd_max_index"]
    assert host.projected == [(41, 7), (30, 7)] and reference_cache(sy).sliced == {}
    assert set(got) == {"swd", "swd_pp", "swd_p", "swd_n_projections", "swd_seed", "swd_max", "swd_max_index", "swd_std_error",
                        "swd_per_projection", "swd_directions"}
    # chunks of 3: the same values, three calls per set
    host.projected.clear()
    small = am.sliced_wasserstein_distance(sx, sy, n_projections=7, p=2, seed=11, cache_reference=False, chunk_projections=3,
                                           return_projections=True)
    assert np.array_equal(small["swd_per_projection"], got["swd_per_projection"])
    assert host.projected == [(41, 3), (30, 3), (41, 3), (30, 3), (41, 1), (30, 1)]
    # the cache: filled by the first call under (seed, n_projections), read by the second (any chunking), the same bits
    host.projected.clear()
    first = am.sliced_wasserstein_distance(sx, sy, n_projections=7, seed=11, return_projections=True)
    assert list(reference_cache(sy).sliced) == [(11, 7)] and host.projected == [(41, 7), (30, 7)]
    for chunk in (128, 3):
        host.projected.clear()
        again = am.sliced_wasserstein_distance(sx, sy, n_projections=7, seed=11, chunk_projections=chunk, return_projections=True)
        assert all(rows == 30 for rows, _ in host.projected), (chunk, host.projected)          # the reference is not projected again
        assert np.array_equal(again["swd_per_projection"], first["swd_per_projection"]) and again["swd"] == got["swd"]
    am.sliced_wasserstein_distance(sx, sy, n_projections=7, seed=12)
    am.sliced_wasserstein_distance(sx, sy, n_projections=6, seed=11)
    assert sorted(reference_cache(sy).sliced) == [(11, 6), (11, 7), (12, 7)]
    am.sliced_wasserstein_distance(sy, sx, n_projections=7, seed=11, cache_reference=False)
    assert reference_cache(sx).sliced == {}
    # an append (any assignment of rows) drops the entries by the key rule of the cache
    sy.embeddings = torch.as_tensor(np.concatenate([y, y[:3]]))
    assert reference_cache(sy).sliced == {}
    # a set against itself: projected once, exactly zero
    host.projected.clear()
    zero = am.sliced_wasserstein_distance(sx, sx, n_projections=4, cache_reference=False)
    assert zero["swd"] == 0.0 and zero["swd_max"] == 0.0 and math.isnan(zero["swd_std_error"]) and host.projected == [(30, 4)]


def test_front_end_reports_non_finite_projections(am, monkeypatch):
    from audio_metrics_amd import hip_ops
    HostOps().install(monkeypatch, hip_ops)
    rng = np.random.default_rng(4)
    x, y = rng.standard_normal((20, 4)).astype(np.float32), rng.standard_normal((25, 4)).astype(np.float32)
    x[3, 1] = np.nan
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = am.sliced_wasserstein_distance(host_set(am, torch.as_tensor(x)), host_set(am, torch.as_tensor(y)), n_projections=6,
                                             return_projections=True)
    assert len(caught) == 1 and issubclass(caught[0].category, RuntimeWarning) and "6 non-finite" in str(caught[0].message)
    assert math.isnan(got["swd"]) and got["swd_per_projection"].shape == (6,) and np.isnan(got["swd_per_projection"]).all()


# ---------------------------------------------------------------------------------------------------- names
def test_header_signature_table_and_package_agree(am, lib):
    with open(os.path.join(ROOT, "include", "audio_metrics_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in am._lib.SIGNATURES and hasattr(lib, name), name
    from audio_metrics_amd.metrics import sliced
    assert am.sliced_wasserstein_distance is sliced.sliced_wasserstein_distance and am.sliced_directions is sliced.sliced_directions
    assert am.metrics.sliced is sliced
    assert all(callable(getattr(am.hip_ops, n)) for n in ("sliced_project", "sort_rows", "sliced_w"))
    assert "sliced" not in inspect.getsource(am.audio_metrics).lower()      # a function call, not a metric name of AudioMetrics


# ---------------------------------------------------------------------------------------------------- entry points
def test_entry_point_error_paths_and_workspaces(lib):
    def project(x=FAKE, n=130, ldx=40, t=FAKE, nl=5, ldt=40, d=40, z=FAKE, ldz=130):
        return lib.am_sliced_project_f32(x, n, ldx, t, nl, ldt, d, z, ldz, None)
    for null in ("x", "t", "z"):
        assert project(**{null: None}) == BAD_ARG, null
    assert project(x=ctypes.c_void_p(0x10004)) == BAD_ARG and project(ldx=42) == BAD_ARG and project(ldt=36) == BAD_ARG
    assert project(ldz=129) == BAD_ARG and "ldz" in lib.am_last_error().decode()
    assert project(n=0) == BAD_SHAPE and project(nl=0) == BAD_SHAPE and project(d=0, ldx=0, ldt=0) == BAD_SHAPE

    nb = lib.am_sort_rows_workspace_bytes(3, 1025)
    assert 3 * 1028 * 4 <= nb <= 3 * 1028 * 4 + 256
    assert lib.am_sort_rows_workspace_bytes(128, 100_000) == 128 * 100_000 * 4

    def sort(src=FAKE, nl=3, n=1025, ld_in=1025, out=FAKE, ld_out=1028, ws=FAKE, nb=nb):
        return lib.am_sort_rows_f32(src, nl, n, ld_in, out, ld_out, ws, nb, None)
    assert sort(src=None) == BAD_ARG and sort(out=None) == BAD_ARG and sort(ld_in=1024) == BAD_ARG and sort(ld_out=1000) == BAD_ARG
    assert sort(nl=0) == BAD_SHAPE and sort(n=0) == BAD_SHAPE and sort(n=1 << 31, ld_in=1 << 31, ld_out=1 << 31) == BAD_SHAPE
    assert sort(nb=nb - 1) == WORKSPACE and sort(ws=None) == WORKSPACE
    for bad in ((0, 5), (5, 0), (5, 1 << 31)):
        assert lib.am_sort_rows_workspace_bytes(*bad) == 0, bad
    assert lib.am_sort_rows_workspace_bytes(1, (1 << 31) - 1) == 1 << 33

    nbw = lib.am_sliced_w_workspace_bytes(4, 300, 1000)
    assert nbw > 0 and nbw == lib.am_sliced_w_workspace_bytes(4, 1000, 300)
    assert 4 * 4 * 12 <= nbw <= 4 * 4 * 12 + 2 * 256                         # (double, int) per 256 atoms of the larger side and row

    def w(zx=FAKE, n=300, ldx=300, zy=FAKE, m=1000, ldy=1000, nl=4, p=2, out=FAKE, cnt=FAKE, ws=FAKE, nb=nbw):
        return lib.am_sliced_w_f32(zx, n, ldx, zy, m, ldy, nl, p, out, cnt, ws, nb, None)
    for null in ("zx", "zy", "out", "cnt"):
        assert w(**{null: None}) == BAD_ARG, null
    for bad in (0, 3, -1):
        assert w(p=bad) == BAD_ARG and "p=" in lib.am_last_error().decode()
    assert w(ldx=299) == BAD_ARG and w(ldy=999) == BAD_ARG
    assert w(nl=0) == BAD_SHAPE and w(n=0) == BAD_SHAPE and w(m=0) == BAD_SHAPE
    big = 100_000_000                                                       # 10^16 > 2^53: the weights would not be exact
    assert w(n=big, ldx=big, m=big, ldy=big) == BAD_SHAPE and "2^53" in lib.am_last_error().decode()
    assert lib.am_sliced_w_workspace_bytes(1, big, big) == 0 and lib.am_sliced_w_workspace_bytes(1, big, 90_000_000) > 0
    assert w(nb=nbw - 1) == WORKSPACE and w(ws=None) == WORKSPACE
