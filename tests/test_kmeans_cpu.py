"""K-means and MAUVE, the part that needs no GPU: validation before any device call (hip_ops.kmeans_assign / kmeans_update,
kmeans, mauve_score), the new names in header / signature table / package, the error paths and workspace queries of the two
entry points, mauve_from_histograms against closed forms, and the compile-time resource check of csrc/kmeans.hip (no
scratch memory, two instantiations of the assign tile kernel, two workgroups per CU)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import kmeans_reference as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-metrics_amd", "csrc")
BAD_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -4
FAKE = ctypes.c_void_p(0x10000)                       # 16-byte aligned, never dereferenced: the calls stop at validation
NAMES = ("am_kmeans_assign_workspace_bytes", "am_kmeans_assign_f32", "am_kmeans_update_workspace_bytes", "am_kmeans_update_f32")


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


# ---------------------------------------------------------------------------------------------------- validation
def test_validation_happens_before_any_device_call(am, monkeypatch):
    from audio_metrics_amd import hip_ops

    def forbidden(*a, **k):
        raise AssertionError("device call before validation")
    for name in ("as_matrix", "_call", "_workspace"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    x, c = torch.zeros((10, 8)), torch.zeros((3, 8))
    labels = torch.zeros(10, dtype=torch.int64)
    for call in (lambda a, b: hip_ops.kmeans_assign(a, b), lambda a, b: hip_ops.kmeans_update(a, labels, b)):
        with pytest.raises(NotImplementedError, match=r"takes float32 rows \(the float64 matrix-core form is not implemented\)"):
            call(x.double(), c)
        with pytest.raises(NotImplementedError, match="float32 rows"):
            call(x, c.double())
        with pytest.raises(ValueError, match="feature widths"):
            call(x, torch.zeros((3, 12)))
        with pytest.raises(ValueError, match="2-D"):
            call(torch.zeros(8), c)
        with pytest.raises(ValueError, match="2-D"):
            call(x, torch.zeros((1, 3, 8)))
        with pytest.raises(ValueError, match="K=0"):
            call(x, torch.zeros((0, 8)))
    with pytest.raises(ValueError, match="one entry per row"):
        hip_ops.kmeans_update(x, labels[:9], c)
    with pytest.raises(ValueError, match="int64"):
        hip_ops.kmeans_update(x, labels.to(torch.int32), c)
    # the front ends: with the two operations themselves forbidden too
    monkeypatch.setattr(hip_ops, "kmeans_assign", forbidden)
    monkeypatch.setattr(hip_ops, "kmeans_update", forbidden)
    for rows in (x, host_set(am, x)):
        with pytest.raises(ValueError, match="exceeds the number of rows"):
            am.kmeans(rows, 11)
        for bad in (0, -2):
            with pytest.raises(ValueError, match="at least 1"):
                am.kmeans(rows, bad)
    for bad in (float("nan"), float("inf")):
        rows = torch.zeros((10, 8))
        rows[4, 3] = bad
        with pytest.raises(ValueError, match="non-finite"):
            am.kmeans(rows, 2)
    with pytest.raises(NotImplementedError, match="float64"):
        am.kmeans(x.double(), 2)
    with pytest.raises(ValueError, match="2-D"):
        am.kmeans(torch.zeros(8), 2)
    with pytest.raises(ValueError, match="keeps none"):
        am.kmeans(am.AudioMetricsData(False), 2)
    with pytest.raises(ValueError, match=r"init must be a \[2, 8\]"):
        am.kmeans(x, 2, init=torch.zeros((3, 8)))
    ok, other = host_set(am, x), host_set(am, torch.zeros((12, 8)))
    with pytest.raises(NotImplementedError, match="float64"):
        am.mauve_score(host_set(am, x.double()), ok)
    with pytest.raises(NotImplementedError, match="float64"):
        am.mauve_score(ok, host_set(am, x.double()))
    with pytest.raises(ValueError, match="feature widths"):
        am.mauve_score(ok, host_set(am, torch.zeros((10, 12))))
    with pytest.raises(ValueError, match="keeps none"):
        am.mauve_score(ok, am.AudioMetricsData(False))
    with pytest.raises(ValueError, match="exceeds the number of rows"):
        am.mauve_score(ok, other, n_clusters=23)
    with pytest.raises(ValueError, match="at least 1"):
        am.mauve_score(ok, other, n_clusters=0)
    rows = torch.zeros((12, 8))
    rows[0, 0] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        am.mauve_score(ok, host_set(am, rows))


# ---------------------------------------------------------------------------------------------------- names
def test_header_signature_table_and_package_agree(am, lib):
    with open(os.path.join(ROOT, "include", "audio_metrics_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in am._lib.SIGNATURES and hasattr(lib, name), name
    assert len(am._lib.SIGNATURES["am_kmeans_assign_f32"][1]) == 13
    assert len(am._lib.SIGNATURES["am_kmeans_update_f32"][1]) == 16
    from audio_metrics_amd.metrics import mauve
    assert am.kmeans is mauve.kmeans and am.mauve_score is mauve.mauve_score
    assert am.mauve_from_histograms is mauve.mauve_from_histograms and am.metrics.mauve is mauve
    assert callable(am.hip_ops.kmeans_assign) and callable(am.hip_ops.kmeans_update)


# ---------------------------------------------------------------------------------------------------- entry points
def test_assign_error_paths(lib):
    n, k, d = 1000, 300, 64
    nb = lib.am_kmeans_assign_workspace_bytes(n, k, d)
    assert nb > 0

    def call(x=FAKE, n=n, ldx=d, c=FAKE, k=k, ldc=d, d=d, labels=FAKE, d2=FAKE, inertia=FAKE, ws=FAKE, nb=nb):
        return lib.am_kmeans_assign_f32(x, n, ldx, c, k, ldc, d, labels, d2, inertia, ws, nb, None)
    assert call(x=None) == BAD_ARG and call(c=None) == BAD_ARG
    for arg in ("labels", "d2", "inertia"):
        assert call(**{arg: None}) == BAD_ARG and "%s is null" % arg in lib.am_last_error().decode()
    assert call(n=0) == BAD_SHAPE and call(k=0) == BAD_SHAPE and call(d=0) == BAD_SHAPE
    # the alignment / leading-dimension rules of am_knn_search_f32
    assert call(ldx=d - 4) == BAD_ARG and call(ldc=d + 1) == BAD_ARG
    assert call(x=ctypes.c_void_p(0x10004)) == BAD_ARG and call(c=ctypes.c_void_p(0x10008)) == BAD_ARG
    assert call(k=(1 << 32) - 1) == BAD_SHAPE and "2^32" in lib.am_last_error().decode()     # an index takes 32 bits of a key
    assert call(nb=nb - 1) == WORKSPACE and str(nb) in lib.am_last_error().decode()
    assert call(ws=None) == WORKSPACE and call(nb=0) == WORKSPACE


def test_update_error_paths(lib):
    n, k, d = 1000, 20, 40
    nb = lib.am_kmeans_update_workspace_bytes(n, k, d)
    assert nb > 0

    def call(x=FAKE, n=n, ldx=d, d=d, labels=FAKE, order=FAKE, offsets=FAKE, k=k, c_old=FAKE, ldo=d, c_new=FAKE, ldn=d,
             counts=FAKE, ws=FAKE, nb=nb):
        return lib.am_kmeans_update_f32(x, n, ldx, d, labels, order, offsets, k, c_old, ldo, c_new, ldn, counts, ws, nb, None)
    assert call(x=None) == BAD_ARG and call(c_old=None) == BAD_ARG and call(c_new=None) == BAD_ARG
    for arg in ("labels", "order", "offsets", "counts"):
        assert call(**{arg: None}) == BAD_ARG and "%s is null" % arg in lib.am_last_error().decode()
    assert call(n=0) == BAD_SHAPE and call(k=0) == BAD_SHAPE and call(d=0) == BAD_SHAPE
    assert call(ldx=d - 4) == BAD_ARG and call(ldo=d + 1) == BAD_ARG and call(ldn=d + 2) == BAD_ARG
    assert call(x=ctypes.c_void_p(0x10004)) == BAD_ARG and call(c_new=ctypes.c_void_p(0x10004)) == BAD_ARG
    assert call(nb=nb - 1) == WORKSPACE and str(nb) in lib.am_last_error().decode()
    assert call(ws=None) == WORKSPACE and call(nb=0) == WORKSPACE


def test_workspace_queries(lib):
    for bad in ((0, 10, 8), (10, 0, 8), (10, 10, 0), (10, (1 << 32) - 1, 8)):
        assert lib.am_kmeans_assign_workspace_bytes(*bad) == 0, bad
    for bad in ((0, 10, 8), (10, 0, 8), (10, 10, 0)):
        assert lib.am_kmeans_update_workspace_bytes(*bad) == 0, bad
    # assign: the norms, ONE key per row and column chunk (the plan of the search), one f64 per 256 rows
    for n, k, d in ((1000, 5000, 64), (130, 300, 40), (200_000, 10_000, 512)):
        chunks = lib.am_knn_search_chunks(n, k, d, 1)
        want = chunks * n * 8 + (n + k) * 4 + (n + 255) // 256 * 8
        nb = lib.am_kmeans_assign_workspace_bytes(n, k, d)
        assert want <= nb <= want + 4 * 256, (n, k, d, nb)
        assert nb < lib.am_knn_search_workspace_bytes(n, k, d, 1)                 # the search keeps 8 keys where this keeps 1
    # update: f64 [segments of 64 rows][2][D rounded up to 4]
    for n, k, d in ((5000, 3, 40), (1000, 20, 64), (130, 7, 41)):
        want = (n + 63) // 64 * 2 * ((d + 3) // 4 * 4) * 8
        assert want <= lib.am_kmeans_update_workspace_bytes(n, k, d) <= want + 256, (n, k, d)


# ---------------------------------------------------------------------------------------------------- the frontier
def test_equal_histograms_score_exactly_one(am):
    f = am.mauve_from_histograms
    for p in ([1], [3, 4, 5], [1, 0, 7, 0], np.random.default_rng(0).integers(0, 50, 300)):
        assert f(p, p) == 1.0
        assert f(p, np.asarray(p) * 3) == 1.0                                    # counts, not probabilities: the totals cancel
        assert f(p, p, scaling=2.0, n_points=7) == 1.0


def test_disjoint_supports_follow_the_closed_form(am):
    f = am.mauve_from_histograms
    for scaling, n_points in ((5.0, 25), (1.0, 25), (5.0, 100), (2.5, 3)):
        want = kr.disjoint_mauve(scaling, n_points)
        for p, q in (([1, 0], [0, 1]), ([5, 3, 0, 0, 0], [0, 0, 9, 1, 4]), ([0, 2, 0, 2], [7, 0, 1, 0])):
            assert abs(f(p, q, scaling, n_points) - want) <= 1e-12, (scaling, n_points, p, q)
        score, pts = f([1, 0], [0, 1], scaling, n_points, return_points=True)
        lam = np.linspace(1e-6, 1 - 1e-6, n_points)
        got = pts[1:-1]                                                           # sorted by x = (1 - lambda)^s: lambda descending
        assert np.allclose(got[:, 0], ((1 - lam) ** scaling)[::-1], rtol=1e-12, atol=0)
        assert np.allclose(got[:, 1], (lam ** scaling)[::-1], rtol=1e-12, atol=0)
        assert tuple(pts[0]) == (0.0, 1.0) and tuple(pts[-1]) == (1.0, 0.0)
    assert 0.0 < kr.disjoint_mauve(5.0, 25) < 0.01


def test_symmetry_monotonicity_and_empty_bins(am):
    f = am.mauve_from_histograms
    rng = np.random.default_rng(1)
    for _ in range(20):
        p, q = rng.integers(0, 30, 40), rng.integers(0, 30, 40)
        assert abs(f(p, q) - f(q, p)) <= 1e-12
        assert 0.0 < f(p, q) <= 1.0
    # a histogram moving away from [8, 4, 2, 1, 0, 0, 0, 0] one step at a time: the score falls strictly
    base = np.array([8, 4, 2, 1, 0, 0, 0, 0])
    scores = [f(base, np.roll(base, s)) for s in range(5)]
    assert scores[0] == 1.0 and all(a > b for a, b in zip(scores, scores[1:])), scores
    mass = [f([100, 0], [100 - t, t]) for t in (0, 10, 30, 60, 90, 100)]
    assert mass[0] == 1.0 and all(a > b for a, b in zip(mass, mass[1:])), mass
    # bins that are empty in both sets change nothing
    p, q = np.array([5, 0, 3, 2]), np.array([1, 4, 0, 5])
    wide_p, wide_q = np.array([0, 5, 0, 0, 3, 0, 2, 0]), np.array([0, 1, 4, 0, 0, 0, 5, 0])
    assert f(wide_p, wide_q) == f(p, q)
    with pytest.raises(ValueError, match="same bins"):
        f([1, 2], [1, 2, 3])
    with pytest.raises(ValueError, match="positive total"):
        f([0, 0], [1, 2])


# ---------------------------------------------------------------------------------------------------- the kernels' resources
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_kmeans_kernels_use_no_scratch_memory():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    import importlib.util
    spec = importlib.util.spec_from_file_location("am_build", os.path.join(ROOT, "audio-metrics_amd", "_build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)                                         # the flags the shipped library is built with
    r = subprocess.run([hipcc, *build.HIPCC_FLAGS, "--cuda-device-only", "-c", "kmeans.hip", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, timeout=900)
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
    ours = {n: u for n, u in usage.items() if "kmeans" in n}
    for part in ("kmeans_assign_kernel", "kmeans_assign_merge_kernel", "kmeans_inertia_kernel", "kmeans_update_kernel",
                 "kmeans_update_finish_kernel"):
        assert any(part in n for n in ours), (part, sorted(usage))
    for n, u in ours.items():
        assert u["scratch"] == 0, (n, u)
    tile = {n: u for n, u in ours.items() if "kmeans_assign_kernel" in n}
    assert len(tile) == 2 and sorted("ILb1E" in n for n in tile) == [False, True], sorted(tile)     # without / with the inner tail
    for n, u in tile.items():
        assert u["vgprs"] <= 256 and u["occupancy"] >= 2, (n, u)           # two workgroups of four waves per CU
