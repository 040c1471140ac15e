"""Multi-scale kernel sums, the part that needs no GPU: the host oracle the GPU tests lean on, validation before any device
call (hip_ops.mmd_multi_sums, kernel_audio_distance_multiscale, energy_distance), how a long scale grid is cut into library
calls, the new names in header / signature table / package, the error paths and workspace query of am_mmd_multi_f32, and the
compile-time resource check of csrc/mmd_multi.hip (no scratch memory in any instantiation, two workgroups per CU)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import kad_reference as ka
import kd_reference as kr
import mmd_multi_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-metrics_amd", "csrc")
BAD_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -4
FAKE = ctypes.c_void_p(0x10000)                       # 16-byte aligned, never dereferenced: the calls stop at validation
NAMES = ("am_mmd_multi_workspace_bytes", "am_mmd_multi_f32")


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
def test_gaussian_oracle_at_scale_one_is_the_kad_oracle():
    rng = np.random.default_rng(3)
    x, y = kr.rbf_rows(rng, 40, 32, 10.0), kr.rbf_rows(rng, 55, 32, 10.0)
    for bw2 in (100.0, 37.5):
        means, scale = mr.parts(x, y, "gaussian", bw2, 1.0)
        want, want_scale = ka.mmd_parts(x, y, 0.5 / bw2)
        assert (means == want).all() and scale == want_scale
    # a scale c is the bandwidth c * bw
    means, _ = mr.parts(x, y, "gaussian", 100.0, 2.0)
    want, _ = ka.mmd_parts(x, y, 0.5 / 400.0)
    assert (means == want).all()


def test_oracle_against_a_direct_double_loop():
    rng = np.random.default_rng(4)
    x, y = kr.rbf_rows(rng, 5, 16, 10.0), kr.rbf_rows(rng, 7, 16, 10.0)

    def dist(a, b):
        return np.sqrt(((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum())
    for kind, k in (("laplacian", lambda a, b: np.exp(-dist(a, b) / (0.5 * 10.0))), ("energy", lambda a, b: -dist(a, b))):
        sxx = sum(k(x[i], x[j]) for i in range(5) for j in range(5) if i != j)
        syy = sum(k(y[i], y[j]) for i in range(7) for j in range(7) if i != j)
        sxy = sum(k(a, b) for a in x for b in y)
        means, scale = mr.parts(x, y, kind, 100.0, 0.5)
        np.testing.assert_allclose(means, [sxx / 20, syy / 42, sxy / 35], rtol=1e-14)
        assert scale > 0.0


def test_energy_distance_of_a_shifted_copy_is_positive():
    x = kr.rbf_rows(np.random.default_rng(5), 60, 32, 10.0)
    shifted = x + np.float32(2.0)
    means, _ = mr.parts(x, shifted, "energy")
    assert (means < 0.0).all()                                         # k = -d
    assert mr.energy_from_means(means) > 0.0
    same, _ = mr.parts(x, x, "energy")
    assert mr.energy_from_means(same) < 0.0                            # the unbiased estimate of 0 drops the diagonal of Kxx / Kyy only


def test_mixture_is_the_mean_of_its_scales():
    rng = np.random.default_rng(6)
    x, y = kr.rbf_rows(rng, 30, 32, 10.0), kr.rbf_rows(rng, 45, 32, 10.0)
    scales = (0.5, 1.0, 2.0, 4.0)
    for kind in ("gaussian", "laplacian"):
        per_scale = np.array([mr.parts(x, y, kind, 100.0, c)[0] for c in scales])
        mixture = mr.mixture_parts(x, y, kind, 100.0, scales)
        np.testing.assert_allclose(mixture, per_scale.mean(0), rtol=1e-14)
        assert abs(ka.mmd2(mixture) - np.mean([ka.mmd2(p) for p in per_scale])) <= 1e-15


# ---------------------------------------------------------------------------------------------------- validation
def test_validation_happens_before_any_device_call(am, monkeypatch):
    from audio_metrics_amd import hip_ops

    def forbidden(*a, **k):
        raise AssertionError("device call before validation")
    for name in ("as_matrix", "_call", "_workspace"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    x, y = torch.zeros((10, 8)), torch.zeros((12, 8))

    def sums(a=x, b=y, kernel="gaussian", scales=(1.0,), bw2=1.0, **kw):
        return hip_ops.mmd_multi_sums(a, b, kernel, scales, bw2=bw2, **kw)
    with pytest.raises(NotImplementedError, match="float32 rows"):
        sums(a=x.double())
    with pytest.raises(NotImplementedError, match="float32 rows"):
        sums(b=y.double())
    with pytest.raises(NotImplementedError, match="float32 rows"):
        sums(a=x.double(), b=y.double())
    with pytest.raises(ValueError, match="feature widths"):
        sums(b=torch.zeros((12, 12)))
    with pytest.raises(ValueError, match="2-D"):
        sums(a=torch.zeros(8))
    for bad in ("rbf", "Gaussian", None, 0):
        with pytest.raises(ValueError, match="kernel="):
            sums(kernel=bad)
    with pytest.raises(ValueError, match="empty"):
        sums(scales=())
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite and positive"):
            sums(scales=(1.0, bad))
        with pytest.raises(ValueError, match="bw2"):
            sums(bw2=bad)
    with pytest.raises(ValueError, match="needs bw2"):
        sums(bw2=None)
    with pytest.raises(ValueError, match="one scale"):
        sums(kernel="energy", scales=(1.0, 2.0))
    for bad in (0, 8):
        with pytest.raises(ValueError, match="blocks"):
            sums(blocks=bad)
    # the front ends: with the operations they are built from forbidden too
    for name in ("mmd_multi_sums", "pairwise_select_sq", "mmd_rbf_sums"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    ok, ref = host_set(am, x), host_set(am, y)
    for call in (am.kernel_audio_distance_multiscale, am.energy_distance):
        with pytest.raises(NotImplementedError, match="float64"):
            call(host_set(am, x.double()), ref)
        with pytest.raises(NotImplementedError, match="float64"):
            call(ok, host_set(am, y.double()))
        with pytest.raises(NotImplementedError, match="float64"):
            call(host_set(am, x.double()), host_set(am, y.double()))
        with pytest.raises(ValueError, match="feature widths"):
            call(ok, host_set(am, torch.zeros((12, 12))))
        with pytest.raises(ValueError, match="at least 2 rows in the candidate"):
            call(host_set(am, torch.zeros((1, 8))), ref)
        with pytest.raises(ValueError, match="at least 2 rows in the reference"):
            call(ok, host_set(am, torch.zeros((1, 8))))
        with pytest.raises(ValueError, match="keeps none"):
            call(am.AudioMetricsData(False), ref)
        with pytest.raises(ValueError, match="keeps none"):
            call(ok, am.AudioMetricsData(False))
    multi = am.kernel_audio_distance_multiscale
    for bad in ("rbf", "energy", None):
        with pytest.raises(ValueError, match="kernel="):
            multi(ok, ref, kernel=bad)
    with pytest.raises(ValueError, match="empty"):
        multi(ok, ref, scales=())
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite and positive"):
            multi(ok, ref, scales=(0.5, bad))
        with pytest.raises(ValueError, match="bandwidth"):
            multi(ok, ref, bandwidth=bad)
    with pytest.raises(ValueError, match="at most 16"):
        multi(ok, ref, scales=[1.0 + 0.1 * j for j in range(17)])


# ---------------------------------------------------------------------------------------------------- the split
def recorded_calls(monkeypatch, lib):
    """hip_ops on host tensors with the library call replaced: every call is recorded and fills the [3][k] doubles behind its
    out_sums pointer with 1000 * call + 10 * block + column for the blocks it names."""
    from audio_metrics_amd import hip_ops
    calls = []

    def fake_call(lib_, name, device, *args):
        xp, n, ldx, yp, m, ldy, d, kind, bw2_dev, bw2, scales, k, blocks, out, ws, nb = args
        grid = list((ctypes.c_double * k).from_address(scales.value))
        dst = (ctypes.c_double * (3 * k)).from_address(out.value)
        for b in range(3):
            if blocks & (1 << b):
                for j in range(k):
                    dst[b * k + j] = 1000.0 * len(calls) + 10.0 * b + j
        calls.append({"name": name, "kind": kind, "scales": grid, "blocks": blocks, "bw2": bw2, "nb": nb,
                      "want_nb": lib.am_mmd_multi_workspace_bytes(n, m, d, k, blocks)})
    monkeypatch.setattr(hip_ops, "_require_cuda", lambda t, name: None)
    monkeypatch.setattr(hip_ops, "_call", fake_call)
    return hip_ops, calls


@pytest.mark.parametrize("blocks", [7, 5, 2])
def test_a_long_grid_is_cut_into_calls_of_at_most_four_scales(lib, monkeypatch, blocks):
    ops, calls = recorded_calls(monkeypatch, lib)
    x, y = torch.zeros((10, 8)), torch.zeros((12, 8))
    grid = (0.25, 0.5, 1.0, 2.0, 4.0, 8.0)
    out = ops.mmd_multi_sums(x, y, "laplacian", grid, bw2=2.5, blocks=blocks)
    assert [c["scales"] for c in calls] == [[0.25, 0.5, 1.0, 2.0], [4.0, 8.0]]
    assert all(c["name"] == "am_mmd_multi_f32" and c["kind"] == 1 and c["blocks"] == blocks and c["bw2"] == 2.5 for c in calls)
    assert all(c["nb"] == c["want_nb"] > 0 for c in calls)
    assert out.dtype == torch.float64 and tuple(out.shape) == (3, 6)
    for b in range(3):
        for j in range(6):
            call, col = divmod(j, 4)
            got = out[b, j].item()
            if blocks & (1 << b):
                assert got == 1000.0 * call + 10.0 * b + col, (b, j)      # each call wrote its own columns, and only those
            else:
                assert np.isnan(got), (b, j)                               # a block that was not asked for: the fresh tensor's NaN
    # a caller's tensor keeps what it held in the blocks that were not asked for
    calls.clear()
    mine = torch.full((3, 6), -7.5, dtype=torch.float64)
    assert ops.mmd_multi_sums(x, y, "gaussian", grid, bw2=2.5, blocks=blocks, out=mine) is mine
    for b in range(3):
        assert ((mine[b] == -7.5).all().item()) == (not blocks & (1 << b)), b
    with pytest.raises(ValueError, match=r"\[3, 6\]"):
        ops.mmd_multi_sums(x, y, "gaussian", grid, bw2=2.5, out=torch.zeros((3, 5), dtype=torch.float64))


def test_a_grid_of_four_is_one_call_that_writes_the_result_itself(lib, monkeypatch):
    ops, calls = recorded_calls(monkeypatch, lib)
    x, y = torch.zeros((10, 8)), torch.zeros((12, 8))
    out = ops.mmd_multi_sums(x, y, "gaussian", (0.5, 1.0, 2.0, 4.0), bw2=2.5)
    assert [c["scales"] for c in calls] == [[0.5, 1.0, 2.0, 4.0]]
    assert out.tolist() == [[0.0, 1.0, 2.0, 3.0], [10.0, 11.0, 12.0, 13.0], [20.0, 21.0, 22.0, 23.0]]
    calls.clear()
    out = ops.mmd_multi_sums(x, y, "energy", (1.0,), blocks=4)
    assert len(calls) == 1 and calls[0]["kind"] == 2 and calls[0]["scales"] == [1.0]
    assert np.isnan(out[0, 0].item()) and np.isnan(out[1, 0].item()) and out[2, 0].item() == 20.0
    calls.clear()
    ops.mmd_multi_sums(x, y, "gaussian", [1.0 + j for j in range(9)], bw2=1.0)
    assert [len(c["scales"]) for c in calls] == [4, 4, 1]


# ---------------------------------------------------------------------------------------------------- names
def test_header_signature_table_and_package_agree(am, lib):
    with open(os.path.join(ROOT, "include", "audio_metrics_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in am._lib.SIGNATURES and hasattr(lib, name), name
    assert len(am._lib.SIGNATURES["am_mmd_multi_f32"][1]) == 17
    assert re.search(r"AM_MMD_GAUSSIAN = 0, AM_MMD_LAPLACIAN = 1, AM_MMD_ENERGY = 2", header)
    assert re.search(r"#define AM_MMD_MULTI_MAX 4\b", header)
    assert am.hip_ops.MMD_KERNELS == {"gaussian": 0, "laplacian": 1, "energy": 2} and am.hip_ops.MMD_MULTI_MAX == 4
    from audio_metrics_amd.metrics import mmd
    assert am.kernel_audio_distance_multiscale is mmd.kernel_audio_distance_multiscale
    assert am.energy_distance is mmd.energy_distance and am.metrics.mmd is mmd
    assert callable(am.hip_ops.mmd_multi_sums)
    from audio_metrics_amd import audio_metrics as front                   # neither becomes a metric name of AudioMetrics
    assert not any("multiscale" in k or "energy" in k for k, _ in front.EVALUATION_TABLE)


# ---------------------------------------------------------------------------------------------------- entry point
def test_error_paths(lib):
    n1, n2, d = 1000, 300, 64
    nb = lib.am_mmd_multi_workspace_bytes(n1, n2, d, 4, 7)
    assert nb > 0
    four = (ctypes.c_double * 4)(0.5, 1.0, 2.0, 4.0)

    def call(x=FAKE, n1=n1, ldx=d, y=FAKE, n2=n2, ldy=d, d=d, kernel=0, bw2_dev=None, bw2=1.5, scales=four, k=4, blocks=7, out=FAKE,
             ws=FAKE, nb=nb):
        return lib.am_mmd_multi_f32(x, n1, ldx, y, n2, ldy, d, kernel, bw2_dev, bw2, ctypes.cast(scales, ctypes.c_void_p) if scales else None,
                                    k, blocks, out, ws, nb, None)
    assert call(x=None) == BAD_ARG and call(y=None) == BAD_ARG and call(out=None) == BAD_ARG and call(scales=None) == BAD_ARG
    assert "null" in lib.am_last_error().decode()
    assert call(blocks=0) == BAD_ARG and call(blocks=8) == BAD_ARG
    assert call(kernel=3) == BAD_ARG and call(kernel=-1) == BAD_ARG and "AM_MMD_GAUSSIAN" in lib.am_last_error().decode()
    assert call(n1=0) == BAD_SHAPE and call(n2=0) == BAD_SHAPE and call(d=0) == BAD_SHAPE
    assert call(k=0) == BAD_SHAPE and call(k=5) == BAD_SHAPE and "AM_MMD_MULTI_MAX" in lib.am_last_error().decode()
    assert call(kernel=2, k=2) == BAD_SHAPE and "energy" in lib.am_last_error().decode()
    assert call(ldx=d - 4) == BAD_ARG and call(ldy=d + 2) == BAD_ARG
    assert call(x=ctypes.c_void_p(0x10004)) == BAD_ARG and call(y=ctypes.c_void_p(0x10008)) == BAD_ARG
    big = 1 << 24
    assert call(n1=big, nb=1 << 40) == BAD_SHAPE and "4 GiB" in lib.am_last_error().decode()
    assert call(n2=big, nb=1 << 40) == BAD_SHAPE
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(scales=(ctypes.c_double * 4)(0.5, 1.0, bad, 4.0)) == BAD_ARG and "scales[2]" in lib.am_last_error().decode()
        assert call(bw2=bad) == BAD_ARG and "bw2" in lib.am_last_error().decode()
        assert call(kernel=1, bw2=bad) == BAD_ARG
        # a device bandwidth replaces the host one; the energy kernel takes neither: both stop at the workspace check
        assert call(bw2=bad, bw2_dev=FAKE, nb=nb - 1) == WORKSPACE
        assert call(kernel=2, k=1, bw2=bad, nb=0) == WORKSPACE
    assert call(nb=nb - 1) == WORKSPACE and str(nb) in lib.am_last_error().decode()
    assert call(ws=None) == WORKSPACE and call(nb=0) == WORKSPACE
    # a mask and a scale count need the workspace of their own blocks and scales only
    assert call(blocks=4, nb=lib.am_mmd_multi_workspace_bytes(n1, n2, d, 4, 4) - 1) == WORKSPACE
    assert call(k=1, nb=lib.am_mmd_multi_workspace_bytes(n1, n2, d, 1, 7) - 1) == WORKSPACE


def test_workspace_query(lib):
    q = lib.am_mmd_multi_workspace_bytes
    for bad in ((0, 10, 64, 1, 7), (10, 0, 64, 1, 7), (10, 10, 0, 1, 7), (10, 10, 64, 0, 7), (10, 10, 64, 5, 7), (10, 10, 64, 1, 0)):
        assert q(*bad) == 0, bad
    # one scale: the norms and one partial per workgroup, as am_mmd_rbf_f32; each further scale adds its partials only
    for n1, n2, d in ((1000, 300, 64), (20_000, 20_000, 512), (129, 5000, 100)):
        for blocks in range(1, 8):
            assert q(n1, n2, d, 1, blocks) == lib.am_mmd_rbf_workspace_bytes(n1, n2, d, blocks), (n1, n2, d, blocks)
            sizes = [q(n1, n2, d, k, blocks) for k in (1, 2, 3, 4)]
            assert sizes == sorted(sizes) and sizes[3] <= 4 * sizes[0], (n1, n2, d, blocks, sizes)


# ---------------------------------------------------------------------------------------------------- the kernels' resources
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_no_instantiation_uses_scratch_memory():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    import importlib.util
    spec = importlib.util.spec_from_file_location("am_build", os.path.join(ROOT, "audio-metrics_amd", "_build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)                                         # the flags the shipped library is built with
    r = subprocess.run([hipcc, *build.HIPCC_FLAGS, "--cuda-device-only", "-c", "mmd_multi.hip", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, timeout=1500)
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
    ours = {n: u for n, u in usage.items() if "mmd_multi" in n}
    tile = {n: u for n, u in ours.items() if "mmd_multi_kernel" in n}
    # what the file declares: Gaussian and Laplacian for 1 .. AM_MMD_MULTI_MAX scales, the energy kernel for one, each without /
    # with the inner-dimension tail
    with open(os.path.join(ROOT, "include", "audio_metrics_hip.h")) as f:
        most = int(re.search(r"#define AM_MMD_MULTI_MAX (\d+)", f.read()).group(1))
    want = {"ILi%dELi%dELb%dE" % (kind, s, tail) for kind in (0, 1) for s in range(1, most + 1) for tail in (0, 1)}
    want |= {"ILi2ELi1ELb%dE" % tail for tail in (0, 1)}
    assert len(tile) == len(want) == 2 * (2 * most + 1), sorted(tile)
    for tag in want:
        assert sum(tag in n for n in tile) == 1, (tag, sorted(tile))
    assert len(ours) == len(tile) + 1 and any("mmd_multi_reduce_kernel" in n for n in ours), sorted(ours)
    for n, u in ours.items():
        print(n, u)
        assert u["scratch"] == 0, (n, u)
        assert u["vgprs"] <= 256 and u["occupancy"] >= 2, (n, u)           # two workgroups of four waves per CU
