"""Per-group Kernel Audio Distance, the part that needs no GPU: the host oracle, the error paths of the new entry point
(validated before the first HIP call, so fake pointers do), its workspace query, validation of the front end before any
device call, the host-side combination step (single-row groups, NaN sums), the export, and the compile-time resources of
csrc/kad_groups.hip (no scratch memory, two workgroups per CU for the tile kernels)."""
import ctypes
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

import kad_groups_reference as kg
import kd_reference as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-metrics_amd", "csrc")
BAD_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -4
FAKE = ctypes.c_void_p(0x10000)                       # 16-byte aligned, never dereferenced: the calls stop at validation
ENTRY_POINTS = ("am_mmd_rbf_groups_workspace_bytes", "am_mmd_rbf_groups_f32")


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    return audio_metrics_amd


@pytest.fixture(scope="module")
def lib(am):
    return am._lib.load()


# ---------------------------------------------------------------------------------------------------- oracle
def test_oracle_against_a_direct_double_loop():
    rng = np.random.default_rng(41)
    x, y = kr.rbf_rows(rng, 9, 16, 10.0), kr.rbf_rows(rng, 6, 16, 10.0)
    g = 1.0 / 200.0
    offs = kg.offsets_of([1, 3, 5])

    def k(a, b):
        return np.exp(-((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum() * g)
    o = kg.group_sums(x, offs, y, g)
    for b in range(3):
        members = range(int(offs[b]), int(offs[b + 1]))
        sxx = sum(k(x[i], x[j]) for i in members for j in members if i != j)
        sxy = sum(k(x[i], yj) for i in members for yj in y)
        np.testing.assert_allclose([o["sxx"][b], o["sxy"][b]], [sxx, sxy], rtol=1e-14, atol=0)
        for i in members:
            np.testing.assert_allclose(o["w"][i], sum(k(x[i], x[j]) for j in members if j != i), rtol=1e-14)
            np.testing.assert_allclose(o["c"][i], sum(k(x[i], yj) for yj in y), rtol=1e-14)
    assert o["sxx"][0] == 0.0 and np.isnan(o["mean_xx"][0]) and np.isfinite(o["mean_xx"][1:]).all()
    np.testing.assert_allclose(o["mean_xx"][1:], o["sxx"][1:] / np.array([6.0, 20.0]), rtol=1e-15)
    np.testing.assert_allclose(o["mean_xy"], o["sxy"] / (np.array([1.0, 3.0, 5.0]) * 6), rtol=1e-15)
    assert 0.0 < o["scale"] <= 1.0
    # the normalisations of a device record are the oracle's own
    xx, xy = kg.device_means(np.stack([o["sxx"], o["sxy"]], axis=1), [1, 3, 5], 6)
    np.testing.assert_array_equal(xx[1:], o["mean_xx"][1:])
    np.testing.assert_array_equal(xy, o["mean_xy"])
    wr, cr = kg.row_means(np.stack([o["w"], o["c"]], axis=1), offs, 6)
    assert np.isnan(wr[0]) and wr[1] == o["w"][1] / 2.0 and cr[8] == o["c"][8] / 6.0
    # one group = the whole-set sums; an emulated dot-product matrix is honoured
    import kad_reference as ka
    whole = kg.group_sums(x, [0, 9], y, g)
    means, _ = ka.mmd_parts(x, y, g)
    np.testing.assert_allclose([whole["mean_xx"][0], whole["mean_xy"][0]], [means[0], means[2]], rtol=1e-14)
    emu = kg.group_sums(x, offs, y, g, dots=kr.emulated_dots("f32"))
    np.testing.assert_allclose(emu["sxy"], o["sxy"], rtol=1e-12)       # exact data: the emulated dot products are exact


# ---------------------------------------------------------------------------------------------------- C ABI without a device
def test_header_exports_and_signature_table_agree(am, lib):
    with open(os.path.join(ROOT, "include", "audio_metrics_hip.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in am._lib.SIGNATURES and hasattr(lib, name), name


def _offsets(values):
    return (ctypes.c_int64 * len(values))(*[int(v) for v in values])


def test_error_paths(lib):
    n1, n2, d, sizes = 1000, 300, 64, [5, 300, 1, 50]
    nb = lib.am_mmd_rbf_groups_workspace_bytes(sum(sizes), len(sizes), n2, d)
    assert nb > 0

    def call(x=FAKE, n1=n1, ldx=d, idx=FAKE, offs=None, b=None, y=FAKE, n2=n2, ldy=d, d=d, bw2=None, gamma=0.5, out=FAKE, rows=None,
             ws=FAKE, nb=nb):
        offs = kg.offsets_of(sizes) if offs is None else offs
        arr = _offsets(offs)
        return lib.am_mmd_rbf_groups_f32(x, n1, ldx, idx, ctypes.cast(arr, ctypes.c_void_p), len(offs) - 1 if b is None else b, y, n2, ldy,
                                         d, bw2, gamma, out, rows, ws, nb, None)
    for kw in ("x", "y", "out"):
        assert call(**{kw: None}) == BAD_ARG, kw
        assert "null" in lib.am_last_error().decode()
    assert lib.am_mmd_rbf_groups_f32(FAKE, n1, d, FAKE, None, 1, FAKE, n2, d, d, None, 0.5, FAKE, None, FAKE, nb, None) == BAD_ARG
    # offsets: start at 0, increase strictly
    assert call(offs=[1, 5, 9]) == BAD_ARG and "offsets[0]" in lib.am_last_error().decode()
    assert call(offs=[0, 5, 5, 9]) == BAD_SHAPE and "group 1 " in lib.am_last_error().decode()
    assert call(offs=[0, 5, 4, 9]) == BAD_SHAPE and "group 1 " in lib.am_last_error().decode()
    # shapes
    assert call(b=0) == BAD_SHAPE and "B=0" in lib.am_last_error().decode()
    assert call(d=0) == BAD_SHAPE and call(n1=0) == BAD_SHAPE
    assert call(n2=1) == BAD_SHAPE and "N2=1" in lib.am_last_error().decode()
    assert call(n2=0) == BAD_SHAPE
    # alignment and leading dimensions
    assert call(ldx=d - 4) == BAD_ARG and call(ldy=d + 2) == BAD_ARG and call(x=ctypes.c_void_p(0x10004)) == BAD_ARG
    assert call(gamma=-1.0) == BAD_ARG and "gamma" in lib.am_last_error().decode()
    assert call(gamma=-1.0, bw2=FAKE, nb=nb - 1) == WORKSPACE            # a device bandwidth replaces gamma
    # the 4 GiB rule, either set
    big = 1 << 24
    assert call(n1=big, nb=1 << 40) == BAD_SHAPE and "4 GiB" in lib.am_last_error().decode()
    assert call(n2=big, nb=1 << 40) == BAD_SHAPE and "4 GiB" in lib.am_last_error().decode()
    # without an index list the groups are stored rows: they must exist
    assert call(idx=None, n1=sum(sizes) - 1) == BAD_SHAPE and "stored rows" in lib.am_last_error().decode()
    assert call(idx=None, n1=sum(sizes), nb=nb - 1) == WORKSPACE
    # workspace
    assert call(nb=nb - 1) == WORKSPACE and str(nb) in lib.am_last_error().decode()
    assert call(ws=None) == WORKSPACE and call(nb=0) == WORKSPACE
    assert call(rows=FAKE, nb=nb - 1) == WORKSPACE                        # out_rows needs no more workspace


def test_workspace_query(lib):
    q = lib.am_mmd_rbf_groups_workspace_bytes
    for d in (32, 100, 512):
        prev = 0
        for nt in (1, 129, 1000, 2100, 20_000, 100_000, 1_000_000):     # (carve-outs are 256-byte aligned)
            w = q(nt, 1, 100_000, d)
            assert w > prev, (nt, d)
            assert w >= nt * (8 + 4 + 4 + 16) + 100_000 * 8            # norms, offsets, groups, row sums; reference norms
            prev = w
        prev = 0
        for n2 in (2, 129, 1000, 2100, 20_000, 100_000, 1_000_000):
            w = q(100_000, 2000, n2, d)
            assert w > prev, (n2, d)
            prev = w
        by_b = [q(100_000, b, 100_000, d) for b in (1, 10, 1000, 2000, 100_000)]
        assert by_b == sorted(by_b) and by_b[0] < by_b[-1]
    # every tile count up to a few thousand rows, in both directions: no step back at a chunk threshold
    for fixed in (128, 5000, 100_000):
        sizes = [q(nt, 3, fixed, 64) for nt in range(1, 6000, 37)]
        assert sizes == sorted(sizes)
        sizes = [q(fixed, 3, n2, 64) for n2 in range(2, 6000, 37)]
        assert sizes == sorted(sizes)
    assert q(0, 1, 10, 64) == 0 and q(10, 0, 10, 64) == 0 and q(10, 1, 1, 64) == 0 and q(10, 1, 10, 0) == 0
    # 100 000 candidate rows against 100 000 reference rows: per-row partials, not a Gram matrix
    assert q(100_000, 2000, 100_000, 512) < 100 << 20


# ---------------------------------------------------------------------------------------------------- front end
def _host_set(am, rows):
    s = am.AudioMetricsData(True)
    s._embeddings = rows
    return s


def test_validation_happens_before_any_device_call(am, monkeypatch):
    from audio_metrics_amd import hip_ops

    def forbidden(*a, **k):
        raise AssertionError("device call before validation")
    for name in ("pairwise_select_sq", "mmd_rbf_sums", "mmd_rbf_group_sums", "as_matrix"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    ok = _host_set(am, torch.zeros((10, 8)))
    labels = np.arange(10) // 3
    f = am.kernel_audio_distance_per_group
    with pytest.raises(ValueError, match="store"):
        f(am.AudioMetricsData(False), ok, labels)
    with pytest.raises(ValueError, match="store"):
        f(_host_set(am, torch.zeros((0, 8))), ok, [])
    with pytest.raises(ValueError, match="empty"):
        f(ok, ok, [])
    with pytest.raises(ValueError, match="9 labels for 10 stored rows"):
        f(ok, ok, np.arange(9))
    with pytest.raises(ValueError, match="11 labels for 10 stored rows"):
        f(ok, ok, torch.arange(11))
    for bad in (np.zeros(10), torch.zeros(10), np.zeros(10, dtype=bool), ["a"] * 10):
        with pytest.raises(ValueError, match="integer"):
            f(ok, ok, bad)
    with pytest.raises(ValueError, match="store"):
        f(ok, am.AudioMetricsData(False), labels)
    with pytest.raises(ValueError, match="at least 2 rows in the reference"):
        f(ok, _host_set(am, torch.zeros((1, 8))), labels)
    with pytest.raises(NotImplementedError, match="reference set holds float64"):
        f(ok, _host_set(am, torch.zeros((10, 8), dtype=torch.float64)), labels)
    with pytest.raises(NotImplementedError, match="candidate set holds float64"):
        f(_host_set(am, torch.zeros((10, 8), dtype=torch.float64)), ok, labels)
    with pytest.raises(ValueError, match="feature widths differ: 8 and 12"):
        f(ok, _host_set(am, torch.zeros((10, 12))), labels)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="bandwidth"):
            f(ok, ok, labels, bandwidth=bad)
    with pytest.raises(AssertionError, match="device call"):                 # valid arguments do reach the device layer
        f(ok, ok, labels)
    with pytest.raises(AssertionError, match="device call"):                 # a single row per group is legal input
        f(_host_set(am, torch.zeros((1, 8))), ok, [7], bandwidth=2.0)


def test_ops_layer_rejects_float64_rows_and_bad_arguments(am):
    ops = am.hip_ops
    x32, x64 = torch.zeros((4, 8)), torch.zeros((4, 8), dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="float32 rows"):
        ops.mmd_rbf_group_sums(x64, None, [0, 4], x32, gamma=1.0)
    with pytest.raises(NotImplementedError, match="float32 rows"):
        ops.mmd_rbf_group_sums(x32, None, [0, 4], x64, gamma=1.0)
    with pytest.raises(ValueError, match="exactly one"):
        ops.mmd_rbf_group_sums(x32, None, [0, 4], x32)
    with pytest.raises(am._lib.HipLibraryError):                              # no CPU fallback
        ops.mmd_rbf_group_sums(x32, None, [0, 4], x32, gamma=1.0)


def test_combination_step_single_rows_and_nan(am):
    from audio_metrics_amd.metrics import kad
    sizes = np.array([4, 1, 3, 1, 2])
    sxx = np.array([6.0, 0.0, 3.0, 0.0, np.nan])
    sxy = np.array([8.0, 1.5, 4.5, 0.5, np.nan])
    syy, m = 45.0, 10
    with pytest.warns(RuntimeWarning, match="2 of 5 groups hold a single row") as rec:
        scaled, mmd2 = kad.combine_group_sums(sxx, sxy, sizes, syy, m, scale=100.0)
    assert len([r for r in rec if issubclass(r.category, RuntimeWarning)]) == 1           # one warning, not one per group
    assert np.isnan(mmd2[[1, 3, 4]]).all() and np.isfinite(mmd2[[0, 2]]).all()            # the NaN sums stay in their own group
    assert mmd2[0] == 6.0 / 12.0 + 45.0 / 90.0 - 2.0 * 8.0 / 40.0
    assert mmd2[2] == 3.0 / 6.0 + 45.0 / 90.0 - 2.0 * 4.5 / 30.0
    np.testing.assert_array_equal(scaled[[0, 2]], 100.0 * mmd2[[0, 2]])
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                                     # no single-row group: no warning
        scaled, mmd2 = kad.combine_group_sums(sxx[[0, 2]], sxy[[0, 2]], sizes[[0, 2]], syy, m)
    assert np.isfinite(mmd2).all() and (scaled == kad.KAD_SCALE * mmd2).all()
    # agreement with the whole-set combination of kernel_audio_distance for one group
    import kad_reference as ka
    one = kad.combine_group_sums([6.0], [8.0], [4], syy, m, scale=1.0)[1][0]
    assert one == ka.mmd2(ka.device_means([6.0, syy, 8.0], 4, m))


def test_export_and_untouched_tables(am):
    from audio_metrics_amd import audio_metrics as front
    from audio_metrics_amd.metrics import kad
    assert am.kernel_audio_distance_per_group is kad.kernel_audio_distance_per_group
    assert [k for k, _ in front.EVALUATION_TABLE] == ["fad", "fad_inf", "kd", "kad", "prdc", "apa"]
    assert not any("group" in k for k in front.ROW_METRICS)


# ---------------------------------------------------------------------------------------------------- compile-time resources
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_kernels_use_no_scratch_memory():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    import importlib.util
    spec = importlib.util.spec_from_file_location("am_build", os.path.join(ROOT, "audio-metrics_amd", "_build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)                                         # the flags the shipped library is built with
    r = subprocess.run([hipcc, *build.HIPCC_FLAGS, "--cuda-device-only", "-c", "kad_groups.hip", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        for key, short in (("ScratchSize \\[bytes/lane\\]", "scratch"), ("VGPRs", "vgprs"), ("VGPRs Spill", "spill"),
                           ("Occupancy \\[waves/SIMD\\]", "occupancy")):
            m = re.search(r"remark:\s+%s: (\d+)" % key, line)
            if m and name:
                usage[name][short] = int(m.group(1))
    for kernel, count in (("kadg_rows_kernel", 4), ("kadg_prep_kernel", 1), ("kadg_rowsum_kernel", 1), ("kadg_finish_kernel", 1)):
        hits = {n: u for n, u in usage.items() if kernel in n}
        assert len(hits) == count, (kernel, sorted(usage))
        for n, u in hits.items():
            assert u["scratch"] == 0 and u["spill"] == 0, (n, u)
            assert u["vgprs"] <= 256 and u["occupancy"] >= 2, (n, u)       # tile kernels: two workgroups of four waves per CU
    # the names of this file must not be counted among the kernels of kad.hip (tests/test_kad_cpu.py counts by substring)
    for n in usage:
        assert not any(s in n for s in ("kad_select_kernel", "kad_mmd_kernel", "kad_scan_kernel", "kad_norms_kernel", "kad_reduce_kernel")), n
