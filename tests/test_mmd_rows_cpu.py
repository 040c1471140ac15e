"""Two-sided row sums and the KAD error statistics, the part that needs no GPU: the host oracle the GPU tests lean on, the
host formulas of metrics/kad_stats.py against direct loops, their calibration on seeded draws, validation before any device
call, the new names in header / signature table / package, the error paths and workspace query of am_mmd_rbf_rows_f32, and
the compile-time resource check of csrc/mmd_rows.hip (no scratch memory in any instantiation, two workgroups per CU)."""
import ctypes
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

import kd_reference as kr
import mmd_rows_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-metrics_amd", "csrc")
BAD_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -4
FAKE = ctypes.c_void_p(0x10000)                       # 16-byte aligned, never dereferenced: the calls stop at validation
NAMES = ("am_mmd_rbf_rows_workspace_bytes", "am_mmd_rbf_rows_f32")


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
def test_oracle_against_a_direct_double_loop():
    rng = np.random.default_rng(11)
    x, y = kr.rbf_rows(rng, 5, 16, 10.0), kr.rbf_rows(rng, 7, 16, 10.0)
    gamma = 1.0 / 200.0

    def k(a, b):
        return np.exp(-((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum() * gamma)
    w = [sum(k(x[i], x[j]) for j in range(5) if j != i) for i in range(5)]
    c = [sum(k(x[i], y[j]) for j in range(7)) for i in range(5)]
    v = [sum(k(y[j], y[l]) for l in range(7) if l != j) for j in range(7)]
    r = [sum(k(x[i], y[j]) for i in range(5)) for j in range(7)]
    got = mr.row_sums(x, y, gamma)
    for name, want in (("w", w), ("c", c), ("v", v), ("r", r)):
        np.testing.assert_allclose(got[name], want, rtol=1e-13, err_msg=name)
    assert 0.0 < got["scale"] <= 1.0
    # blocks of rows are an implementation detail of the oracle
    big_x, big_y = kr.rbf_rows(rng, 70, 16, 10.0), kr.rbf_rows(rng, 45, 16, 10.0)
    whole = mr.row_sums(big_x, big_y, gamma)
    old, mr.BLOCK = mr.BLOCK, 32
    try:
        cut = mr.row_sums(big_x, big_y, gamma)
    finally:
        mr.BLOCK = old
    for name in ("w", "c", "v", "r"):
        np.testing.assert_allclose(cut[name], whole[name], rtol=1e-14, err_msg=name)
    # y is x: v = w, and c keeps the diagonal that w drops
    same = mr.row_sums(big_x, big_x, gamma, same=True)
    assert np.array_equal(same["v"], same["w"])
    np.testing.assert_allclose(same["c"], same["w"] + 1.0, rtol=1e-14)
    np.testing.assert_allclose(same["r"], same["c"], rtol=1e-14)


# ---------------------------------------------------------------------------------------------------- host formulas
def test_host_formulas_against_direct_loops(am):
    rng = np.random.default_rng(12)
    for n, m in ((5, 7), (40, 23)):
        x, y, b = rng.standard_normal((n, 8)) + 0.5, rng.standard_normal((m, 8)), rng.standard_normal((n + 3, 8)) + 0.7
        s, t = mr.row_sums(x, y, 1.0 / 32.0), mr.row_sums(b, y, 1.0 / 32.0)
        mmd2, se = am.mmd_standard_error(s["w"], s["c"], s["v"], s["r"])
        want_mmd2, want_se = mr.standard_error(s["w"], s["c"], s["v"], s["r"])
        np.testing.assert_allclose([mmd2, se], [want_mmd2, want_se], rtol=1e-13)
        assert se > 0.0
        got = am.mmd_difference_test(s["w"], s["c"], s["r"], t["w"], t["c"], t["r"])
        want = mr.difference_test(s["w"], s["c"], s["r"], t["w"], t["c"], t["r"])
        assert list(got) == ["difference", "std_error", "z", "p_value", "p_value_two_sided"]
        np.testing.assert_allclose(list(got.values()), want, rtol=1e-13)
        assert 0.0 < got["p_value"] < 1.0 and got["p_value_two_sided"] == pytest.approx(2.0 * min(got["p_value"], 1.0 - got["p_value"]), abs=1e-14)
        # A and B swapped: the sign of z flips
        swapped = am.mmd_difference_test(t["w"], t["c"], t["r"], s["w"], s["c"], s["r"])
        assert swapped["z"] == -got["z"] and swapped["p_value"] == pytest.approx(1.0 - got["p_value"], abs=1e-14)
        # lists and float32 arrays are taken as they come
        assert am.mmd_standard_error(list(s["w"]), list(s["c"]), list(s["v"]), list(s["r"])) == (mmd2, se)
    with pytest.raises(ValueError, match="at least 2 rows"):
        am.mmd_standard_error([1.0], [1.0], [1.0, 2.0], [1.0, 2.0])
    with pytest.raises(ValueError, match="one entry per"):
        am.mmd_standard_error([1.0, 2.0], [1.0], [1.0, 2.0], [1.0, 2.0])
    with pytest.raises(ValueError, match="disagree"):
        am.mmd_difference_test([1.0, 2.0], [1.0, 2.0], [1.0, 2.0, 3.0], [1.0, 2.0], [1.0, 2.0], [1.0, 2.0])


def test_identical_candidates_give_nan_and_one_warning(am):
    rng = np.random.default_rng(13)
    x, y = rng.standard_normal((30, 8)) + 0.5, rng.standard_normal((20, 8))
    s = mr.row_sums(x, y, 1.0 / 32.0)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = am.mmd_difference_test(s["w"], s["c"], s["r"], s["w"], s["c"], s["r"])
    assert len(rec) == 1 and issubclass(rec[0].category, RuntimeWarning) and "same rows" in str(rec[0].message)
    assert got["difference"] == 0.0
    assert np.isnan(got["z"]) and np.isnan(got["p_value"]) and np.isnan(got["p_value_two_sided"])
    # a variance of exactly 0 (constant influence values): the same answer
    flat = np.ones(6)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = am.mmd_difference_test(flat, flat, np.ones(4), 2.0 * flat, flat, np.ones(4))
    assert len(rec) == 1 and got["std_error"] == 0.0 and np.isnan(got["z"]) and np.isnan(got["p_value"])
    assert np.isnan(mr.difference_test(flat, flat, np.ones(4), 2.0 * flat, flat, np.ones(4))[2])


# ---------------------------------------------------------------------------------------------------- calibration
DRAWS, DIM = 300, 8
GAMMA = 0.5 / (2 * DIM)


@pytest.mark.parametrize("n, m, shift", [(200, 200, 0.5), (100, 400, 0.5), (300, 150, 1.0)])
def test_standard_error_is_calibrated(am, n, m, shift):
    """mean estimated se / empirical sd of mmd^2 over 300 seeded draws of two DIFFERENT distributions lies in [0.85, 1.15]
    (measured when the estimator was chosen: 0.994, 0.940, 0.953)."""
    rng = np.random.default_rng(1)
    res = []
    for _ in range(DRAWS):
        x = rng.standard_normal((n, DIM)) + shift
        y = rng.standard_normal((m, DIM))
        s = mr.row_sums(x, y, GAMMA)
        res.append(am.mmd_standard_error(s["w"], s["c"], s["v"], s["r"]))
    res = np.array(res)
    ratio = res[:, 1].mean() / res[:, 0].std(ddof=1)
    print(f"({n}, {m}, {shift}): mean se {res[:, 1].mean():.6e} empirical sd {res[:, 0].std(ddof=1):.6e} ratio {ratio:.3f}")
    assert 0.85 <= ratio <= 1.15, ratio


@pytest.mark.parametrize("na, nb, m, shift_a, shift_b", [(200, 200, 300, 0.5, 0.5), (120, 260, 200, 0.5, 0.5), (200, 200, 300, 0.4, 0.6)])
def test_difference_test_is_calibrated(am, na, nb, m, shift_a, shift_b):
    """mean estimated se / empirical sd of the difference in [0.85, 1.15] (measured: 1.058, 0.950, 1.085); with equal shifts z
    has sd in [0.85, 1.15]; with shifts (0.4, 0.6) every draw rejects one-sided at 5 %."""
    rng = np.random.default_rng(2)
    res = []
    for _ in range(DRAWS):
        a = rng.standard_normal((na, DIM)) + shift_a
        b = rng.standard_normal((nb, DIM)) + shift_b
        ref = rng.standard_normal((m, DIM))
        s, t = mr.row_sums(a, ref[:2], GAMMA), mr.row_sums(b, ref[:2], GAMMA)          # w alone: the reference block is not needed
        ca, cb = mr._kernel(a, ref, GAMMA, None), mr._kernel(b, ref, GAMMA, None)
        got = am.mmd_difference_test(s["w"], ca.sum(1), ca.sum(0), t["w"], cb.sum(1), cb.sum(0))
        res.append((got["difference"], got["std_error"], got["z"]))
    res = np.array(res)
    ratio = res[:, 1].mean() / res[:, 0].std(ddof=1)
    print(f"({na}, {nb}, {m}, {shift_a}, {shift_b}): ratio {ratio:.3f} z mean {res[:, 2].mean():.3f} z sd {res[:, 2].std(ddof=1):.3f} "
          f"z max {res[:, 2].max():.3f}")
    assert 0.85 <= ratio <= 1.15, ratio
    if shift_a == shift_b:
        assert 0.85 <= res[:, 2].std(ddof=1) <= 1.15, res[:, 2].std(ddof=1)
    else:
        assert (res[:, 2] < -1.645).all(), res[:, 2].max()


# ---------------------------------------------------------------------------------------------------- validation
def test_validation_happens_before_any_device_call(am, monkeypatch):
    from audio_metrics_amd import hip_ops

    def forbidden(*a, **k):
        raise AssertionError("device call before validation")
    for name in ("as_matrix", "_call", "_workspace"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    x, y = torch.zeros((10, 8)), torch.zeros((12, 8))

    def sums(a=x, b=y, **kw):
        kw.setdefault("gamma", 0.5)
        return hip_ops.mmd_rbf_row_sums(a, b, **kw)
    for kw in (dict(a=x.double()), dict(b=y.double()), dict(a=x.double(), b=y.double())):
        with pytest.raises(NotImplementedError, match="float32 rows"):
            sums(**kw)
    with pytest.raises(ValueError, match="feature widths"):
        sums(b=torch.zeros((12, 12)))
    with pytest.raises(ValueError, match="2-D"):
        sums(a=torch.zeros(8))
    for bad in (0, 8, -1):
        with pytest.raises(ValueError, match="blocks"):
            sums(blocks=bad)
    with pytest.raises(ValueError, match="exactly one of"):
        sums(gamma=None)
    with pytest.raises(ValueError, match="exactly one of"):
        sums(gamma=0.5, bw2=torch.zeros(()))
    # the front ends: with the operations they are built from forbidden too
    for name in ("mmd_rbf_row_sums", "pairwise_select_sq", "mmd_rbf_sums"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    ok, ref = host_set(am, x), host_set(am, y)
    wide, one, none = host_set(am, torch.zeros((12, 12))), host_set(am, torch.zeros((1, 8))), am.AudioMetricsData(False)
    calls = [lambda s, r: am.kernel_audio_distance_with_error(s, r), lambda s, r: am.kernel_audio_distance_compare(s, ok, r),
             lambda s, r: am.kernel_audio_distance_compare(ok, s, r)]
    for call in calls:
        with pytest.raises(NotImplementedError, match="float64"):
            call(host_set(am, x.double()), ref)
        with pytest.raises(NotImplementedError, match="float64"):
            call(ok, host_set(am, y.double()))
        with pytest.raises(NotImplementedError, match="float64"):
            call(host_set(am, x.double()), host_set(am, y.double()))
        with pytest.raises(ValueError, match="feature widths"):
            call(ok, wide)
        with pytest.raises(ValueError, match="feature widths"):
            call(wide, ref)
        with pytest.raises(ValueError, match="at least 2 rows in the candidate"):
            call(one, ref)
        with pytest.raises(ValueError, match="at least 2 rows in the reference"):
            call(ok, one)
        with pytest.raises(ValueError, match="keeps none"):
            call(none, ref)
        with pytest.raises(ValueError, match="keeps none"):
            call(ok, none)
        for bad in (0.0, -2.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="bandwidth"):
                am.kernel_audio_distance_with_error(ok, ref, bandwidth=bad)
            with pytest.raises(ValueError, match="bandwidth"):
                am.kernel_audio_distance_compare(ok, ok, ref, bandwidth=bad)
    for bad in (0.0, 1.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="confidence"):
            am.kernel_audio_distance_with_error(ok, ref, confidence=bad)


# ---------------------------------------------------------------------------------------------------- names
def test_header_signature_table_and_package_agree(am, lib):
    with open(os.path.join(ROOT, "include", "audio_metrics_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in am._lib.SIGNATURES and hasattr(lib, name), name
    assert len(am._lib.SIGNATURES["am_mmd_rbf_rows_f32"][1]) == 15
    assert len(am._lib.SIGNATURES["am_mmd_rbf_rows_workspace_bytes"][1]) == 4
    from audio_metrics_amd.metrics import kad, kad_stats
    assert am.metrics.kad_stats is kad_stats
    for name in ("mmd_standard_error", "mmd_difference_test", "kernel_audio_distance_with_error", "kernel_audio_distance_compare"):
        assert getattr(am, name) is getattr(kad_stats, name), name
    assert callable(am.hip_ops.mmd_rbf_row_sums)
    assert kad._ReferenceCache((0, 0)).vrow == {}
    from audio_metrics_amd import audio_metrics as front                   # neither becomes a metric name of AudioMetrics
    assert not any("error" in k or "compare" in k for k, _ in front.EVALUATION_TABLE)


# ---------------------------------------------------------------------------------------------------- entry point
def test_error_paths(lib):
    n1, n2, d = 1000, 300, 64
    nb = lib.am_mmd_rbf_rows_workspace_bytes(n1, n2, d, 7)
    assert nb > 0

    def call(x=FAKE, n1=n1, ldx=d, y=FAKE, n2=n2, ldy=d, d=d, bw2_dev=None, gamma=0.5, blocks=7, out_x=FAKE, out_y=FAKE, ws=FAKE, nb=nb):
        return lib.am_mmd_rbf_rows_f32(x, n1, ldx, y, n2, ldy, d, bw2_dev, gamma, blocks, out_x, out_y, ws, nb, None)
    assert call(x=None) == BAD_ARG and call(y=None) == BAD_ARG
    assert "null" in lib.am_last_error().decode()
    assert call(blocks=0) == BAD_ARG and call(blocks=8) == BAD_ARG and "AM_MMD_XX" in lib.am_last_error().decode()
    # an output may be missing only if no named block writes through it
    for blocks in (1, 4, 5, 7):
        assert call(blocks=blocks, out_x=None) == BAD_ARG and "out_x" in lib.am_last_error().decode(), blocks
    for blocks in (2, 4, 6, 7):
        assert call(blocks=blocks, out_y=None) == BAD_ARG and "out_y" in lib.am_last_error().decode(), blocks
    assert call(blocks=2, out_x=None, nb=0) == WORKSPACE and call(blocks=1, out_y=None, nb=0) == WORKSPACE
    assert call(n1=0) == BAD_SHAPE and call(n2=0) == BAD_SHAPE and call(d=0) == BAD_SHAPE
    assert call(ldx=d - 4) == BAD_ARG and call(ldy=d + 2) == BAD_ARG and "ld" in lib.am_last_error().decode()
    assert call(x=ctypes.c_void_p(0x10004)) == BAD_ARG and call(y=ctypes.c_void_p(0x10008)) == BAD_ARG
    big = 1 << 24
    assert call(n1=big, nb=1 << 40) == BAD_SHAPE and "4 GiB" in lib.am_last_error().decode()
    assert call(n2=big, nb=1 << 40) == BAD_SHAPE
    assert call(gamma=-1.0) == BAD_ARG and call(gamma=float("nan")) == BAD_ARG and "gamma" in lib.am_last_error().decode()
    assert call(gamma=-1.0, bw2_dev=FAKE, nb=nb - 1) == WORKSPACE           # a device bandwidth replaces the host one
    assert call(nb=nb - 1) == WORKSPACE and str(nb) in lib.am_last_error().decode()
    assert call(ws=None) == WORKSPACE and call(nb=0) == WORKSPACE
    # a mask needs the workspace of its own blocks only; a single row in either set is a valid shape
    assert call(blocks=5, nb=lib.am_mmd_rbf_rows_workspace_bytes(n1, n2, d, 5) - 1) == WORKSPACE
    assert call(n1=1, nb=0) == WORKSPACE and call(n2=1, nb=0) == WORKSPACE


def test_workspace_query(lib):
    q = lib.am_mmd_rbf_rows_workspace_bytes
    for bad in ((0, 10, 64, 7), (10, 0, 64, 7), (10, 10, 0, 7), (10, 10, 64, 0), (10, 10, 64, 8)):
        assert q(*bad) == 0, bad
    # 100 000 x 100 000 x 512: positive and below 256 MiB - the Q-side partials are bounded by the band of P tiles, not by
    # (P tiles) x N doubles (625 MB here)
    full = q(100_000, 100_000, 512, 7)
    assert 0 < full < 256 << 20, full
    # linear in the rows once the band is full: ten times the rows, about ten times the bytes
    assert q(1_000_000, 1_000_000, 64, 7) < 11 * full
    # the width does not matter, a smaller mask never needs more, and XX | XY against a small candidate set is small
    assert q(100_000, 100_000, 128, 7) == full
    for blocks in range(1, 8):
        assert 0 < q(20_000, 5_000, 64, blocks) <= q(20_000, 5_000, 64, 7), blocks
    assert q(1_000, 100_000, 512, 5) < 32 << 20


# ---------------------------------------------------------------------------------------------------- the kernels' resources
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_no_instantiation_uses_scratch_memory():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    import importlib.util
    spec = importlib.util.spec_from_file_location("am_build", os.path.join(ROOT, "audio-metrics_amd", "_build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)                                         # the flags the shipped library is built with
    r = subprocess.run([hipcc, *build.HIPCC_FLAGS, "--cuda-device-only", "-c", "mmd_rows.hip", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, timeout=600)
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
    with open(os.path.join(CSRC, "mmd_rows.hip")) as f:
        declared = set(re.findall(r"\b(mmd_rows\w*_kernel)\(", f.read()))
    assert declared == {"mmd_rows_kernel", "mmd_rows_fold_p_kernel", "mmd_rows_fold_q_kernel", "mmd_rows_write_kernel"}, declared
    tile = {n: u for n, u in usage.items() if "mmd_rows_kernel" in n}
    # the tile kernel: symmetric / cross, each without / with the inner-dimension tail
    want = {"ILb%dELb%dE" % (sym, tail) for sym in (0, 1) for tail in (0, 1)}
    assert len(tile) == len(want) == 4, sorted(tile)
    for tag in want:
        assert sum(tag in n for n in tile) == 1, (tag, sorted(tile))
    assert len(usage) == 7 and all(any(k in n for n in usage) for k in declared), sorted(usage)      # every __global__ kernel of the file
    for n, u in usage.items():
        print(n, u)
        assert u["scratch"] == 0, (n, u)
        assert u["vgprs"] <= 256 and u["occupancy"] >= 2, (n, u)           # two workgroups of four waves per CU
