"""Distance correlation and HSIC / CKA of paired sets, the part that needs no GPU: the host arithmetic of metrics/dependence.py
against the explicitly U-centred oracle (tests/dependence_reference.py), the properties of the statistics, the calibration of
the t-test and of the song-level permutation null, the bookkeeping of a re-pairing, validation before any device call, the
names in header / signature table / package, the error paths of am_pair_dependence_f32, and the compile-time resource check
of csrc/pair_dependence.hip (no scratch memory, two workgroups per CU).

The front ends run here on host tensors with hip_ops.pair_dependence replaced by the oracle's row sums (oracle_op)."""
import ctypes
import math
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

import dependence_reference as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-metrics_amd", "csrc")
BAD_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -4
FAKE = ctypes.c_void_p(0x10000)                       # 16-byte aligned, never dereferenced: the calls stop at validation
NAMES = ("am_pair_dependence_workspace_bytes", "am_pair_dependence_f32")
BAND = (0.012, 0.088)                                 # 0.05 +- 3 sqrt(0.05 0.95 / 300): the three-sigma band of 300 draws


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    return audio_metrics_amd


@pytest.fixture(scope="module")
def dep(am):
    from audio_metrics_amd.metrics import dependence
    return dependence


@pytest.fixture(scope="module")
def lib(am):
    return am._lib.load()


def host_sums(dep, x, y, kind="energy", bw2x=None, bw2y=None):
    """(a, b, [n, 5] row sums) of the oracle"""
    a, b = dr.pair_matrix(x, kind, bw2x), dr.pair_matrix(y, kind, bw2y)
    return a, b, dr.row_sums(a, b)


def host_dcor(dep, x, y):
    st = dep.dependence_from_sums(host_sums(dep, x, y)[2], len(x))
    return st["u_ab"] / np.sqrt(st["u_aa"] * st["u_bb"]), st


def oracle_op(calls=None):
    """hip_ops.pair_dependence on host tensors, from the oracle"""
    def op(x, y, kernel, bw2x=None, bw2y=None, perm=None):
        xs, ys = x.numpy(), y.numpy()
        if perm is not None:
            ys = ys[perm.numpy()]
        bw = [float(b) if b is not None else None for b in (bw2x, bw2y)]
        rows = dr.row_sums(dr.pair_matrix(xs, kernel, bw[0]), dr.pair_matrix(ys, kernel, bw[1]))
        bad = ~(np.isfinite(xs).all(1) & np.isfinite(ys).all(1))
        if bad.any():
            rows[:] = np.nan
        sums = np.array([*rows.sum(0), rows[:, 0] @ rows[:, 1], (~bad).sum(), bad.sum()])
        if calls is not None:
            calls.append(perm)
        return torch.as_tensor(rows), torch.as_tensor(sums)
    return op


# ---------------------------------------------------------------------------------------------------- the formulas
@pytest.mark.parametrize("n", [4, 5, 33])
@pytest.mark.parametrize("kind", dr.KINDS)
def test_row_sum_identity_equals_explicit_u_centring(dep, n, kind):
    rng = np.random.default_rng(100 * n + len(kind))
    x = rng.standard_normal((n, 6)).astype(np.float32)
    y = (0.7 * x[:, :3] + rng.standard_normal((n, 3))).astype(np.float32)
    a, b, rows = host_sums(dep, x, y, kind, 12.0, 6.0)
    want = dr.statistics(a, b)
    for got in (dep.dependence_from_sums(rows, n), dep.dependence_from_sums(dr.totals(rows), n)):
        for key, terms in (("u_ab", (a * b)), ("u_aa", a * a), ("u_bb", b * b), ("v_ab", a * b), ("v_aa", a * a), ("v_bb", b * b)):
            size = np.abs(terms).sum() / (n * (n - 3.0) if key[0] == "u" else n * n)      # the size of the terms the statistic is a difference of
            print(f"n={n} {kind} {key}: {got[key]!r} oracle {want[key]!r} terms {size:.3e}")
            assert abs(got[key] - want[key]) <= 1e-12 * size, (n, kind, key, got[key], want[key], size)
    six = dep.dependence_from_sums(dr.totals(rows)[:6], n)                    # the device totals alone: no variances
    assert six["u_ab"] == dep.dependence_from_sums(dr.totals(rows), n)["u_ab"] and np.isnan(six["u_aa"]) and np.isnan(six["u_bb"])
    shares = dep.row_dependence(rows)
    assert shares.shape == (n,) and abs(shares.mean() - want["u_ab"]) <= 1e-12 * np.abs(a * b).sum() / (n * (n - 3.0))


def test_dependence_from_sums_rejects_bad_input(dep):
    with pytest.raises(ValueError, match="at least 4"):
        dep.dependence_from_sums(np.zeros((3, 5)), 3)
    with pytest.raises(ValueError, match="shape"):
        dep.dependence_from_sums(np.zeros((6, 5)), 5)
    with pytest.raises(ValueError, match="6 or 8"):
        dep.dependence_from_sums(np.zeros(7), 5)


def test_properties_of_the_distance_correlation(dep):
    rng = np.random.default_rng(7)
    n = 40
    x = rng.standard_normal((n, 5)).astype(np.float64)
    # dcor_v lies in [0, 1] and is 1 for y = 2 x + c; so is the bias-corrected one there
    _, _, rows = host_sums(dep, x, 2.0 * x + 3.0)
    st = dep.dependence_from_sums(rows, n)
    assert abs(st["v_ab"] / np.sqrt(st["v_aa"] * st["v_bb"]) - 1.0) <= 1e-12
    assert abs(st["u_ab"] / np.sqrt(st["u_aa"] * st["u_bb"]) - 1.0) <= 1e-12
    y = (0.5 * x[:, :2] + rng.standard_normal((n, 2)))
    for trial in range(5):
        z = rng.standard_normal((n, 3))
        s = dep.dependence_from_sums(host_sums(dep, x, z)[2], n)
        v = s["v_ab"] / np.sqrt(s["v_aa"] * s["v_bb"])
        assert 0.0 <= v <= 1.0, (trial, v)
    # invariant under rotation and translation of either side
    base, _ = host_dcor(dep, x, y)
    qx, _ = np.linalg.qr(rng.standard_normal((5, 5)))
    qy, _ = np.linalg.qr(rng.standard_normal((2, 2)))
    moved, _ = host_dcor(dep, x @ qx + 4.0, y @ qy - 2.5)
    assert abs(moved - base) <= 1e-11, (moved, base)
    assert 0.05 < base < 1.0


def test_t_test_figures(dep):
    from scipy import stats
    n = 64
    v = n * (n - 3) / 2.0
    t, dof, p = dep.dcor_t_test(0.1, n)
    assert dof == v - 1 and abs(t - np.sqrt(v - 1) * 0.1 / np.sqrt(1 - 0.01)) <= 1e-14 * t
    assert abs(p - stats.t.sf(t, dof)) <= 1e-15 and p < 0.05
    t0, _, p0 = dep.dcor_t_test(-0.01, n)
    assert t0 < 0 and p0 > 0.5                                           # one-sided: a negative value is no evidence
    # above 1e6 degrees of freedom the normal tail, continuous with Student's t there
    big = 2000
    tb, dofb, pb = dep.dcor_t_test(0.001, big)
    assert dofb > 1e6 and abs(pb - stats.t.sf(tb, dofb)) <= 1e-6 * pb
    assert abs(pb - 0.5 * math.erfc(tb / math.sqrt(2.0))) <= 1e-15
    assert dep.dcor_t_test(1.0, n)[2] == 0.0 and np.isnan(dep.dcor_t_test(float("nan"), n)[2])


# ---------------------------------------------------------------------------------------------------- calibration
def test_t_test_is_calibrated_on_independent_pairs(dep):
    """d = 4, 300 seeded draws of 64 iid pairs under independence: the 5 % test rejects inside the three-sigma band.
    Measured: 6.0 %."""
    rng = np.random.default_rng(2024)
    rejected = 0
    for _ in range(300):
        x, y = rng.standard_normal((64, 4)), rng.standard_normal((64, 4))
        dcor, _ = host_dcor(dep, x, y)
        rejected += dep.dcor_t_test(dcor, 64)[2] <= 0.05
    rate = rejected / 300.0
    print(f"independent pairs: the t-test rejects at 5 % in {rate:.3f} of 300 draws")
    assert BAND[0] <= rate <= BAND[1], rate


def test_windows_of_songs_need_the_song_level_null(dep):
    """16 songs x 8 windows, window spread 0.3 of the song spread, X and Y independent ACROSS songs: windows of one song are
    near-duplicates, the row-level t-test takes them for 128 independent pairs and rejects far above its level; the
    song-level permutation null (199 labellings) stays inside the band.  Measured: 100 % and 5.0 % (README)."""
    rng = np.random.default_rng(77)
    songs, windows, P = 16, 8, 199
    n = songs * windows
    groups = np.repeat(np.arange(songs), windows)
    t_rejected = perm_rejected = 0
    for draw in range(300):
        x = rng.standard_normal((songs, 4))[groups] + 0.3 * rng.standard_normal((n, 4))
        y = rng.standard_normal((songs, 4))[groups] + 0.3 * rng.standard_normal((n, 4))
        a, b, rows = host_sums(dep, x, y)
        st = dep.dependence_from_sums(rows, n)
        dcor = st["u_ab"] / np.sqrt(st["u_aa"] * st["u_bb"])
        t_rejected += dep.dcor_t_test(dcor, n)[2] <= 0.05
        perms, movable, fixed = dep.dependence_permutations(n, groups, P, seed=draw)
        assert movable == songs and fixed == 0
        s_ab = np.einsum("ij,pij->p", a, b[perms[:, :, None], perms[:, None, :]])
        c_ab = rows[:, 1][perms] @ rows[:, 0]
        null = dep._u(s_ab, c_ab, rows[:, 0].sum(), rows[:, 1].sum(), float(n))
        perm_rejected += (1.0 + np.count_nonzero(~(null < st["u_ab"]))) / (1.0 + P) <= 0.05
    t_rate, perm_rate = t_rejected / 300.0, perm_rejected / 300.0
    print(f"windows of songs: row-level t-test rejects in {t_rate:.3f}, song-level permutation null in {perm_rate:.3f} of 300 draws")
    assert t_rate > 0.5, t_rate
    assert BAND[0] <= perm_rate <= BAND[1], perm_rate


# ---------------------------------------------------------------------------------------------------- re-pairings
def test_permutations_move_whole_songs_inside_size_classes(dep):
    sizes = [3, 5, 3, 2, 5, 3, 7]                                         # classes: 3 x 3 rows, 2 x 5 rows; 2 and 7 are alone
    labels = np.repeat([40, 10, 30, 20, 50, 60, 70], sizes)
    order = np.random.default_rng(3).permutation(len(labels))             # stored order is not song order
    labels = labels[order]
    n = len(labels)
    perms, movable, fixed = dep.dependence_permutations(n, labels, 50, seed=5)
    assert perms.shape == (50, n) and perms.dtype == np.int64 and movable == 5 and fixed == 2
    again, _, _ = dep.dependence_permutations(n, labels, 50, seed=5)
    assert (perms == again).all() and not (perms == dep.dependence_permutations(n, labels, 50, seed=6)[0]).all()
    rows_of = {s: np.nonzero(labels == s)[0] for s in np.unique(labels)}
    moved = 0
    for p in perms:
        assert sorted(p) == list(range(n))
        for s, rows in rows_of.items():
            src = labels[p[rows]]
            assert len(set(src)) == 1, "a song takes the y block of ONE song"
            t = src[0]
            assert len(rows_of[t]) == len(rows) and (p[rows] == rows_of[t]).all(), "same row count, window order kept"
            if len(rows) in (2, 7):
                assert t == s, "a song alone in its class stays fixed"
            moved += t != s
    assert moved > 0
    free, movable, fixed = dep.dependence_permutations(9, None, 4, seed=1)
    rng = np.random.default_rng(1)
    assert movable == 9 and fixed == 0 and all((free[k] == rng.permutation(9)).all() for k in range(4))
    assert dep.dependence_permutations(9, None, 0)[0].shape == (0, 9)


def test_a_repairing_changes_s_ab_and_c_ab_only(dep):
    """C_ab(pi) from the OBSERVED row sums equals a recomputation on the re-paired set, and so does the statistic."""
    rng = np.random.default_rng(11)
    n = 48
    groups = np.repeat(np.arange(8), 6)
    x = rng.standard_normal((n, 5))
    y = 0.5 * x[:, :3] + rng.standard_normal((n, 3))
    a, b, rows = host_sums(dep, x, y)
    for labels in (None, groups):
        perms, _, _ = dep.dependence_permutations(n, labels, 6, seed=2)
        for p in perms:
            _, bp, rows_p = host_sums(dep, x, y[p])
            assert np.abs(bp - b[np.ix_(p, p)]).max() == 0.0
            c_host = rows[:, 0] @ rows[:, 1][p]
            assert abs(c_host - rows_p[:, 0] @ rows_p[:, 1]) <= 1e-13 * abs(c_host)
            u_host = dep._u(rows_p[:, 2].sum(), c_host, rows[:, 0].sum(), rows[:, 1].sum(), float(n))
            want = dr.u_statistic(a, bp)
            assert abs(u_host - want) <= 1e-12 * np.abs(a * bp).sum() / (n * (n - 3.0))
            np.testing.assert_allclose(rows_p[:, [1, 4]], rows[p][:, [1, 4]], rtol=1e-13)     # B and BB move with their rows


# ---------------------------------------------------------------------------------------------------- front ends on the oracle
def test_front_ends_on_the_oracle(am, dep, monkeypatch):
    calls = []
    monkeypatch.setattr(dep.ops, "pair_dependence", oracle_op(calls))
    rng = np.random.default_rng(21)
    n = 60
    groups = np.repeat(np.arange(10), 6)
    x = rng.standard_normal((n, 6)).astype(np.float32)
    y = (0.6 * x[:, :4] + rng.standard_normal((n, 4))).astype(np.float32)
    xt, yt = torch.as_tensor(x), torch.as_tensor(y)
    got = am.distance_correlation(xt, yt, groups=groups, n_permutations=19, seed=3, return_rows=True)
    a, b, rows = host_sums(dep, x, y)
    want = dr.statistics(a, b)
    assert list(got)[:10] == ["dcov2", "dvar_x", "dvar_y", "dcor", "dcor_v", "dcor_t", "dcor_dof", "dcor_p_value", "dcor_rows",
                              "dcor_rows_nonfinite"]
    for key, w in (("dcov2", want["u_ab"]), ("dvar_x", want["u_aa"]), ("dvar_y", want["u_bb"])):
        assert abs(got[key] - w) <= 1e-12 * abs(w)
    assert abs(got["dcor"] - want["u_ab"] / np.sqrt(want["u_aa"] * want["u_bb"])) <= 1e-12
    assert abs(got["dcor_v"] - want["v_ab"] / np.sqrt(want["v_aa"] * want["v_bb"])) <= 1e-12 and 0.0 <= got["dcor_v"] <= 1.0
    assert (got["dcor_t"], got["dcor_dof"], got["dcor_p_value"]) == dep.dcor_t_test(got["dcor"], n) and got["dcor_p_value"] < 1e-3
    assert got["dcor_rows"] == n and got["dcor_rows_nonfinite"] == 0
    assert abs(got["row_dependence"].mean() - got["dcov2"]) <= 1e-12 * abs(got["dcov2"]) and got["row_sums"].shape == (n, 5)
    # the null: one sweep per labelling with the labellings of dependence_permutations, recomputed here
    perms, movable, fixed = dep.dependence_permutations(n, groups, 19, seed=3)
    assert len(calls) == 20 and calls[0] is None and all((c.numpy() == p).all() for c, p in zip(calls[1:], perms))
    null = np.array([dr.u_statistic(a, b[np.ix_(p, p)]) for p in perms])
    assert got["dcor_p_value_permutation"] == (1.0 + np.count_nonzero(null >= got["dcov2"])) / 20.0 == 0.05
    assert abs(got["dcor_null_mean"] - null.mean()) <= 1e-12 and abs(got["dcor_null_std"] - null.std(ddof=1)) <= 1e-12
    assert abs(got["dcor_null_q95"] - np.quantile(null, 0.95)) <= 1e-12
    assert (got["dcor_n_permutations"], got["units_movable"], got["units_fixed"]) == (19, 10, 0)
    # HSIC / CKA with fixed bandwidths
    for kernel in ("gaussian", "laplacian"):
        k = am.kernel_alignment(xt, yt, kernel=kernel, bandwidth_x=3.0, bandwidth_y=2.0, n_permutations=5, seed=1)
        a, b, _ = host_sums(dep, x, y, kernel, 9.0, 4.0)
        w = dr.statistics(a, b)
        assert abs(k["hsic"] - w["u_ab"]) <= 1e-12 * abs(w["u_ab"]) and abs(k["cka"] - w["u_ab"] / np.sqrt(w["u_aa"] * w["u_bb"])) <= 1e-12
        assert (k["hsic_bandwidth_x"], k["hsic_bandwidth_y"], k["hsic_kernel"], k["hsic_rows_nonfinite"]) == (3.0, 2.0, kernel, 0)
        assert k["units_movable"] == n and 0.0 < k["hsic_p_value_permutation"] <= 1.0 and "hsic_null_q95" in k


def test_degenerate_inputs_give_nan_and_one_warning(am, dep, monkeypatch):
    monkeypatch.setattr(dep.ops, "pair_dependence", oracle_op())
    rng = np.random.default_rng(31)
    x, y = torch.as_tensor(rng.standard_normal((12, 3)).astype(np.float32)), torch.as_tensor(rng.standard_normal((12, 2)).astype(np.float32))

    def one_warning(fn, match):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = fn()
        assert len(w) == 1 and issubclass(w[0].category, RuntimeWarning) and match in str(w[0].message), [str(i.message) for i in w]
        return out
    # the same object twice
    out = one_warning(lambda: am.distance_correlation(x, x), "same object")
    assert np.isnan(out["dcor"]) and np.isnan(out["dcor_p_value"]) and np.isnan(out["dcor_t"]) and out["dcov2"] > 0
    assert np.isnan(one_warning(lambda: am.kernel_alignment(x, x, bandwidth_x=1.0, bandwidth_y=1.0), "same object")["cka"])
    # a variance of 0: every row of y equal
    out = one_warning(lambda: am.distance_correlation(x, torch.ones((12, 2))), "not positive")
    assert np.isnan(out["dcor"]) and np.isnan(out["dcor_v"]) and out["dvar_y"] == 0.0
    # non-finite rows: every figure NaN, the count returned
    bad = y.clone()
    bad[[2, 7], 0] = float("nan")
    out = one_warning(lambda: am.distance_correlation(x, bad, n_permutations=3, return_rows=True), "2 of 12")
    assert out["dcor_rows_nonfinite"] == 2 and all(np.isnan(out[k]) for k in ("dcov2", "dcor", "dcor_v", "dcor_p_value", "dcor_p_value_permutation"))
    assert np.isnan(out["row_dependence"]).all()
    out = one_warning(lambda: am.kernel_alignment(x, bad, bandwidth_x=1.0, bandwidth_y=1.0), "2 of 12")
    assert out["hsic_rows_nonfinite"] == 2 and np.isnan(out["hsic"]) and np.isnan(out["cka"])
    # fewer than two movable units: every song alone in its class
    out = one_warning(lambda: am.distance_correlation(x, y, groups=np.repeat([0, 1, 2], [3, 4, 5]), n_permutations=9), "movable")
    assert np.isnan(out["dcor_p_value_permutation"]) and out["units_movable"] == 0 and out["units_fixed"] == 3 and np.isfinite(out["dcor"])


# ---------------------------------------------------------------------------------------------------- validation
def test_validation_happens_before_any_device_call(am, dep, monkeypatch):
    from audio_metrics_amd import hip_ops

    def forbidden(*a, **k):
        raise AssertionError("device call before validation")
    for name in ("as_matrix", "_call", "_workspace"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    x, y = torch.zeros((10, 8)), torch.zeros((10, 6))

    def op(a=x, b=y, kernel="energy", **kw):
        return hip_ops.pair_dependence(a, b, kernel, **kw)
    for a, b in ((x.double(), y), (x, y.double()), (x.double(), y.double())):
        with pytest.raises(NotImplementedError, match="float32 rows"):
            op(a=a, b=b)
    with pytest.raises(ValueError, match="2-D"):
        op(a=torch.zeros(8))
    with pytest.raises(ValueError, match="row counts differ"):
        op(b=torch.zeros((11, 6)))
    with pytest.raises(ValueError, match="at least 4"):
        op(a=torch.zeros((3, 8)), b=torch.zeros((3, 6)))
    with pytest.raises(ValueError, match="feature widths"):
        op(b=torch.zeros((10, 0)))
    for bad in ("rbf", "Energy", None, 2):
        with pytest.raises(ValueError, match="kernel="):
            op(kernel=bad)
    for kernel in ("gaussian", "laplacian"):
        with pytest.raises(ValueError, match="needs bw2x"):
            op(kernel=kernel, bw2y=1.0)
        with pytest.raises(ValueError, match="needs bw2y"):
            op(kernel=kernel, bw2x=1.0)
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="bw2x"):
                op(kernel=kernel, bw2x=bad, bw2y=1.0)
            with pytest.raises(ValueError, match="bw2y"):
                op(kernel=kernel, bw2x=1.0, bw2y=bad)
    for bad in (torch.zeros(9, dtype=torch.int64), torch.zeros(10, dtype=torch.int32), torch.zeros((10, 1), dtype=torch.int64), [0] * 10):
        with pytest.raises(ValueError, match="perm"):
            op(perm=bad)
    # the front ends: with the operations they are built from forbidden too
    for name in ("pair_dependence", "pairwise_select_sq"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    s = am.AudioMetricsData(True)
    s._embeddings = x
    for call in (am.distance_correlation, am.kernel_alignment):
        for a, b in ((x.double(), y), (x, y.double())):
            with pytest.raises(NotImplementedError, match="float32 rows"):
                call(a, b)
        with pytest.raises(ValueError, match="paired row by row"):
            call(x, torch.zeros((11, 6)))
        with pytest.raises(ValueError, match="at least 4"):
            call(torch.zeros((3, 8)), torch.zeros((3, 6)))
        with pytest.raises(ValueError, match="keeps none"):
            call(am.AudioMetricsData(False), y)
        with pytest.raises(ValueError, match="keeps none"):
            call(s, am.AudioMetricsData(False))
        with pytest.raises(ValueError, match="n_permutations"):
            call(x, y, n_permutations=-1)
        with pytest.raises(ValueError, match="one label per pair"):
            call(x, y, groups=np.arange(9))
        with pytest.raises(ValueError, match="integer labels"):
            call(x, y, groups=np.linspace(0.0, 1.0, 10))
    with pytest.raises(ValueError, match="kernel="):
        am.kernel_alignment(x, y, kernel="energy")
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="bandwidth_x"):
            am.kernel_alignment(x, y, bandwidth_x=bad, bandwidth_y=1.0)
        with pytest.raises(ValueError, match="bandwidth_y"):
            am.kernel_alignment(x, y, bandwidth_x=1.0, bandwidth_y=bad)


# ---------------------------------------------------------------------------------------------------- names
def test_header_signature_table_and_package_agree(am, dep, lib):
    with open(os.path.join(ROOT, "include", "audio_metrics_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in am._lib.SIGNATURES and hasattr(lib, name), name
    assert len(am._lib.SIGNATURES["am_pair_dependence_f32"][1]) == 18
    for name in ("distance_correlation", "kernel_alignment", "dependence_from_sums", "dependence_permutations", "row_dependence",
                 "dcor_t_test"):
        assert getattr(am, name) is getattr(dep, name), name
    assert am.metrics.dependence is dep and callable(am.hip_ops.pair_dependence)
    from audio_metrics_amd import audio_metrics as front                   # not a metric name of AudioMetrics
    assert not any("dcor" in k or "hsic" in k or "cka" in k or "dependence" in k for k, _ in front.EVALUATION_TABLE)


# ---------------------------------------------------------------------------------------------------- entry point
def test_error_paths(lib):
    n, dx, dy = 1000, 64, 36
    nb = lib.am_pair_dependence_workspace_bytes(n, dx, dy)
    assert nb > 0

    def call(x=FAKE, n=n, ldx=dx, dx=dx, y=FAKE, ldy=dy, dy=dy, perm=None, kernel=0, bwx_dev=None, bwx=1.5, bwy_dev=None, bwy=2.5,
             rows=FAKE, sums=FAKE, ws=FAKE, nb=nb):
        return lib.am_pair_dependence_f32(x, n, ldx, dx, y, ldy, dy, perm, kernel, bwx_dev, bwx, bwy_dev, bwy, rows, sums, ws, nb, None)
    assert call(x=None) == BAD_ARG and call(y=None) == BAD_ARG and call(rows=None) == BAD_ARG and call(sums=None) == BAD_ARG
    assert "null" in lib.am_last_error().decode()
    assert call(kernel=3) == BAD_ARG and call(kernel=-1) == BAD_ARG and "AM_MMD_GAUSSIAN" in lib.am_last_error().decode()
    assert call(n=3) == BAD_SHAPE and "N >= 4" in lib.am_last_error().decode()
    assert call(n=0) == BAD_SHAPE and call(dx=0) == BAD_SHAPE and call(dy=0, ldy=4) == BAD_SHAPE
    assert call(ldx=dx - 4) == BAD_ARG and call(ldy=dy + 2) == BAD_ARG
    assert call(x=ctypes.c_void_p(0x10004)) == BAD_ARG and call(y=ctypes.c_void_p(0x10008)) == BAD_ARG
    big = 1 << 24
    assert call(n=big, nb=1 << 42) == BAD_SHAPE and "4 GiB" in lib.am_last_error().decode()          # X: 2^24 x 64 x 4 bytes
    assert call(n=big, dx=32, ldx=32, ldy=64, nb=1 << 42) == BAD_SHAPE                                # Y alone
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        for kernel in (0, 1):
            assert call(kernel=kernel, bwx=bad) == BAD_ARG and "bw2x" in lib.am_last_error().decode()
            assert call(kernel=kernel, bwy=bad) == BAD_ARG and "bw2y" in lib.am_last_error().decode()
            # a device bandwidth replaces the host one: the call stops at the workspace check
            assert call(kernel=kernel, bwx=bad, bwx_dev=FAKE, bwy=bad, bwy_dev=FAKE, nb=nb - 1) == WORKSPACE
        assert call(kernel=2, bwx=bad, bwy=bad, nb=0) == WORKSPACE                                    # the distance kind takes neither
    assert call(nb=nb - 1) == WORKSPACE and str(nb) in lib.am_last_error().decode()
    assert "am_pair_dependence_workspace_bytes" in lib.am_last_error().decode()
    assert call(ws=None) == WORKSPACE and call(nb=0) == WORKSPACE


def test_workspace_query(lib):
    q = lib.am_pair_dependence_workspace_bytes
    for bad in ((3, 8, 8), (0, 8, 8), (10, 0, 8), (10, 8, 0), (1 << 28, 8, 8)):
        assert q(*bad) == 0, bad
    # the norms and the offset table per padded row, five partials per row and chunk, at most 16 chunks: the widths do not enter
    assert q(1000, 64, 36) == q(1000, 512, 512)
    assert q(4, 64, 64) == q(128, 64, 64) < q(129, 64, 64)                    # whole 128-row tiles
    for n in (4, 2048, 2049, 100_000, 1_000_000):                            # (17 tiles are 9 chunks of 2: fewer partials than 16 tiles)
        pad = -(-n // 128) * 128
        assert q(n, 64, 64) <= pad * (8 + 8 + 4 + 16 * 5 * 8) + 4 * 256, n


# ---------------------------------------------------------------------------------------------------- the kernels' resources
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_no_instantiation_uses_scratch_memory():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    import importlib.util
    spec = importlib.util.spec_from_file_location("am_build", os.path.join(ROOT, "audio-metrics_amd", "_build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)                                         # the flags the shipped library is built with
    r = subprocess.run([hipcc, *build.HIPCC_FLAGS, "--cuda-device-only", "-c", "pair_dependence.hip", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        for key, short in (("ScratchSize \\[bytes/lane\\]", "scratch"), ("VGPRs", "vgprs"), ("AGPRs", "agprs"),
                           ("Occupancy \\[waves/SIMD\\]", "occupancy")):
            m = re.search(r"remark:\s+%s: (\d+)" % key, line)
            if m and name:
                usage[name][short] = int(m.group(1))
    ours = {n: u for n, u in usage.items() if "pdep_" in n}
    tile = {n: u for n, u in ours.items() if "pdep_kernel" in n}
    # what the file declares: one sweep kernel per kind, and the prep / rows / sums kernels
    assert len(tile) == 3 and all(sum("ILi%dEE" % kind in n for n in tile) == 1 for kind in (0, 1, 2)), sorted(tile)
    assert len(ours) == 6 and all(any(small in n for n in ours) for small in ("pdep_prep_kernel", "pdep_rows_kernel", "pdep_sums_kernel"))
    for n, u in ours.items():
        print(n, u)
        assert u["scratch"] == 0, (n, u)
        assert u["vgprs"] + u["agprs"] <= 256 and u["occupancy"] >= 2, (n, u)        # two workgroups of four waves per CU
