"""The KAD permutation test, the part that needs no GPU: mmd_permutation_null against relabel-and-recompute, the p-value
formula, the seeded labellings, the calibration of the test on seeded draws (blocks of iid rows; songs of windows; and single
rows of windowed data, which MUST fail - the reason the units are songs), the argument checks of the front end before any
library call, the new names in header / signature table / package, and the error paths and workspace query of
am_mmd_rbf_cells_f32."""
import ctypes
import math
import os
import re
import warnings

import numpy as np
import pytest
import torch

import kad_reference as ka
import kd_reference as kr
import mmd_cells_reference as mc
import mmd_rows_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -4
FAKE = ctypes.c_void_p(0x10000)                       # 16-byte aligned, never dereferenced: the calls stop at validation
NAMES = ("am_mmd_rbf_cells_workspace_bytes", "am_mmd_rbf_cells_f32")


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
    rng = np.random.default_rng(21)
    x, y = kr.rbf_rows(rng, 70, 16, 10.0), kr.rbf_rows(rng, 45, 16, 10.0)
    gamma = 1.0 / 200.0

    def k(a, b):
        return np.exp(-((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum() * gamma)
    got = mc.unit_sums(x, y, gamma)
    assert got["xx"].shape == (3, 3) and got["yy"].shape == (2, 2) and got["xy"].shape == (3, 2)
    want = sum(k(x[i], x[j]) for i in range(32, 64) for j in range(64, 70))
    np.testing.assert_allclose(got["xx"][1, 2], want, rtol=1e-13)
    want = sum(k(y[i], y[j]) for i in range(32, 45) for j in range(32, 45) if i != j)
    np.testing.assert_allclose(got["yy"][1, 1], want, rtol=1e-13)
    want = sum(k(x[i], y[j]) for i in range(64, 70) for j in range(0, 32))
    np.testing.assert_allclose(got["xy"][2, 0], want, rtol=1e-13)
    assert np.allclose(got["xx"], got["xx"].T, rtol=1e-14, atol=0.0) and 0.0 < got["scale"] <= 1.0
    # the totals are those of the row-sum oracle
    rows = mr.row_sums(x, y, gamma)
    np.testing.assert_allclose([got["xx"].sum(), got["yy"].sum(), got["xy"].sum()], [rows["w"].sum(), rows["v"].sum(), rows["c"].sum()],
                               rtol=1e-13)
    # a list with holes: the -1 positions move rows into other cells and contribute nothing
    idx = np.full(96, -1, dtype=np.int64)
    idx[:40], idx[64:94] = np.arange(40), np.arange(40, 70)
    listed = mc.unit_sums(x, y, gamma, idx_x=idx, units_x=[0, 2, 3])
    assert listed["xx"].shape == (2, 2) and listed["xy"].shape == (2, 2)
    np.testing.assert_allclose(listed["xx"][0, 1], sum(k(x[i], x[j]) for i in range(40) for j in range(40, 70)), rtol=1e-13)
    np.testing.assert_allclose(listed["xy"][1].sum(), sum(k(x[i], y[j]) for i in range(40, 70) for j in range(45)), rtol=1e-13)


# ---------------------------------------------------------------------------------------------------- the host logic
def ragged_case(seed=31):
    """pooled rows in 9 units of ragged sizes, 4 of them X: (K, unit of every row, sizes, G)"""
    rng = np.random.default_rng(seed)
    sizes = np.array([5, 17, 2, 9, 30, 1, 12, 7, 3])
    z = rng.standard_normal((int(sizes.sum()), 6))
    z[:33] += 0.4
    K = np.exp(-ka.d2_matrix(z, z) / 12.0)
    unit = np.repeat(np.arange(len(sizes)), sizes)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    G = K.copy()
    np.fill_diagonal(G, 0.0)
    return K, unit, sizes, mc.fold(G, offs, offs)


def test_null_equals_relabel_and_recompute(am):
    """50 random labellings of ragged units: within 1e-12 of mean |K| of the direct recomputation, the p-value equal"""
    K, unit, sizes, G = ragged_case()
    want_obs, want_null, want_p = mc.permutation_null(K, unit, 4, 50, seed=7)
    limit = 1e-12 * np.abs(K).mean()
    for form in (G, torch.as_tensor(G)):
        t_obs, null, p = am.mmd_permutation_null(form, sizes, 4, n_permutations=50, seed=7)
        assert isinstance(null, np.ndarray) and null.dtype == np.float64 and null.shape == (50,)
        err = max(abs(t_obs - want_obs), float(np.abs(null - want_null).max()))
        print(f"max |err| {err:.3e} limit {limit:.3e}")
        assert err <= limit and p == want_p
    assert len({tuple(sorted(s)) for s in mc.labellings(9, 4, 50, 7)}) > 30       # the labellings do differ


def test_identity_labelling_reproduces_the_row_sum_mmd2(am):
    rng = np.random.default_rng(32)
    x, y = rng.standard_normal((70, 8)) + 0.3, rng.standard_normal((45, 8))
    s = mr.row_sums(x, y, 1.0 / 32.0)
    want, _ = am.mmd_standard_error(s["w"], s["c"], s["v"], s["r"])
    cells = mc.unit_sums(x, y, 1.0 / 32.0)
    t_obs, _, _ = am.mmd_permutation_null(mc.pooled(cells), [32, 32, 6, 32, 13], 3, n_permutations=5, seed=0)
    assert abs(t_obs - want) <= 1e-12 * cells["scale"]


def test_p_value_formula_on_a_hand_made_null(am):
    """Four units of two rows and a G whose statistic is known for every labelling: p = (1 + #{T_p >= T_obs}) / (1 + P), ties
    counting as exceeding."""
    G = np.array([[2.0, 1.0, 0.0, 0.0], [1.0, 2.0, 0.0, 0.0], [0.0, 0.0, 2.0, 1.0], [0.0, 0.0, 1.0, 2.0]])
    sizes = [2, 2, 2, 2]
    t_obs, null, p = am.mmd_permutation_null(G, sizes, 2, n_permutations=40, seed=3)
    # identity: XX = YY = 6 over 4 * 3 ordered pairs each, XY = 0 -> T = 1; the same for the complement; every mixed
    # labelling: XX = YY = 4, XY = 2 -> T = 4 / 12 + 4 / 12 - 4 / 16 = 5 / 12
    assert t_obs == pytest.approx(1.0, abs=1e-15)
    same = np.array([set(s) in ({0, 1}, {2, 3}) for s in mc.labellings(4, 2, 40, 3)])
    assert 0 < same.sum() < 40
    np.testing.assert_allclose(null, np.where(same, 1.0, 5.0 / 12.0), atol=1e-15)
    assert p == (1.0 + same.sum()) / 41.0
    # a labelling that leaves a side fewer than 2 rows has no statistic and counts as exceeding
    t_obs, null, p = am.mmd_permutation_null(np.ones((3, 3)), [1, 1, 5], 2, n_permutations=30, seed=1)
    lone = np.array([2 in s for s in mc.labellings(3, 2, 30, 1)])                # X = {a small unit, the big one}: Y keeps one row
    assert lone.any() and np.array_equal(np.isnan(null), lone)
    assert p == (1.0 + np.count_nonzero(~(null < t_obs))) / 31.0 and p >= (1.0 + lone.sum()) / 31.0
    for bad in (dict(n_x_units=0), dict(n_x_units=4), dict(n_permutations=0), dict(sizes=[2, 2, 2]), dict(sizes=[2, 0, 2, 2])):
        kw = dict(sizes=sizes, n_x_units=2, n_permutations=10)
        kw.update(bad)
        with pytest.raises(ValueError):
            am.mmd_permutation_null(G, kw.pop("sizes"), kw.pop("n_x_units"), **kw)
    with pytest.raises(ValueError, match="square"):
        am.mmd_permutation_null(np.ones((3, 4)), [1, 1, 1], 1)


def test_one_seed_one_set_of_labellings(am):
    _, _, sizes, G = ragged_case()
    a = am.mmd_permutation_null(G, sizes, 4, n_permutations=60, seed=11)
    b = am.mmd_permutation_null(G, sizes, 4, n_permutations=60, seed=11)
    c = am.mmd_permutation_null(G, sizes, 4, n_permutations=60, seed=12)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert a[0] == c[0] and not np.array_equal(a[1], c[1])
    # a longer run continues the shorter one: the draws are one stream
    longer = am.mmd_permutation_null(G, sizes, 4, n_permutations=80, seed=11)
    assert np.array_equal(longer[1][:60], a[1])


# ---------------------------------------------------------------------------------------------------- calibration
DRAWS, PERMS, DIM = 300, 199, 8


def iid_draw(rng, shift=0.0):
    x = rng.standard_normal((256, DIM))
    y = rng.standard_normal((224, DIM)) + shift
    return x, y


def song_draw(rng, shift=0.0):
    cx = rng.standard_normal((16, 1, DIM))
    cy = rng.standard_normal((14, 1, DIM)) + shift
    x = (cx + 0.3 * rng.standard_normal((16, 16, DIM))).reshape(-1, DIM)
    y = (cy + 0.3 * rng.standard_normal((14, 16, DIM))).reshape(-1, DIM)
    return x, y


def p_values(am, draw, unit_rows, shift=0.0):
    """the p-value of every seeded draw: bandwidth^2 = the median squared distance of y's pairs, units = runs of unit_rows rows"""
    out = []
    for s in range(DRAWS):
        x, y = draw(np.random.default_rng(1000 + s), shift)
        d2 = ka.d2_matrix(y, y)
        gamma = 0.5 / float(np.median(d2[np.triu_indices(len(y), 1)]))
        K = mc.pooled_gram(x, y, gamma)
        np.fill_diagonal(K, 0.0)
        offs = np.concatenate([np.arange(0, len(x), unit_rows), len(x) + np.arange(0, len(y), unit_rows), [len(x) + len(y)]])
        sizes = np.diff(offs)
        out.append(am.mmd_permutation_null(mc.fold(K, offs, offs), sizes, len(x) // unit_rows, n_permutations=PERMS, seed=s)[2])
    return np.array(out)


@pytest.mark.parametrize("name, draw, unit_rows", [("iid rows in blocks of 32", iid_draw, 32), ("songs of 16 windows", song_draw, 16)])
def test_the_test_is_calibrated_under_equality(am, name, draw, unit_rows):
    """300 seeded draws of two sets from ONE distribution, 199 permutations each: the rejection rate at the 5 % level in
    [0.02, 0.09] and the mean p in [0.45, 0.56] - about 3 binomial standard deviations (measured when the units were chosen:
    0.047 / 0.511 for the blocks, 0.063 / 0.509 for the songs)."""
    p = p_values(am, draw, unit_rows)
    rate = float((p <= 0.05).mean())
    print(f"{name}: rejection rate {rate:.3f} mean p {p.mean():.3f}")
    assert 0.02 <= rate <= 0.09, rate
    assert 0.45 <= p.mean() <= 0.56, p.mean()


def test_permuting_rows_of_windowed_data_is_invalid(am):
    """the same song data with single rows as units: equal distributions are rejected in at least 90 % of the draws (measured
    100 %) - windows of one song are not exchangeable, which is why the front end takes groups"""
    p = p_values(am, song_draw, 1)
    rate = float((p <= 0.05).mean())
    print(f"songs, rows permuted: rejection rate {rate:.3f}")
    assert rate >= 0.9, rate


def test_a_shift_is_found(am):
    """a shift of 0.25 on the iid data gives the smallest possible p, 1 / 200, in at least 95 % of the draws (measured 100 %):
    nothing is lost to the coarser unit"""
    p = p_values(am, iid_draw, 32, shift=0.25)
    hit = float((p == 1.0 / 200.0).mean())
    print(f"shift 0.25: p = 1/200 in {hit:.3f} of the draws")
    assert hit >= 0.95, hit


# ---------------------------------------------------------------------------------------------------- the front end on the host
def host_cell_sums(calls):
    """ops.mmd_rbf_cell_sums emulated by the oracle on host tensors (and every call recorded)"""
    def cell_sums(x, y, idx_x=None, idx_y=None, units_x=None, units_y=None, blocks=7, gamma=None, bw2=None):
        assert gamma is not None and bw2 is None
        calls.append(dict(blocks=blocks, idx_x=idx_x, idx_y=idx_y, units_x=units_x, units_y=units_y))
        lst = lambda t: None if t is None else t.numpy()
        s = mc.unit_sums(x.numpy(), y.numpy(), gamma, lst(idx_x), lst(idx_y), units_x, units_y)
        return tuple(torch.as_tensor(s[k]) if blocks & b else None for k, b in (("xx", 1), ("yy", 2), ("xy", 4)))
    return cell_sums


def test_front_end_on_the_host(am, monkeypatch):
    """The front end with the library call replaced by the oracle: units from runs and from labels, the pooled matrix, the
    statistic against relabel-and-recompute, the reference-side cache, the warning about too few relabellings."""
    from audio_metrics_amd import hip_ops
    from audio_metrics_amd.metrics import kad
    calls = []
    monkeypatch.setattr(hip_ops, "mmd_rbf_cell_sums", host_cell_sums(calls))
    rng = np.random.default_rng(41)
    x, y = rng.standard_normal((150, 8)).astype(np.float32) + 0.2, rng.standard_normal((100, 8)).astype(np.float32)
    sx, sy = host_set(am, torch.as_tensor(x)), host_set(am, torch.as_tensor(y))
    bw = 4.0
    gamma = 1.0 / (2.0 * bw * bw)
    K = mc.pooled_gram(x, y, gamma)
    limit = 1e-12 * np.abs(K).mean()
    # default units: runs of 32 rows, 5 + 4 units
    got = am.kernel_audio_distance_permutation_test(sx, sy, n_permutations=60, seed=5, bandwidth=bw, return_null=True)
    unit = np.concatenate([mc.run_units(150, 32), mc.run_units(100, 32, 5)])
    t_obs, null, p = mc.permutation_null(K, unit, 5, 60, 5)
    assert list(got) == ["kad", "kad_mmd2", "kad_bandwidth", "kad_p_value", "kad_null_mean", "kad_null_std", "kad_null_q95", "kad_units",
                         "kad_n_permutations", "kad_null"]
    assert got["kad_units"] == (5, 4) and got["kad_n_permutations"] == 60 and got["kad_bandwidth"] == bw
    assert abs(got["kad_mmd2"] - t_obs) <= limit and np.abs(got["kad_null"] - null).max() <= limit and got["kad_p_value"] == p
    assert got["kad"] == 100.0 * got["kad_mmd2"]
    np.testing.assert_allclose([got["kad_null_mean"], got["kad_null_std"], got["kad_null_q95"]],
                               [100.0 * null.mean(), 100.0 * null.std(ddof=1), 100.0 * np.quantile(null, 0.95)], rtol=1e-9)
    assert calls[-1]["blocks"] == 7 and calls[-1]["units_x"] is None and calls[-1]["idx_x"] is None
    # the reference's YY matrix is cached under (gamma, unit_rows): the second call asks for XX | XY only and returns the bits
    cache = kad.reference_cache(sy)
    assert list(cache.cells) == [(kad._gamma_bits(gamma), 32)] and cache.syy == {} and cache.vrow == {}
    again = am.kernel_audio_distance_permutation_test(sx, sy, n_permutations=60, seed=5, bandwidth=bw, return_null=True)
    assert calls[-1]["blocks"] == 5 and again["kad_mmd2"] == got["kad_mmd2"] and np.array_equal(again["kad_null"], got["kad_null"])
    assert "kad_null" not in am.kernel_audio_distance_permutation_test(sx, sy, n_permutations=10, bandwidth=bw)
    # runs of 64 rows: cell offsets, a short last unit on both sides; another cache entry
    with pytest.warns(RuntimeWarning, match="10 distinct relabellings"):
        got = am.kernel_audio_distance_permutation_test(sx, sy, unit_rows=64, n_permutations=30, seed=2, bandwidth=bw, return_null=True)
    assert calls[-1]["units_x"] == [0, 2, 4, 5] and calls[-1]["units_y"] == [0, 2, 4] and got["kad_units"] == (3, 2)
    unit = np.concatenate([mc.run_units(150, 64), mc.run_units(100, 64, 3)])
    t_obs, null, p = mc.permutation_null(K, unit, 3, 30, 2)
    assert abs(got["kad_mmd2"] - t_obs) <= limit and np.nanmax(np.abs(got["kad_null"] - null)) <= limit and got["kad_p_value"] == p
    assert len(cache.cells) == 2
    # labels in shuffled stored order: one unit per label, padded to whole cells with -1; the reference side keeps its runs
    songs = rng.permutation(np.repeat(np.arange(3), 50))
    got = am.kernel_audio_distance_permutation_test(sx, sy, x_groups=songs, n_permutations=30, seed=2, bandwidth=bw, return_null=True)
    idx = calls[-1]["idx_x"].numpy()
    assert calls[-1]["units_x"] == [0, 2, 4, 6] and idx.shape == (192,) and calls[-1]["idx_y"] is None and calls[-1]["blocks"] == 5
    for u in range(3):
        assert np.array_equal(idx[64 * u:64 * u + 50], np.flatnonzero(songs == u)) and (idx[64 * u + 50:64 * u + 64] == -1).all()
    t_obs, null, p = mc.permutation_null(K, np.concatenate([songs, mc.run_units(100, 32, 3)]), 3, 30, 2)
    assert abs(got["kad_mmd2"] - t_obs) <= limit and np.abs(got["kad_null"] - null).max() <= limit and got["kad_p_value"] == p
    # labels on the reference side: nothing is cached for them
    before = dict(cache.cells)
    ref_songs = np.repeat(np.arange(4), 25)
    got = am.kernel_audio_distance_permutation_test(sx, sy, y_groups=ref_songs, n_permutations=20, bandwidth=bw)
    assert calls[-1]["blocks"] == 7 and got["kad_units"] == (5, 4) and cache.cells == before
    # an append drops the cache with everything else the reference side keeps
    sy._content_version = getattr(sy, "_content_version", 0) + 1
    assert kad.reference_cache(sy).cells == {}
    # fewer distinct relabellings than permutations: one RuntimeWarning
    assert math.comb(5, 3) < 20
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        am.kernel_audio_distance_permutation_test(sx, sy, unit_rows=64, n_permutations=20, bandwidth=bw)
    assert len(rec) == 1 and issubclass(rec[0].category, RuntimeWarning) and "10 distinct relabellings" in str(rec[0].message)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        am.kernel_audio_distance_permutation_test(sx, sy, n_permutations=20, bandwidth=bw)
    assert not rec


def test_validation_happens_before_any_library_call(am, monkeypatch):
    from audio_metrics_amd import hip_ops

    def forbidden(*a, **k):
        raise AssertionError("library call before validation")
    for name in ("as_matrix", "_call", "_workspace", "mmd_rbf_cell_sums", "pairwise_select_sq", "mmd_rbf_sums"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    test = am.kernel_audio_distance_permutation_test
    x, y = torch.zeros((100, 8)), torch.zeros((120, 8))
    ok, ref = host_set(am, x), host_set(am, y)
    for bad in (16, 48, 0, -32, 33.5):
        with pytest.raises(ValueError, match="multiple of 32"):
            test(ok, ref, unit_rows=bad)
    with pytest.raises(ValueError, match="candidate set has fewer than 2 units"):
        test(ok, ref, unit_rows=128)
    with pytest.raises(ValueError, match="reference set has fewer than 2 units"):
        test(host_set(am, torch.zeros((300, 8))), ref, unit_rows=128)
    with pytest.raises(ValueError, match="candidate set has fewer than 2 units"):
        test(ok, ref, x_groups=np.zeros(100, dtype=np.int64))
    with pytest.raises(ValueError, match="reference set has fewer than 2 units"):
        test(ok, ref, y_groups=np.full(120, 7))
    for kw in (dict(x_groups=np.arange(99)), dict(y_groups=np.arange(121))):
        with pytest.raises(ValueError, match="one label per row"):
            test(ok, ref, **kw)
    with pytest.raises(ValueError, match="integer labels"):
        test(ok, ref, x_groups=np.linspace(0.0, 1.0, 100))
    for a, b in ((host_set(am, x.double()), ref), (ok, host_set(am, y.double())), (host_set(am, x.double()), host_set(am, y.double()))):
        with pytest.raises(NotImplementedError, match="float32 rows"):
            test(a, b)
        with pytest.raises(NotImplementedError, match="float64 rows"):
            test(a, b, x_groups=np.arange(100) // 10, y_groups=np.arange(120) // 10)
    with pytest.raises(ValueError, match="feature widths"):
        test(ok, host_set(am, torch.zeros((120, 12))))
    with pytest.raises(ValueError, match="at least 2 rows in the candidate"):
        test(host_set(am, torch.zeros((1, 8))), ref)
    with pytest.raises(ValueError, match="keeps none"):
        test(ok, am.AudioMetricsData(False))
    with pytest.raises(ValueError, match="n_permutations"):
        test(ok, ref, n_permutations=0)
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="bandwidth"):
            test(ok, ref, bandwidth=bad, n_permutations=50)
    # the wrapper: everything that can be said about the arguments is said before the library is loaded
    def sums(a=x, b=y, **kw):
        kw.setdefault("gamma", 0.5)
        return hip_ops.mmd_rbf_cell_sums(a, b, **kw)
    monkeypatch.undo()
    for name in ("as_matrix", "_call", "_workspace"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    for kw in (dict(a=x.double()), dict(b=y.double())):
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
    for bad in ([0, 2], [1, 4], [0, 2, 2, 4], [0, 5], [0]):          # 100 rows are 4 cells
        with pytest.raises(ValueError, match="units_x"):
            sums(units_x=bad)
    with pytest.raises(ValueError, match="units_y"):
        sums(units_y=[0, 3], idx_y=torch.zeros(128, dtype=torch.int64))          # the list decides the number of cells
    with pytest.raises(ValueError, match="idx_x"):
        sums(idx_x=torch.zeros((2, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="idx_y"):
        sums(idx_y=torch.zeros(4))


def test_default_unit_rows():
    from audio_metrics_amd.metrics import kad_perm
    assert kad_perm._default_unit_rows(100, 100) == 32
    assert kad_perm._default_unit_rows(131_072, 131_072) == 32                    # 262 144 pooled rows: 8192 units of 32
    assert kad_perm._default_unit_rows(131_073, 131_072) == 64
    assert kad_perm._default_unit_rows(1_000_000, 500_000) == 192
    idx, offs, sizes = kad_perm._run_units(150, 64)
    assert idx is None and offs == [0, 2, 4, 5] and sizes.tolist() == [64, 64, 22]
    assert kad_perm._run_units(64, 32)[1] is None and kad_perm._run_units(65, 32)[2].tolist() == [32, 32, 1]


# ---------------------------------------------------------------------------------------------------- names
def test_header_signature_table_and_package_agree(am, lib):
    with open(os.path.join(ROOT, "include", "audio_metrics_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in am._lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"#define AM_MMD_CELL 32\b", header) and am.hip_ops.MMD_CELL == 32
    assert len(am._lib.SIGNATURES["am_mmd_rbf_cells_f32"][1]) == 24
    assert len(am._lib.SIGNATURES["am_mmd_rbf_cells_workspace_bytes"][1]) == 4
    from audio_metrics_amd.metrics import kad, kad_perm
    assert am.metrics.kad_perm is kad_perm
    for name in ("mmd_permutation_null", "kernel_audio_distance_permutation_test"):
        assert getattr(am, name) is getattr(kad_perm, name), name
    assert callable(am.hip_ops.mmd_rbf_cell_sums)
    assert kad._ReferenceCache((0, 0)).cells == {}
    from audio_metrics_amd import audio_metrics as front                   # it is not a metric name of AudioMetrics
    assert not any("perm" in k for k, _ in front.EVALUATION_TABLE)


# ---------------------------------------------------------------------------------------------------- entry point
def test_error_paths(lib):
    n1, n2, d = 1000, 300, 64
    c1, c2 = 32, 10
    nb = lib.am_mmd_rbf_cells_workspace_bytes(n1, n2, d, 7)
    assert nb > 0
    arr = lambda *v: ctypes.cast((ctypes.c_int64 * len(v))(*v), ctypes.c_void_p)

    def call(x=FAKE, n1=n1, ldx=d, idx_x=None, p1=n1, ux=None, u1=0, y=FAKE, n2=n2, ldy=d, idx_y=None, p2=n2, uy=None, u2=0, d=d,
             bw2_dev=None, gamma=0.5, blocks=7, xx=FAKE, yy=FAKE, xy=FAKE, ws=FAKE, nb=nb):
        return lib.am_mmd_rbf_cells_f32(x, n1, ldx, idx_x, p1, ux, u1, y, n2, ldy, idx_y, p2, uy, u2, d, bw2_dev, gamma, blocks, xx, yy, xy,
                                        ws, nb, None)
    err = lambda: lib.am_last_error().decode()
    assert call(x=None) == BAD_ARG and call(y=None) == BAD_ARG and "null" in err()
    assert call(blocks=0) == BAD_ARG and call(blocks=8) == BAD_ARG and "AM_MMD_XX" in err()
    # an output may be missing only if its block is not named
    for name, bit in (("xx", 1), ("yy", 2), ("xy", 4)):
        for blocks in range(1, 8):
            rc = call(blocks=blocks, nb=0, **{name: None})
            assert rc == (BAD_ARG if blocks & bit else WORKSPACE), (name, blocks)
            assert not blocks & bit or "out_" + name in err()
    assert call(n1=0) == BAD_SHAPE and call(n2=0) == BAD_SHAPE and call(d=0) == BAD_SHAPE
    assert call(ldx=d - 4) == BAD_ARG and call(ldy=d + 2) == BAD_ARG and "ld" in err()
    assert call(x=ctypes.c_void_p(0x10004)) == BAD_ARG and call(y=ctypes.c_void_p(0x10008)) == BAD_ARG
    big = 1 << 24
    assert call(n1=big, p1=big, nb=1 << 40) == BAD_SHAPE and "4 GiB" in err()
    assert call(gamma=-1.0) == BAD_ARG and call(gamma=float("nan")) == BAD_ARG and "gamma" in err()
    assert call(gamma=-1.0, bw2_dev=FAKE, nb=nb - 1) == WORKSPACE           # a device bandwidth replaces the host one
    # positions: without a list they are the stored rows; with one, any number below 2^30
    assert call(p1=n1 - 1) == BAD_SHAPE and "n1_pos" in err() and call(p2=n2 + 1) == BAD_SHAPE and "n2_pos" in err()
    assert call(idx_x=FAKE, p1=0) == BAD_SHAPE and call(idx_y=FAKE, p2=1 << 30) == BAD_SHAPE and "2^30" in err()
    assert call(idx_x=FAKE, p1=5000, nb=0) == WORKSPACE and call(idx_y=FAKE, p2=7, nb=0) == WORKSPACE
    # units: U + 1 offsets from 0 to the number of cells, strictly increasing
    assert call(ux=arr(0, 10, c1), u1=2, uy=arr(0, 1, 5, c2), u2=3, nb=nb - 1) == WORKSPACE
    assert call(ux=arr(1, 10, c1), u1=2) == BAD_ARG and "units_x" in err()
    assert call(uy=arr(0, 5, c2 + 1), u2=2) == BAD_ARG and "units_y" in err()
    assert call(ux=arr(0, 10, 10, c1), u1=3) == BAD_SHAPE and "unit 1" in err()
    assert call(ux=arr(0, 12, 10, c1), u1=3) == BAD_SHAPE
    assert call(ux=arr(0, c1), u1=0) == BAD_SHAPE and call(uy=arr(*range(c2 + 2)), u2=c2 + 1) == BAD_SHAPE
    assert call(idx_x=FAKE, p1=64, ux=arr(0, 1, 2), u1=2, nb=0) == WORKSPACE           # the list decides the number of cells
    assert call(nb=nb - 1) == WORKSPACE and str(nb) in err() and "am_mmd_rbf_cells_workspace_bytes" in err()
    assert call(ws=None) == WORKSPACE and call(nb=0) == WORKSPACE
    assert call(blocks=5, nb=lib.am_mmd_rbf_cells_workspace_bytes(n1, n2, d, 5) - 1) == WORKSPACE
    assert call(n1=1, p1=1, nb=0) == WORKSPACE and call(n2=1, p2=1, nb=0) == WORKSPACE


def test_workspace_query(lib):
    q = lib.am_mmd_rbf_cells_workspace_bytes
    for bad in ((0, 10, 64, 7), (10, 0, 64, 7), (10, 10, 0, 7), (10, 10, 64, 0), (10, 10, 64, 8), (1 << 30, 10, 64, 7)):
        assert q(*bad) == 0, bad
    # 100 000 x 100 000 positions: three cell matrices of 3125^2 doubles (78 MB each) and 12 bytes of tables per position
    full = q(100_000, 100_000, 512, 7)
    cells = 3125 * 3125 * 8
    assert 3 * cells < full < 3 * cells + (4 << 20), full
    assert q(100_000, 100_000, 128, 7) == full
    for blocks in range(1, 8):
        assert 0 < q(20_000, 5_000, 64, blocks) <= q(20_000, 5_000, 64, 7), blocks
    # a cached reference: XX | XY against 1 000 candidate rows stays small
    assert q(1_000, 100_000, 512, 5) < 4 << 20
