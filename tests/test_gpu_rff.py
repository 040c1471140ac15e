"""Random Fourier features, their moment matrix and the three scores built on it, on the device against the float64 oracle of
tests/rff_reference.py (the same float32 rows, the same float32 frequencies).

  1   features at the tile edges: every |F - oracle| within R^(-1/2) ((D + 16) 2^-24 |x_i| |w_l| inv_bw + 2^-50)
  2   bits: a frequency alone and among others, a row under any (row0, nrows), two calls, nothing written outside [2R][nrows]
  3   moment: exactly symmetric, trace 1, within 4 n 2^-52 / R of F F^T / n of the device's own features; the fold over chunks
  4   end to end with the same W: eigenvalues within Weyl's bound, every order within the log-score bound derived from it
  5   against the exact routes (rke_score, vendi_score on the Gram route) on the 1200 x 32 cluster set
  6   rke_score against the f64 oracle
  7   closed form: identical rows
  8   a non-finite row
  9   novelty: a set against itself, the planted cluster, the reference cache
  10  bandwidth=None through the shared KAD cache"""
import math
import warnings

import numpy as np
import pytest
import torch

import kad_reference as ka
import kd_reference as kr
import rff_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ORDERS = (1.0, 2.0, math.inf)


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    audio_metrics_amd._lib.load()
    return audio_metrics_amd


@pytest.fixture(scope="module")
def ops(am):
    return am.hip_ops


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def rows(seed, n, d, shift=0.0):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32) + np.float32(shift)


def data_set(am, a):
    s = am.AudioMetricsData(True)
    s.add(dev(a))
    return s


# ---------------------------------------------------------------------------------------------------- 1 features
@pytest.mark.parametrize("n", [1, 63, 129, 257])
@pytest.mark.parametrize("d", [1, 31, 32, 65, 512])
def test_features_against_the_oracle_at_the_tile_edges(ops, n, d):
    x = rows(1000 * n + d, n, d, 0.25)
    inv_bw = 1.3 / math.sqrt(d)
    for r in (1, 33, 130):
        w = ref.frequencies(d, r, 5)
        f = ops.rff_features(dev(x), dev(w), inv_bw=inv_bw)
        assert f.shape == (2 * r, n) and f.dtype == torch.float64
        got, want, bound = f.cpu().numpy(), ref.features(x, w, inv_bw), ref.feature_bound(x, w, inv_bw)
        ratio = float((np.abs(got - want) / np.concatenate([bound, bound])).max())
        print(f"features {n} x {d}, R = {r}: largest error / bound {ratio:.4f}")
        assert ratio <= 1.0, (n, d, r, ratio)


# ---------------------------------------------------------------------------------------------------- 2 bits
def test_feature_bits_depend_on_nothing_but_the_frequency_and_the_row(ops):
    n, d, r = 300, 40, 130
    x, w = dev(rows(3, n, d)), dev(ref.frequencies(d, r, 9))
    inv_bw = 0.2
    whole = ops.rff_features(x, w, inv_bw=inv_bw)
    assert torch.equal(ops.rff_features(x, w, inv_bw=inv_bw), whole)                        # two calls
    # every third frequency alone: R^(-1/2) is another number then, so cos and sin themselves are compared.  Either side is four
    # roundings away from them (R^(-1/2) on the device, the scaling, sqrt(R) here, the multiplication here), each 2^-53 relative
    # of a value <= 1: 2^-50 in all
    some = ops.rff_features(x, w[::3].contiguous(), inv_bw=inv_bw)
    rs = some.shape[0] // 2
    third = torch.cat([whole[:r][::3], whole[r:][::3]])
    assert float((some * math.sqrt(rs) - third * math.sqrt(r)).abs().max()) <= 2.0 ** -50
    # the same R with the frequencies in another order, at other tile positions: the same bits
    same_r = ops.rff_features(x, torch.cat([w[::3], w[1::3], w[2::3]]).contiguous(), inv_bw=inv_bw)
    perm = torch.cat([torch.arange(0, r, 3), torch.arange(1, r, 3), torch.arange(2, r, 3)]).to(DEV)
    assert torch.equal(same_r[:r], whole[:r][perm]) and torch.equal(same_r[r:], whole[r:][perm])
    # three row ranges against the whole
    for row0, nrows in ((0, 129), (129, 70), (199, 101)):
        part = ops.rff_features(x, w, inv_bw=inv_bw, row0=row0, nrows=nrows)
        assert part.shape == (2 * r, nrows) and torch.equal(part, whole[:, row0:row0 + nrows]), (row0, nrows)
    # a device bandwidth gives the bits of the number it stands for
    bw2 = torch.tensor(1.0 / (inv_bw * inv_bw), dtype=torch.float32, device=DEV)
    assert float(bw2) == 25.0 and torch.equal(ops.rff_features(x, w, bw2=bw2), whole)
    # a poisoned out: columns from nrows on keep the poison, the rest is the result; the count is 0
    out = torch.full((2 * r, 136), -7.0, dtype=torch.float64, device=DEV)
    back, check = ops.rff_features(x, w, inv_bw=inv_bw, row0=129, nrows=70, out=out, return_check=True)
    assert back is out and torch.equal(out[:, :70], whole[:, 129:199]) and bool((out[:, 70:] == -7.0).all()) and check() == 0
    # the last rows of the matrix: nothing is read or written past row N
    tail = ops.rff_features(x, w, inv_bw=inv_bw, row0=n - 1)
    assert tail.shape == (2 * r, 1) and torch.equal(tail, whole[:, n - 1:])


# ---------------------------------------------------------------------------------------------------- 3 moment
@pytest.mark.parametrize("n,d,r", [(300, 65, 1024), (1000, 32, 33), (20_000, 64, 64)])
def test_moment_is_symmetric_of_trace_one_and_the_gram_of_its_own_features(ops, n, d, r):
    x, w = dev(rows(n + r, n, d)), dev(ref.frequencies(d, r, 2))
    inv_bw = 1.0 / math.sqrt(2.0 * d)
    chunks = ops.rff_moment_chunks(n, r)
    if n == 20_000:
        assert chunks >= 3                                                                  # the fold over chunks runs
    s, check = ops.rff_moment(x, w, inv_bw=inv_bw)
    assert s.shape == (2 * r, 2 * r) and s.dtype == torch.float64 and check() == 0
    assert torch.equal(s, s.T)
    again, _ = ops.rff_moment(x, w, inv_bw=inv_bw)
    assert torch.equal(again, s)
    got = s.cpu().numpy()
    trace = abs(float(np.trace(got)) - 1.0)
    f = ops.rff_features(x, w, inv_bw=inv_bw).cpu().numpy()
    err = float(np.abs(got - (f @ f.T) / n).max())
    bound = 4.0 * n * 2.0 ** -52 / r
    print(f"moment {n} x {d}, R = {r}, {chunks} chunks: |trace - 1| {trace:.3e}, largest |s - F F^T / n| / bound {err / bound:.4f}")
    assert trace <= 1e-13 and err <= bound


# ---------------------------------------------------------------------------------------------------- 4 end to end
@pytest.mark.parametrize("n,d,r,seed", [(300, 65, 130, 1), (1000, 32, 256, 4), (5000, 64, 64, 0)])
def test_scores_against_the_oracle_with_the_same_frequencies(am, n, d, r, seed):
    x = rows(7 * n + d, n, d)
    bw = math.sqrt(2.0 * d)
    got = am.vendi_score_rff(dev(x), orders=ORDERS + (3.0,), bandwidth=bw, n_features=r, seed=seed, return_eigenvalues=True)
    w = ref.frequencies(d, r, seed)
    lam = ref.eigenvalues(x, w, 1.0 / bw)
    eps = ref.eigenvalue_bound(x, w, 1.0 / bw)
    dev_lam = got["vendi_rff_eigenvalues"]
    assert dev_lam.shape == lam.shape == (min(n, 2 * r),) and got["vendi_rff_features"] == r and got["vendi_rff_seed"] == seed
    assert got["vendi_rff_bandwidth"] == bw and got["vendi_rff_orders"] == ORDERS + (3.0,)
    err = float(np.abs(dev_lam - lam).max())
    print(f"{n} x {d}, R = {r}: largest eigenvalue error {err:.3e}, bound {eps:.3e}")
    assert err <= eps
    want = ref.scores(lam, ORDERS + (3.0,))
    for q, g, wv in zip(ORDERS + (3.0,), got["vendi_rff_per_order"], want):
        bound = ref.log_score_bound(lam, eps, q)
        print(f"    order {q}: device {g!r} oracle {wv!r} |ln ratio| {abs(math.log(g / wv)):.3e} bound {bound:.3e}")
        assert abs(math.log(g / wv)) <= bound, (q, g, wv, bound)
    assert got["vendi_rff"] == got["vendi_rff_per_order"][0] and got["vendi_rff_rank"] == int((dev_lam > 0.0).sum())
    assert got["vendi_rff_per_order"][1] == pytest.approx(1.0 / float(np.sum(dev_lam ** 2)), rel=1e-14)


# ---------------------------------------------------------------------------------------------------- 5 the exact routes
def test_against_the_exact_routes_on_the_cluster_set(am):
    x = ref.cluster_set()
    bw = ref.median_bandwidth(x)
    xd = dev(x)
    seed, r = 0, 1024
    got = am.vendi_score_rff(xd, orders=(1.0, 2.0), bandwidth=bw, n_features=r, seed=seed)
    rke = am.rke_score(xd, bandwidth=bw)
    gram = am.vendi_score(xd, "gaussian", orders=(1.0,), bandwidth=bw, route="gram")
    w = ref.frequencies(x.shape[1], r, seed)
    lam, exact = ref.eigenvalues(x, w, 1.0 / bw), ref.exact_eigenvalues(x, bw)
    eps = ref.eigenvalue_bound(x, w, 1.0 / bw)
    oracle_gap = np.abs(np.log(ref.scores(lam, (1.0, 2.0))) - np.log(ref.scores(exact, (1.0, 2.0))))
    gap1 = abs(math.log(got["vendi_rff_per_order"][0]) - math.log(gram["vendi"]))
    gap2 = abs(math.log(got["vendi_rff_per_order"][1]) - math.log(rke["rke"]))
    print(f"order 1: |ln(rff / gram route)| {gap1:.4e} (oracle's own gap {oracle_gap[0]:.4e});  "
          f"order 2: |ln(rff / rke)| {gap2:.4e} (oracle's own gap {oracle_gap[1]:.4e})")
    assert gap1 <= min(oracle_gap[0] + ref.log_score_bound(lam, eps, 1.0), 0.1)
    assert gap2 <= min(oracle_gap[1] + ref.log_score_bound(lam, eps, 2.0), 0.1)


# ---------------------------------------------------------------------------------------------------- 6 rke
def test_rke_score_against_the_oracle(am):
    """The normalised kernel sum within MARGIN x the emulated error of the same sum, as tests/test_gpu_kad.py holds Sxx
    (f32 dot products rounded once per 32-element slab; MARGIN covers the matrix cores' rounding after every product); rke =
    n^2 / (n + S) moves by |dS| / (n + S) relative."""
    n, d = 1000, 64
    x = rows(61, n, d)
    bw = ref.median_bandwidth(x)
    gamma = 1.0 / (bw * bw)
    want, _ = ka.mmd_parts(x, x, gamma)
    emulated, _ = ka.mmd_parts(x, x, gamma, dots=kr.emulated_dots("f32"))
    limit = kr.MARGIN * abs(emulated[0] - want[0])
    got = am.rke_score(dev(x), bandwidth=bw)
    mean = got["rke_sum"] / (n * (n - 1.0))
    want_rke, want_sum = ref.rke_exact(x, bw)
    print(f"rke {got['rke']!r} oracle {want_rke!r};  Sxx / (n (n - 1)): |err| {abs(mean - want[0]):.3e} limit {limit:.3e}")
    assert want_sum / (n * (n - 1.0)) == pytest.approx(want[0], rel=1e-12)                  # the two oracles agree
    assert abs(mean - want[0]) <= limit and got["rke_bandwidth"] == bw
    assert abs(got["rke"] / want_rke - 1.0) <= limit * n * (n - 1.0) / (n + want_sum) + 4 * 2.0 ** -52
    assert got["rke"] == n * n / (n + got["rke_sum"])


# ---------------------------------------------------------------------------------------------------- 7 closed form
def test_identical_rows_have_one_mode(am):
    x = np.tile(rows(8, 1, 48), (200, 1))
    got = am.vendi_score_rff(dev(x), orders=ORDERS + (4.0,), bandwidth=3.0, n_features=96, return_eigenvalues=True)
    print("identical rows:", got["vendi_rff_per_order"], got["vendi_rff_rank"])
    assert np.abs(got["vendi_rff_per_order"] - 1.0).max() <= 1e-12 and got["vendi_rff_rank"] == 1
    assert abs(am.rke_score(dev(x), bandwidth=3.0)["rke"] - 1.0) <= 1e-12


# ---------------------------------------------------------------------------------------------------- 8 non-finite
def test_a_non_finite_row_gives_nan_and_is_left_out_of_the_moment(am, ops):
    n, d, r = 5000, 40, 48
    x = rows(12, n, d)
    bad = x.copy()
    bad[4500, 7] = np.nan
    w = dev(ref.frequencies(d, r, 0))
    s_bad, check = ops.rff_moment(dev(bad), w, inv_bw=0.1)
    assert check() == 1 and bool(torch.isfinite(s_bad).all())
    clean, check_clean = ops.rff_moment(dev(np.delete(x, 4500, axis=0)), w, inv_bw=0.1)
    assert check_clean() == 0
    err = float((s_bad * n - clean * (n - 1)).abs().max())
    print("non-finite row: largest |n s - (n - 1) s_clean|", err)
    assert err <= 4.0 * n * 2.0 ** -52 / r * n                                              # two sums of the same terms, chunked differently
    f, fcheck = ops.rff_features(dev(bad), w, inv_bw=0.1, row0=4400, nrows=200, return_check=True)
    assert fcheck() == 1 and bool((f[:, 100] == 0.0).all()) and bool((f[:, 99] != 0.0).any())
    inf = x.copy()
    inf[0, 0], inf[1, 3], inf[1, 4] = np.inf, -np.inf, np.nan
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = am.vendi_score_rff(dev(inf), bandwidth=9.0, n_features=r, return_eigenvalues=True, modes=2)
    assert len(caught) == 1 and issubclass(caught[0].category, RuntimeWarning) and "2 rows" in str(caught[0].message)
    assert math.isnan(got["vendi_rff"]) and np.isnan(got["vendi_rff_per_order"]).all() and got["vendi_rff_rank"] == 0
    assert np.isnan(got["vendi_rff_eigenvalues"]).all() and got["vendi_rff_bandwidth"] == 9.0 and np.isnan(got["mode_scores"]).all()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        nov = am.kernel_novelty_score(dev(x), dev(bad), bandwidth=9.0, n_features=r)
    assert len(caught) == 1 and "1 rows" in str(caught[0].message) and math.isnan(nov["ken"]) and math.isnan(nov["novel_mass"])


# ---------------------------------------------------------------------------------------------------- 9 novelty
def test_a_set_has_no_novelty_against_itself(am):
    x = data_set(am, rows(5, 700, 32))
    got = am.kernel_novelty_score(x, x, eta=1.0, n_features=128)
    assert got["novel_mass"] == 0.0 and got["ken"] == 0.0 and got["novel_modes"] == 0.0 and got["novel_eigenvalues"].size == 0
    assert got["ken_eta"] == 1.0 and got["ken_bandwidth"] > 0.0


def test_the_planted_cluster_is_the_novel_mode_and_the_reference_is_cached(am, ops, monkeypatch):
    from audio_metrics_amd.metrics.kad import reference_cache
    refrows, cand, lab, same = ref.planted_sets()
    y, xc, xs = data_set(am, refrows), data_set(am, cand), data_set(am, same)
    calls = []
    moment = ops.rff_moment
    monkeypatch.setattr(ops, "rff_moment", lambda rows_, *a, **k: calls.append(int(rows_.shape[0])) or moment(rows_, *a, **k))
    got = am.kernel_novelty_score(xc, y, eta=1.0, n_features=1024, seed=0, modes=2, rows_per_mode=20)
    assert calls == [900, 700] and list(reference_cache(y).rff) == [(("median",), 1024, 0)]
    lam = got["mode_eigenvalues"]
    print("planted: top", lam[0], "second", lam[1], "mass", got["novel_mass"], "modes", got["novel_modes"])
    assert lam[0] >= 10.0 * lam[1] and got["mode_rows"].shape == (2, 20) and got["mode_rows"].dtype == np.int64
    assert (lab[got["mode_rows"][0]] == 4).all()
    assert (np.diff(got["mode_scores"], axis=1) <= 0.0).all() and got["mode_scores"][0, 0] > 0.0
    assert got["novel_eigenvalues"][0] == lam[0] and got["novel_mass"] >= lam[0] and got["novel_modes"] >= 1.0
    # the oracle at the bandwidth the device reports: eigenvalues, and the rows of mode 0
    bw = got["ken_bandwidth"]
    assert bw == pytest.approx(ref.median_bandwidth(refrows), rel=1e-6)
    w = ref.frequencies(32, 1024, 0)
    want_lam, want_vec, fc = ref.novelty(cand, refrows, w, 1.0 / bw, 1.0)
    eps = 2.0 * max(ref.eigenvalue_bound(cand, w, 1.0 / bw), ref.eigenvalue_bound(refrows, w, 1.0 / bw))      # S_cand and eta S_ref each move
    assert abs(lam[0] - want_lam[0]) <= eps and abs(lam[1] - want_lam[1]) <= eps
    want_rows, want_scores = ref.mode_rows(fc, want_vec[0], 20)
    assert set(got["mode_rows"][0]) == set(want_rows) or np.abs(np.sort(got["mode_scores"][0]) - np.sort(want_scores)).max() <= 1e-3
    # the same law: a top eigenvalue at most half as large; the reference's matrix is not computed again and the bits are those
    # of an uncached call
    calls.clear()
    plain = am.kernel_novelty_score(xs, y, eta=1.0, n_features=1024, seed=0, modes=1)
    print("same law: top", plain["mode_eigenvalues"][0])
    assert calls == [700] and lam[0] >= 2.0 * plain["mode_eigenvalues"][0]
    calls.clear()
    uncached = am.kernel_novelty_score(dev(same), dev(refrows), eta=1.0, bandwidth=plain["ken_bandwidth"], n_features=1024, seed=0, modes=1)
    fixed = am.kernel_novelty_score(xs, y, eta=1.0, bandwidth=plain["ken_bandwidth"], n_features=1024, seed=0, modes=1)
    again = am.kernel_novelty_score(xs, y, eta=1.0, bandwidth=plain["ken_bandwidth"], n_features=1024, seed=0, modes=1)
    assert calls == [900, 700, 900, 700, 700] and len(reference_cache(y).rff) == 2
    for key in ("ken", "novel_mass", "novel_modes"):
        assert uncached[key] == fixed[key] == again[key], key
    assert np.array_equal(uncached["novel_eigenvalues"], again["novel_eigenvalues"]) and np.array_equal(uncached["mode_rows"], again["mode_rows"])
    # an append drops the cache
    y.add(dev(refrows[:5]))
    assert reference_cache(y).rff == {}


def test_mode_rows_on_a_small_set_with_ties(am):
    """duplicated rows tie exactly: the smallest indices win, in order; the sign makes the scores sum to >= 0"""
    base = rows(2, 50, 16)
    x = np.concatenate([base, base, base])                                                   # row i = row i + 50 = row i + 100
    got = am.vendi_score_rff(dev(x), bandwidth=4.0, n_features=32, modes=3, rows_per_mode=4, return_eigenvalues=True)
    w = ref.frequencies(16, 32, 0)
    f = ref.features(x, w, 0.25)
    assert np.array_equal(got["mode_eigenvalues"], got["vendi_rff_eigenvalues"][:3])
    lam, vec = np.linalg.eigh((f @ f.T) / len(x))
    for j in range(3):
        s = np.tile(vec[:, -1 - j] @ f[:, :50], 3)                                          # the oracle's ties are exact by construction
        s = -s if s.sum() < 0.0 else s
        want_rows = np.argsort(-s, kind="stable")[:4]
        assert want_rows[1] == want_rows[0] + 50 and want_rows[2] == want_rows[0] + 100 and want_rows[3] < 50
        assert np.array_equal(got["mode_rows"][j], want_rows), (j, got["mode_rows"][j], want_rows)
        assert np.abs(got["mode_scores"][j] - s[want_rows]).max() <= 1e-6, (j, got["mode_scores"][j], s[want_rows])


# ---------------------------------------------------------------------------------------------------- 10 the shared cache
def test_median_bandwidth_through_the_shared_cache(am, monkeypatch):
    """bandwidth=None is the median pairwise distance of x's own rows through the cache a KAD reference fills: computed once,
    and every score equals the one at the bandwidth it reports to 1e-12 (the bar of
    test_gaussian_median_bandwidth_and_the_shared_cache: the device forms 1 / sqrt(bw2), the host 1 / sqrt(bw2) from the same
    float32 - a few 2^-52 apart at most)."""
    n, d = 129, 20
    x = rows(77, n, d)
    data = data_set(am, x)
    calls = []
    select = am.hip_ops.pairwise_select_sq
    monkeypatch.setattr(am.hip_ops, "pairwise_select_sq", lambda *a, **k: calls.append(1) or select(*a, **k))
    first = am.vendi_score_rff(data, n_features=64)
    second = am.vendi_score_rff(data, n_features=64)
    rke = am.rke_score(data)
    gram = am.vendi_score(data, kernel="gaussian")
    nov = am.kernel_novelty_score(data_set(am, rows(78, 100, d)), data, n_features=64)
    assert len(calls) == 1
    assert first["vendi_rff_bandwidth"] == second["vendi_rff_bandwidth"] == rke["rke_bandwidth"] == gram["vendi_bandwidth"] == nov["ken_bandwidth"]
    assert np.array_equal(first["vendi_rff_per_order"], second["vendi_rff_per_order"])
    bw = first["vendi_rff_bandwidth"]
    assert bw == pytest.approx(ref.median_bandwidth(x), rel=1e-6)
    fixed = am.vendi_score_rff(data, n_features=64, bandwidth=bw)
    rel = float(np.abs(fixed["vendi_rff_per_order"] / first["vendi_rff_per_order"] - 1.0).max())
    rel_rke = abs(am.rke_score(data, bandwidth=bw)["rke"] / rke["rke"] - 1.0)
    print("median bandwidth against the same number:", rel, rel_rke)
    assert rel <= 1e-12 and rel_rke <= 1e-12 and fixed["vendi_rff_rank"] == first["vendi_rff_rank"]
    # a plain tensor has no cache to fill, and gives the same bits
    plain = am.vendi_score_rff(data.embeddings, n_features=64)
    assert len(calls) == 2 and plain["vendi_rff"] == first["vendi_rff"] and plain["vendi_rff_bandwidth"] == bw
