"""Per-sample realism, ball count and rarity on the device (hip_ops.sample_scores, sample_fidelity, sample_fidelity_per_group).

  1  lattice rows: all five outputs bit for bit against the numpy-f32 oracle (tests/fidelity_reference.py), through one and
     through 32 column chunks, exact ties included;  2  randn rows: the definition applied to the d2 bits of knn_search, the
     counts of prdc_counts;  3  padded views;  4  degenerate values;  5  determinism;  6  the front ends against prdc().

The shapes are the smallest that cross the edges: 128 + 2 rows, a partial third column tile, one column, D with and
without the inner-dimension tail, 4000 columns for the cross-chunk merge."""
import numpy as np
import pytest
import torch

import fidelity_reference as fr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ("realism", "realism_index", "ball_count", "rarity", "rarity_index")


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    audio_metrics_amd._lib.load()
    return audio_metrics_amd


@pytest.fixture(scope="module")
def ops(am):
    return am.hip_ops


@pytest.fixture(scope="module")
def lattice():
    """The oracle of every lattice case, computed once and left unchanged."""
    cases = {c[:3]: fr.lattice_oracle(*c) for c in fr.LATTICE_CASES}
    cases[(130, 1, 40)] = fr.lattice_oracle(130, 1, 40, 5, False)          # one column: its radius is +inf (no k-th neighbour)
    return cases


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def randn(seed, n, d):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def as_bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32) if v.dtype == np.float32 else v


def scores(ops, x, y, r):
    out = ops.sample_scores(x, y, r)
    assert [t.dtype for t in out] == [torch.float32, torch.int64, torch.int32, torch.float32, torch.int64]
    assert all(t.is_cuda and tuple(t.shape) == (x.shape[0],) for t in out)
    return tuple(t.cpu().numpy() for t in out)


def assert_same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        bad = np.flatnonzero(as_bits(g) != as_bits(w))
        assert bad.size == 0, (what, name, bad[:8], g[bad[:8]], w[bad[:8]])


def padded(a, extra, fill):
    """The same rows as a view of a wider buffer whose padding must never be read as data."""
    buf = torch.full((a.shape[0], a.shape[1] + extra), fill, dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = dev(a)
    view = buf[:, :a.shape[1]]
    assert view.stride(0) == a.shape[1] + extra
    return view


# ---------------------------------------------------------------------------------------------------- 1. lattice, bit-exact
@pytest.mark.parametrize("n,m,d", [(130, 300, 40), (130, 300, 64), (257, 130, 40), (130, 1, 40), (130, 4000, 40)])
def test_lattice_rows_match_the_oracle_bit_for_bit(ops, lattice, n, m, d):
    case = lattice[(n, m, d)]
    if m == 4000:
        assert ops.sample_scores_chunks(n, m, d) == 32                     # the cross-chunk merge, ties across chunks
    if m > 1:
        print(fr.check_lattice_is_not_degenerate(case, case["tie_heavy"]))
    got = scores(ops, dev(case["x"]), dev(case["y"]), dev(case["r"]))
    assert_same(got, case["want"], (n, m, d))


# ---------------------------------------------------------------------------------------------------- 2. randn, existing bits
def d2_bits_from_the_search(ops, x, y):
    """The full f32 [n, m] matrix of squared distances, assembled from knn_search on blocks of 32 rows of y (row slices of a
    contiguous matrix stay 16-byte aligned): every pair's d2 with the bits of the exact kernels."""
    n, m = x.shape[0], y.shape[0]
    d2 = torch.full((n, m), float("inf"), dtype=torch.float32, device=DEV)
    for b in range(0, m, 32):
        dist, idx = ops.knn_search(x, y[b:b + 32], 32, squared=True)
        found = idx >= 0
        rows = torch.arange(n, device=DEV)[:, None].expand_as(idx)
        d2[rows[found], idx[found] + b] = dist[found]
    return d2.cpu().numpy()


@pytest.mark.parametrize("n,m,d", [(130, 300, 40), (1000, 130, 64), (130, 4000, 40)])
def test_randn_rows_have_the_bits_of_the_search_and_of_prdc(ops, n, m, d):
    k = 5
    x, y = randn(n + m, n, d), randn(n + m + d, m, d)
    near = min(n // 2, m)
    x[:near] = y[:near] + 0.05 * randn(3, near, d)                         # samples near the manifold, the rest far from it
    xt, yt = dev(x), dev(y)
    r_y, r_x = ops.knn_radii(yt, k), ops.knn_radii(xt, k)
    got = scores(ops, xt, yt, r_y)
    want = fr.scores_from_d2(d2_bits_from_the_search(ops, xt, yt), r_y.cpu().numpy())
    assert 0 < (want[2] > 0).sum() < n
    for name in ("realism", "realism_index", "rarity", "rarity_index"):
        i = NAMES.index(name)
        assert np.array_equal(as_bits(got[i]), as_bits(want[i])), name
    col_count = ops.prdc_counts(yt, xt, r_y, r_x)[0].cpu().numpy()
    assert np.array_equal(got[2], col_count.astype(np.int32))
    assert np.array_equal(got[2], want[2])


# ---------------------------------------------------------------------------------------------------- 3. views and padding
@pytest.mark.parametrize("d", [40, 64])
def test_padded_views_give_the_bits_of_contiguous_rows(ops, lattice, d):
    case = lattice[(130, 300, d)]
    got = scores(ops, padded(case["x"], 8, 1e30), padded(case["y"], 24, 1e30), dev(case["r"]))
    assert_same(got, case["want"], d)
    x, y = randn(5, 130, d), randn(6, 300, d)
    r = ops.knn_radii(dev(y), 5)
    assert_same(scores(ops, padded(x, 4, float("nan")), padded(y, 12, float("inf")), r), scores(ops, dev(x), dev(y), r), d)


# ---------------------------------------------------------------------------------------------------- 4. degenerate values
def test_non_finite_sample_rows_score_nothing(ops):
    n, m, d = 257, 300, 40
    x, y = randn(11, n, d), randn(12, m, d)
    r = ops.knn_radii(dev(y), 5)
    clean = scores(ops, dev(x), dev(y), r)
    xb = x.copy()
    xb[130, 3] = np.nan
    xb[200, 0] = np.inf
    xb[5, 39] = -np.inf
    bad = [5, 130, 200]
    got = scores(ops, dev(xb), dev(y), r)
    for i in bad:
        assert got[0][i] == 0 and got[1][i] == -1 and got[2][i] == 0 and got[3][i] == 0 and got[4][i] == -1, (i, [g[i] for g in got])
    keep = np.setdiff1d(np.arange(n), bad)
    assert_same([g[keep] for g in got], [c[keep] for c in clean])


def test_non_finite_reference_rows_and_bad_radii_are_nobodys_ball(ops):
    n, m, d, k = 130, 300, 40, 5
    x, y = randn(21, n, d), randn(22, m, d)
    x[:40] = y[:40] + 0.05 * randn(23, 40, d)
    drop = np.array([0, 7, 129, 299])
    # a non-finite reference row: its radius (knn_radii) is +inf, its distance to everything is +inf
    yb = y.copy()
    yb[0, 1], yb[7, 0], yb[129, 39], yb[299, 5] = np.nan, np.inf, -np.inf, np.nan
    r_bad = ops.knn_radii(dev(yb), k)
    assert torch.isinf(r_bad[torch.as_tensor(drop, device=DEV)]).all()
    got = scores(ops, dev(x), dev(yb), r_bad)
    keep = np.setdiff1d(np.arange(m), drop)
    # the same set without those rows, with the radii the others had beside them
    sub = scores(ops, dev(x), dev(yb[keep]), r_bad[torch.as_tensor(keep, device=DEV)].contiguous())
    assert not np.isin(got[1], drop).any() and not np.isin(got[4], drop).any()
    for i in (0, 2, 3):
        assert np.array_equal(as_bits(got[i]), as_bits(sub[i])), NAMES[i]
    for i in (1, 4):
        assert np.array_equal(got[i], np.where(sub[i] >= 0, keep[np.maximum(sub[i], 0)], -1)), NAMES[i]
    # radii of 0, negative or NaN passed explicitly: those rows are ignored
    r = ops.knn_radii(dev(y), k)
    r_cut = r.clone()
    r_cut[torch.as_tensor(drop, device=DEV)] = torch.tensor([0.0, -1.0, float("nan"), -float("inf")], device=DEV)
    got = scores(ops, dev(x), dev(y), r_cut)
    sub = scores(ops, dev(x), dev(y[keep]), r[torch.as_tensor(keep, device=DEV)].contiguous())
    for i in (0, 2, 3):
        assert np.array_equal(as_bits(got[i]), as_bits(sub[i])), NAMES[i]
    for i in (1, 4):
        assert np.array_equal(got[i], np.where(sub[i] >= 0, keep[np.maximum(sub[i], 0)], -1)), NAMES[i]
    # no positive radius at all
    none = scores(ops, dev(x), dev(y), torch.zeros(m, device=DEV))
    assert (none[0] == 0).all() and (none[1] == -1).all() and (none[2] == 0).all() and (none[3] == 0).all() and (none[4] == -1).all()


def test_a_sample_on_a_reference_row_and_a_set_of_identical_rows(ops, lattice):
    # lattice rows: the squared distance of two equal rows is exactly 0 (on randn rows the Gram form leaves a rounding residue,
    # in the search as here)
    case = lattice[(130, 300, 40)]
    m, d, k = 300, 40, 5
    x, y, r = case["x"].copy(), case["y"], case["r"]
    x[3], x[129] = y[250], y[17]
    got = scores(ops, dev(x), dev(y), dev(r))
    for i, j in ((3, 250), (129, 17)):
        assert np.isposinf(got[0][i]) and got[1][i] == j and got[2][i] >= 1
        assert 0 < got[3][i] <= r[j]
    # X may be Y: nothing is skipped
    own = scores(ops, dev(y), dev(y), dev(r))
    assert np.isposinf(own[0]).all() and np.array_equal(own[1], np.arange(m)) and (own[2] >= 1).all()
    assert_same(own, fr.scores_from_d2(fr.exact_d2(y, y), r), "X is Y")
    # k + 1 identical rows: every radius is 0, nobody is a member, every ratio is 0 (0 / 0 on the rows themselves)
    same = np.repeat(fr.int_rows(33, 1, d), k + 1, axis=0)
    r0 = ops.knn_radii(dev(same), k)
    assert (r0 == 0).all()
    xs = np.concatenate([same[:2], fr.int_rows(34, 128, d)])
    got = scores(ops, dev(xs), dev(same), r0)
    assert (got[0] == 0).all() and (got[1] == -1).all() and (got[2] == 0).all() and (got[3] == 0).all() and (got[4] == -1).all()


# ---------------------------------------------------------------------------------------------------- 5. determinism
def test_two_calls_return_the_same_bits(ops, lattice):
    case = lattice[(130, 4000, 40)]                                        # the tie-heavy case, 32 column chunks
    x, y, r = dev(case["x"]), dev(case["y"]), dev(case["r"])
    a, b = scores(ops, x, y, r), scores(ops, x, y, r)
    assert_same(a, b)


# ---------------------------------------------------------------------------------------------------- 6. front ends
def test_front_ends_agree_with_prdc_exactly(am):
    rng = np.random.default_rng(41)
    n, m, d, k = 2000, 3000, 64, 5
    y = rng.standard_normal((m, d)).astype(np.float32)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[: n // 2] += 1.5                                                     # a shifted half: precision neither 0 nor 1
    samples, manifold = am.AudioMetricsData(True), am.AudioMetricsData(True)
    for rows, dst in ((x, samples), (y, manifold)):
        for s in range(0, len(rows), 32):                                  # 32-row adds, like the embedding pipeline
            dst.add(dev(rows[s:s + 32]))
    res = am.sample_fidelity(samples, manifold, nearest_k=k)
    assert sorted(res) == sorted([*NAMES, "in_manifold", "nearest_k", "precision", "density"])
    assert res["realism"].dtype == np.float32 and res["rarity"].dtype == np.float32 and res["ball_count"].dtype == np.int32
    assert res["realism_index"].dtype == np.int64 and res["rarity_index"].dtype == np.int64 and res["in_manifold"].dtype == bool
    assert all(res[name].shape == (n,) for name in (*NAMES, "in_manifold")) and res["nearest_k"] == k
    want = am.prdc(manifold, samples, k)
    assert 0 < want["precision"] < 1
    assert res["precision"] == want["precision"] and res["density"] == want["density"]       # no tolerance
    assert np.array_equal(res["in_manifold"], res["ball_count"] > 0)
    assert (res["rarity"][res["in_manifold"]] > 0).all() and (res["rarity"][~res["in_manifold"]] == 0).all()
    assert (res["rarity_index"][~res["in_manifold"]] == -1).all() and (res["realism_index"] >= 0).all()

    groups = rng.integers(0, 37, size=n) * 3 - 20                           # unsorted, negative labels included
    for g in (groups, torch.as_tensor(groups).to(DEV)):
        per = am.sample_fidelity_per_group(samples, manifold, g, nearest_k=k, return_rows=True)
        for name in (*NAMES, "in_manifold"):
            assert np.array_equal(as_bits(per[name]), as_bits(res[name])), name
        host = am.fidelity_by_group(groups, res["realism"], res["ball_count"], res["rarity"], k)
        assert sorted(host) == ["density_per_group", "group_labels", "group_sizes", "precision_per_group",
                                "rarity_median_per_group", "realism_median_per_group"]
        for name, v in host.items():
            assert np.array_equal(per[name], v, equal_nan=True), name
        assert per["group_sizes"].sum() == n and np.array_equal(per["group_labels"], np.unique(groups))
        assert per["nearest_k"] == k
    short = am.sample_fidelity_per_group(samples, manifold, groups, nearest_k=k)
    assert "realism" not in short and np.array_equal(short["precision_per_group"], host["precision_per_group"])
    # the size-weighted mean of the per-group precision is the precision
    assert abs((short["precision_per_group"] * short["group_sizes"]).sum() / n - res["precision"]) < 1e-12

    f64 = am.AudioMetricsData(True)
    f64.add(dev(x[:64].astype(np.float64)))
    for a, b in ((f64, manifold), (samples, f64)):
        with pytest.raises(NotImplementedError, match="float64"):
            am.sample_fidelity(a, b, nearest_k=k)
    with pytest.raises(NotImplementedError, match="float64"):
        am.sample_fidelity_per_group(f64, manifold, np.zeros(64, dtype=np.int64), nearest_k=k)
    with pytest.raises(NotImplementedError, match=r"sample_scores takes float32 rows \(the float64 matrix-core form is not implemented\)"):
        am.hip_ops.sample_scores(dev(x[:64].astype(np.float64)), dev(y), manifold.get_radii(k))
