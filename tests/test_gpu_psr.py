"""Probabilistic precision and recall on the device (hip_ops.psr_scores, probabilistic_precision_recall,
probabilistic_precision_per_group) against tests/psr_reference.py.

  1  the bits of the engine: the device contract applied to the d2 bits of knn_search - counts exactly, the product of the
     factors within its grouping error;  2  the float64 definition inside error_bound;  3  the dense regime (randn, 40 % of
     all pairs in range);  4  padded views and X is Y;  5  degenerate values;  6  determinism and the sums;  7  the front ends.

The device returns psr = fl(1 - prod), not prod.  The product check |prod_dev - prod_want| <= B, B = 2 c 2^-24 prod_want +
1e-37, is therefore made on psr through the monotone rounding of the subtraction: fl(1 - (prod_want + B)) <= psr_dev <=
fl(1 - (prod_want - B)) - nothing wider than B is admitted, and 1 - psr_dev is never asked to resolve a product below 2^-53.

The shapes are the smallest that cross the edges: 128 + 2 rows, a partial third column tile, one column, D with and
without the inner-dimension tail, 4000 columns for the cross-chunk product."""
import warnings

import numpy as np
import pytest
import torch

import psr_reference as pr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K, A = 4, 1.2
SHAPES = [(130, 300, 40), (257, 130, 64), (130, 1, 40), (130, 4000, 40), (1000, 130, 64)]
DENSE = (400, 500, 64)


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


def randn(seed, n, d):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def padded(a, extra, fill):
    """The same rows as a view of a wider buffer whose padding must never be read as data."""
    buf = torch.full((a.shape[0], a.shape[1] + extra), fill, dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = dev(a)
    return buf[:, :a.shape[1]]


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


def scores(ops, x, y, R, sums=True):
    psr, count, totals = ops.psr_scores(x, y, R, sums=sums)
    assert psr.dtype == torch.float64 and count.dtype == torch.int32
    assert all(t.is_cuda and tuple(t.shape) == (x.shape[0],) for t in (psr, count))
    if sums:
        assert totals.dtype == torch.float64 and tuple(totals.shape) == (2,) and totals.is_cuda
        return psr.cpu().numpy(), count.cpu().numpy(), totals.cpu().numpy()
    assert totals is None
    return psr.cpu().numpy(), count.cpu().numpy(), None


def set_radius(ops, yt):
    return A * float(ops.knn_radii(yt, K).to(torch.float64).mean())


def rows_of(shape):
    n, m, d = shape
    if shape == DENSE:
        return randn(21, n, d), randn(22, m, d)
    return pr.latent_pair(n, m, d)


@pytest.fixture(scope="module")
def cases(ops):
    """Rows, radius, device result, the d2 bits of the search and both oracles of every shape: computed once on first use and
    left unchanged."""
    made = {}

    def get(shape):
        if shape not in made:
            x, y = rows_of(shape)
            xt, yt = dev(x), dev(y)
            if shape[1] == 1:
                R = float(np.median(pr.psr_f64(x, y, 1.0)[2]))             # one column has no k-th neighbour: about half in range
            else:
                R = set_radius(ops, yt)
            psr, count, sums = scores(ops, xt, yt, R)
            d2 = d2_bits_from_the_search(ops, xt, yt)
            made[shape] = dict(x=x, y=y, xt=xt, yt=yt, R=R, psr=psr, count=count, sums=sums, d2=d2,
                               want=pr.psr_from_d2(d2, R), f64=pr.psr_f64(x, y, R))
        return made[shape]
    return get


def check_bits(c, what):
    want_psr, want_count, want_prod = c["want"]
    psr, count, d2 = c["psr"], c["count"], c["d2"]
    assert np.isfinite(d2).all(), what
    bad = np.flatnonzero(count != want_count)
    assert bad.size == 0, (what, bad[:8], count[bad[:8]], want_count[bad[:8]])
    B = 2.0 * want_count * pr.EPS32 * want_prod + 1e-37
    lo, hi = 1.0 - (want_prod + B), 1.0 - (want_prod - B)
    bad = np.flatnonzero(~((lo <= psr) & (psr <= hi)))
    assert bad.size == 0, (what, bad[:8], psr[bad[:8]], want_psr[bad[:8]], want_count[bad[:8]])
    assert (psr[want_count == 0] == 0.0).all(), what
    on_a_row = ((d2 == 0) & (d2 < pr.threshold(c["R"]))).any(1)
    assert (psr[on_a_row] == 1.0).all(), what
    assert ((psr >= 0.0) & (psr <= 1.0)).all(), what
    print(f"{what}: R {c['R']:.4f} mean psr {psr.mean():.4f} mean count {count.mean():.1f} max {count.max()} "
          f"largest |psr - contract| {np.abs(psr - want_psr).max():.2e}")


def check_f64(c, what):
    psr64, count64, d = c["f64"]
    x, y, R = c["x"], c["y"], c["R"]
    bound = pr.error_bound(x, y, d, R)
    err = np.abs(c["psr"] - psr64)
    assert np.isfinite(bound).all()
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: largest error {err.max():.3e} largest bound {bound.max():.3e} median bound {np.median(bound):.3e} "
          f"largest error / bound {ratio:.4f}; mean error {abs(c['psr'].mean() - psr64.mean()):.3e} mean bound {bound.mean():.3e}")
    bad = np.flatnonzero(err > bound)
    assert bad.size == 0, (what, bad[:8], err[bad[:8]], bound[bad[:8]])
    assert abs(c["psr"].mean() - psr64.mean()) <= bound.mean(), what
    # counts differ from the oracle's only on pairs within delta of the radius
    delta = pr.d2_delta(x, y)
    sure, maybe = ((d * d) < R * R - delta).sum(1), ((d * d) <= R * R + delta).sum(1)
    assert ((sure <= c["count"]) & (c["count"] <= maybe)).all(), what
    return ratio


# ---------------------------------------------------------------------------------------------------- 1. the bits of the engine
@pytest.mark.parametrize("shape", SHAPES)
def test_device_contract_on_the_bits_of_the_search(ops, cases, shape):
    n, m, d = shape
    if shape == (130, 4000, 40):
        assert ops.psr_chunks(n, m, d) == 32                               # the cross-chunk product
    c = cases(shape)
    assert 0 < c["count"].sum() and (c["count"] == 0).sum() < n
    check_bits(c, str(shape))


# ---------------------------------------------------------------------------------------------------- 2. the float64 oracle
@pytest.mark.parametrize("shape", SHAPES)
def test_float64_definition_inside_the_error_bound(ops, cases, shape):
    assert check_f64(cases(shape), str(shape)) <= 1.0


# ---------------------------------------------------------------------------------------------------- 3. the dense regime
def test_dense_regime(ops, cases):
    c = cases(DENSE)
    n, m, _ = DENSE
    fraction = c["count"].sum() / (n * m)
    print(f"dense: {100 * fraction:.1f} % of all pairs in range")
    assert 0.2 < fraction < 0.8, fraction                                  # the ungated path: every sub-tile passes the gate
    check_bits(c, "dense")
    assert check_f64(c, "dense") <= 1.0


# ---------------------------------------------------------------------------------------------------- 4. padded views
def test_padded_views_and_a_set_against_itself(ops, cases):
    c = cases((130, 300, 40))
    got = scores(ops, padded(c["x"], 8, float("nan")), padded(c["y"], 24, float("nan")), c["R"])
    for g, w in zip(got, (c["psr"], c["count"], c["sums"])):
        assert np.array_equal(g, w)
    # X is Y: same pointer, one set of norms; a row's own column is in range
    yt = c["yt"]
    R = c["R"]
    alone = scores(ops, yt, yt, R)
    view = padded(c["y"], 12, float("nan"))
    again = scores(ops, view, view, R)
    for g, w in zip(again, alone):
        assert np.array_equal(g, w)
    d2 = d2_bits_from_the_search(ops, yt, yt)
    want_psr, want_count, want_prod = pr.psr_from_d2(d2, R)
    assert np.array_equal(alone[1], want_count) and (alone[1] >= 1).all()
    own_zero = np.diag(d2) == 0
    assert (alone[0][own_zero] == 1.0).all()
    one = alone[0] == 1.0
    assert (own_zero[one] | (want_prod[one] < 2.0 ** -53)).all()          # 1.0 only on a d2 of 0 (or a product below half an ulp of 1)
    print(f"X is Y: {int(own_zero.sum())} of {len(own_zero)} rows have an own d2 of exactly 0, {int(one.sum())} a psr of 1.0")


# ---------------------------------------------------------------------------------------------------- 5. degenerate values
def test_degenerate_values(ops, cases):
    c = cases((130, 300, 40))
    x, y, R = c["x"].copy(), c["y"].copy(), c["R"]
    x[3, 7] = np.nan
    x[64, 0] = np.inf
    x[129, 39] = -np.inf
    x[10] = y[17]                                                          # a candidate on a reference row
    y2 = y.copy()
    y2[5] = np.nan                                                         # in nobody's range
    psr, count, _ = scores(ops, dev(x), dev(y2), R)
    for i in (3, 64, 129):
        assert psr[i] == 0.0 and count[i] == 0, i
    delta = pr.d2_delta(x[np.isfinite(x).all(1)], y)
    assert psr[10] >= 1.0 - np.sqrt(delta) / R and count[10] >= 1
    keep = np.ones(130, dtype=bool)
    keep[[3, 64, 129, 10]] = False
    d2 = c["d2"].copy()
    d2[:, 5] = np.inf
    want = pr.psr_from_d2(d2, R)
    assert np.array_equal(count[keep], want[1][keep])
    assert np.array_equal(count[keep], c["count"][keep] - (c["d2"][:, 5] < pr.threshold(R))[keep])
    # small integers: every sum is exact, a copied row has d2 == 0 and psr exactly 1.0
    rng = np.random.default_rng(8)
    li, lj = rng.integers(-3, 4, (130, 40)).astype(np.float32), rng.integers(-3, 4, (300, 40)).astype(np.float32)
    li[[0, 77, 129]] = lj[[299, 4, 128]]
    lpsr, lcount, _ = scores(ops, dev(li), dev(lj), 9.0)
    want = pr.psr_from_d2(((li[:, None, :].astype(np.float64) - lj[None, :, :]) ** 2).sum(2).astype(np.float32), 9.0)
    assert np.array_equal(lcount, want[1]) and (lpsr[[0, 77, 129]] == 1.0).all() and (lcount == 0).any()
    assert (np.abs(lpsr - want[0]) <= 2.0 * want[1] * pr.EPS32 * want[2] + 1e-16).all()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius"):
            ops.psr_scores(c["xt"], c["yt"], bad)


# ---------------------------------------------------------------------------------------------------- 6. determinism
@pytest.mark.parametrize("shape", SHAPES + [DENSE])
def test_two_calls_return_the_same_bits_and_the_sums_add_up(ops, cases, shape):
    c = cases(shape)
    psr, count, sums = scores(ops, c["xt"], c["yt"], c["R"])
    assert np.array_equal(psr, c["psr"]) and np.array_equal(count, c["count"]) and np.array_equal(sums, c["sums"])
    n = shape[0]
    total = float(np.sum(psr.astype(np.longdouble)))
    assert abs(sums[0] - total) <= n * 2.0 ** -52 * total
    assert sums[1] == float(count.astype(np.int64).sum())
    without = scores(ops, c["xt"], c["yt"], c["R"], sums=False)
    assert np.array_equal(without[0], psr) and np.array_equal(without[1], count)


# ---------------------------------------------------------------------------------------------------- 7. the front ends
def stored(am, rows):
    s = am.AudioMetricsData(True)
    for b in range(0, len(rows), 32):                                      # 32-row adds, like the embedding pipeline
        s.add(dev(rows[b:b + 32]))
    return s


def test_front_ends(am, ops, monkeypatch):
    n, m, d = 300, 257, 40
    x, y = pr.latent_pair(n, m, d)
    cand, ref = stored(am, x), stored(am, y)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                     # no saturation on the latent rows
        res = am.probabilistic_precision_recall(cand, ref, return_rows=True)
    assert list(res) == ["p_precision", "p_recall", "p_radius_reference", "p_radius_candidate", "p_in_range_reference",
                         "p_in_range_candidate", "nearest_k", "a", "candidate_psr", "candidate_in_range", "reference_psr",
                         "reference_in_range"]
    assert res["nearest_k"] == 4 and res["a"] == 1.2
    r_ref, r_cand = res["p_radius_reference"], res["p_radius_candidate"]
    # the radii: a * mean of the f32 k-NN radii, against the float64 ones inside the d2 bound of the engine
    for got, rows in ((r_ref, y), (r_cand, x)):
        r64 = pr.knn_radii_f64(rows, 4)
        delta = pr.d2_delta(rows, rows)
        assert abs(got - 1.2 * r64.mean()) <= 1.2 * (np.minimum(delta / r64, np.sqrt(delta)).mean() + 2 * pr.EPS32 * r64.mean())
    assert r_ref == pytest.approx(4.418, abs=2e-3) and r_cand == pytest.approx(4.113, abs=2e-3)
    # values against the oracle at the radii the front end used
    for (a, b, R), key, rows_key, cnt_key in (((x, y, r_ref), "p_precision", "candidate_psr", "candidate_in_range"),
                                              ((y, x, r_cand), "p_recall", "reference_psr", "reference_in_range")):
        psr64, count64, dist = pr.psr_f64(a, b, R)
        bound = pr.error_bound(a, b, dist, R)
        assert (np.abs(res[rows_key] - psr64) <= bound).all(), key
        assert abs(res[key] - psr64.mean()) <= bound.mean(), key
        assert res[rows_key].dtype == np.float64 and res[cnt_key].dtype == np.int32
        # the per-row vectors are the direct call's, bit for bit
        direct = scores(ops, dev(a), dev(b), R)
        assert np.array_equal(res[rows_key], direct[0]) and np.array_equal(res[cnt_key], direct[1])
        assert res[key] == direct[2][0] / len(a)
    assert res["p_in_range_reference"] == res["candidate_in_range"].astype(np.int64).sum() / n / m
    assert res["p_in_range_candidate"] == res["reference_in_range"].astype(np.int64).sum() / m / n
    assert res["p_precision"] == pytest.approx(0.735, abs=5e-3) and res["p_recall"] == pytest.approx(0.696, abs=5e-3)
    # the same pass from the other side
    swapped = am.probabilistic_precision_recall(ref, cand)
    assert swapped["p_recall"] == res["p_precision"] and swapped["p_precision"] == res["p_recall"]
    assert swapped["p_radius_candidate"] == r_ref and swapped["p_radius_reference"] == r_cand
    assert "candidate_psr" not in swapped

    # per group, against psr_by_group of the per-row vector
    labels = np.random.default_rng(9).integers(0, 7, n).astype(np.int64) * 3 - 5
    for g in (labels, torch.as_tensor(labels).to(DEV)):
        grouped = am.probabilistic_precision_per_group(cand, ref, g)
        want = am.psr_by_group(labels, res["candidate_psr"])
        for key in ("group_labels", "group_sizes", "p_precision_per_group"):
            assert np.array_equal(grouped[key], want[key]), key
        assert grouped["p_radius_reference"] == r_ref and grouped["nearest_k"] == 4 and grouped["a"] == 1.2

    # the cached radii are reused: nothing computes radii again
    def forbidden(*a, **k):
        raise AssertionError("the radii were computed again")
    with monkeypatch.context() as mp:
        mp.setattr(ops, "knn_radii", forbidden)
        mp.setattr(cand, "get_radii", forbidden)
        mp.setattr(ref, "get_radii", forbidden)
        again = am.probabilistic_precision_recall(cand, ref)
        assert again["p_precision"] == res["p_precision"] and again["p_recall"] == res["p_recall"]
    # explicit radii skip get_radii on fresh sets
    fresh_c, fresh_r = stored(am, x), stored(am, y)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "knn_radii", forbidden)
        mp.setattr(fresh_c, "get_radii", forbidden)
        mp.setattr(fresh_r, "get_radii", forbidden)
        explicit = am.probabilistic_precision_recall(fresh_c, fresh_r, radius_reference=r_ref, radius_candidate=r_cand)
        assert explicit["p_precision"] == res["p_precision"] and explicit["p_recall"] == res["p_recall"]
        assert fresh_c.radii == {} and fresh_r.radii == {}
    # an append: get_radii keeps its old vector, the radius is computed from fresh radii of all stored rows
    more = pr.latent_rows(40, d, 3, 5, 0.0)
    ref.add(dev(more))
    assert ref.get_radii(4).shape[0] == m
    grown = am.probabilistic_precision_recall(cand, ref)
    assert ref.get_radii(4).shape[0] == m
    all_rows = dev(np.concatenate([y, more]))
    assert grown["p_radius_reference"] == pytest.approx(set_radius(ops, all_rows), rel=1e-13) and grown["p_radius_reference"] != r_ref
    assert grown["p_radius_candidate"] == r_cand
    assert grown["p_precision"] == float(ops.psr_scores(dev(x), all_rows, grown["p_radius_reference"])[2][0]) / n


def test_saturation_warning_and_non_finite_radii(am, ops):
    a, b = stored(am, randn(31, 300, 512)), stored(am, randn(32, 257, 512))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        res = am.probabilistic_precision_recall(a, b)
    hits = [w for w in rec if issubclass(w.category, RuntimeWarning) and "saturate" in str(w.message)]
    assert len(hits) == 1, [str(w.message) for w in rec]
    assert max(res["p_in_range_reference"], res["p_in_range_candidate"]) > am.metrics.pprecall.SATURATION_FRACTION
    # a row with a NaN element has a non-finite k-NN radius: left out of the mean, one warning
    x, y = pr.latent_pair(300, 257, 40)
    y_bad = y.copy()
    y_bad[11, 3] = np.nan
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = am.probabilistic_precision_recall(stored(am, x), stored(am, y_bad))
    assert sum("left out" in str(w.message) for w in rec) == 1 and not any("saturate" in str(w.message) for w in rec), \
        [str(w.message) for w in rec]
    r64 = pr.knn_radii_f64(np.delete(y, 11, axis=0), 4)
    assert got["p_radius_reference"] == pytest.approx(1.2 * r64.mean(), rel=1e-5)
    all_bad = y.copy()
    all_bad[:, 0] = np.inf
    with pytest.raises(ValueError, match="no finite"):
        am.probabilistic_precision_recall(stored(am, x), stored(am, all_bad))
    f64 = am.AudioMetricsData(True)
    f64.add(dev(x[:64].astype(np.float64)))
    with pytest.raises(NotImplementedError, match="float64"):
        am.probabilistic_precision_recall(f64, stored(am, y))
    with pytest.raises(NotImplementedError, match=r"psr_scores takes float32 rows \(the float64 matrix-core form is not implemented\)"):
        ops.psr_scores(dev(x[:64].astype(np.float64)), dev(y), 1.0)
