"""K-means on the device (hip_ops.kmeans_assign / kmeans_update, kmeans) and the MAUVE score.

  1  assign has the bits of knn_search(k = 1, squared), through one and through 32 column chunks;  2  exact ties go to the
  smallest centroid, contiguous rows and padded views;  3  non-finite rows and centroids;  4  the f64 inertia;
  5 / 6  update: bit-exact means on integer rows with skewed sizes, empty clusters, ignored labels, views; one ulp on randn;
  7  determinism;  8  planted blobs;  9  a Lloyd trajectory against the f64 oracle step by step;  10  mauve_score;
  11  the front ends.

The shapes are the smallest that cross the edges: 128 + 2 rows, a partial third column tile, D with and without the
inner-dimension tail, a cluster longer than two 64-row segments of the update."""
import numpy as np
import pytest
import torch

import kmeans_reference as kr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEG = 64                                             # rows per segment of the update kernel (csrc/kmeans.hip: SEG_ROWS)


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


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def randn(seed, n, d):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def assign(ops, x, c):
    labels, d2, inertia = ops.kmeans_assign(x, c)
    assert labels.dtype == torch.int64 and d2.dtype == torch.float32 and inertia.dtype == torch.float64
    assert labels.is_cuda and d2.is_cuda and inertia.is_cuda
    assert tuple(labels.shape) == tuple(d2.shape) == (x.shape[0],) and inertia.dim() == 0
    return labels.cpu().numpy(), d2.cpu().numpy(), float(inertia)


def update(ops, x, labels, c_old):
    c_new, counts = ops.kmeans_update(x, labels, c_old)
    assert c_new.dtype == torch.float32 and counts.dtype == torch.int64 and c_new.is_cuda and counts.is_cuda
    assert tuple(c_new.shape) == tuple(c_old.shape) and tuple(counts.shape) == (c_old.shape[0],)
    return c_new.cpu().numpy(), counts.cpu().numpy()


def padded(a, extra, fill):
    """The same rows as a view of a wider buffer whose padding must never be read as data."""
    buf = torch.full((a.shape[0], a.shape[1] + extra), fill, dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = dev(a)
    view = buf[:, :a.shape[1]]
    assert view.stride(0) == a.shape[1] + extra
    return view


# ---------------------------------------------------------------------------------------------------- 1. the search's bits
@pytest.mark.parametrize("n,k,d", [(130, 300, 40), (130, 300, 64), (1000, 5, 64), (130, 1, 40), (130, 4000, 40)])
def test_assign_has_the_bits_of_the_search(ops, n, k, d):
    x, c = dev(randn(n + k, n, d)), dev(randn(n + k + d, k, d))
    if k == 4000:
        assert ops.knn_search_chunks(n, k, d, 1) == 32                     # the cross-chunk merge
    labels, d2, _ = assign(ops, x, c)
    want_d, want_i = ops.knn_search(x, c, 1, squared=True)
    assert np.array_equal(labels, want_i.cpu().numpy()[:, 0])
    assert np.array_equal(bits(d2), bits(want_d.cpu().numpy()[:, 0]))
    assert labels.min() >= 0 and labels.max() < k


# ---------------------------------------------------------------------------------------------------- 2. exact ties
@pytest.fixture(scope="module")
def tie_case():
    out = {}
    for d in (40, 64):
        x, c = kr.int_rows(10 + d, 130, d), kr.int_rows(20 + d, 300, d)
        c[150:200] = c[20:70]                                              # duplicated centroids, in another column tile
        c[299] = c[0]
        xi, ci = x.astype(np.int64), c.astype(np.int64)
        d2 = (xi * xi).sum(1)[:, None] + (ci * ci).sum(1)[None, :] - 2 * xi @ ci.T
        out[d] = (x, c, d2)
    return out


@pytest.mark.parametrize("d", [40, 64])
def test_exact_ties_go_to_the_smallest_centroid(ops, tie_case, d):
    x, c, d2 = tie_case[d]
    assert d2.max() < 2 ** 24
    want = np.argmin(d2, axis=1)                                           # numpy: the first minimum
    assert sum((row == row.min()).sum() > 1 for row in d2) > 10            # the data does tie
    for xt, ct in ((dev(x), dev(c)), (padded(x, 8, 1e30), padded(c, 24, 1e30))):
        labels, got, inertia = assign(ops, xt, ct)
        assert np.array_equal(labels, want)
        assert np.array_equal(bits(got), bits(d2[np.arange(len(x)), want].astype(np.float32)))
        assert inertia == float(d2.min(axis=1).sum())                      # integers: exact in every order


def test_ties_across_column_chunks(ops):
    x, c = kr.int_rows(31, 130, 40), kr.int_rows(32, 4000, 40)
    c[3000:3100] = c[100:200]                                              # duplicates in a later chunk must lose
    xi, ci = x.astype(np.int64), c.astype(np.int64)
    d2 = (xi * xi).sum(1)[:, None] + (ci * ci).sum(1)[None, :] - 2 * xi @ ci.T
    labels, got, _ = assign(ops, dev(x), dev(c))
    assert np.array_equal(labels, np.argmin(d2, axis=1))
    assert np.array_equal(bits(got), bits(d2.min(axis=1).astype(np.float32)))


# ---------------------------------------------------------------------------------------------------- 3. non-finite values
def test_non_finite_rows_and_centroids(ops):
    n, k, d = 257, 300, 40
    x, c = randn(11, n, d), randn(12, k, d)
    clean_l, clean_d, _ = assign(ops, dev(x), dev(c))
    xb = x.copy()
    xb[130, 3] = np.nan
    xb[200, 0] = np.inf
    xb[5, 39] = -np.inf
    bad = [5, 130, 200]
    labels, d2, inertia = assign(ops, dev(xb), dev(c))
    assert np.all(labels[bad] == -1) and np.all(np.isposinf(d2[bad]))
    good = np.ones(n, dtype=bool)
    good[bad] = False
    assert np.array_equal(labels[good], clean_l[good]) and np.array_equal(bits(d2[good]), bits(clean_d[good]))
    want = float(d2[good].astype(np.float64).sum())
    assert np.isfinite(inertia) and abs(inertia - want) <= 1e-12 * want    # such rows are left out
    # a non-finite centroid is nobody's label
    victim = int(np.bincount(clean_l).argmax())
    cb = c.copy()
    cb[victim, 7] = np.nan
    cb[(victim + 1) % k, 0] = np.inf
    labels, d2, _ = assign(ops, dev(x), dev(cb))
    assert not np.any(labels == victim) and not np.any(labels == (victim + 1) % k) and labels.min() >= 0
    keep = (clean_l != victim) & (clean_l != (victim + 1) % k)
    assert keep.sum() > n // 2
    assert np.array_equal(labels[keep], clean_l[keep]) and np.array_equal(bits(d2[keep]), bits(clean_d[keep]))
    # no finite centroid at all
    labels, d2, inertia = assign(ops, dev(x[:130]), dev(np.full((1, d), np.nan, dtype=np.float32)))
    assert np.all(labels == -1) and np.all(np.isposinf(d2)) and inertia == 0.0


# ---------------------------------------------------------------------------------------------------- 4. inertia
@pytest.mark.parametrize("n,k,d", [(130, 300, 40), (1000, 20, 64)])
def test_inertia_is_the_f64_sum_of_the_distances(ops, n, k, d):
    x, c = dev(randn(40 + n, n, d)), dev(randn(41 + n, k, d))
    _, d2, inertia = assign(ops, x, c)
    want = float(d2.astype(np.float64).sum())
    print("inertia", inertia, "numpy", want, "relative difference", abs(inertia - want) / want)
    assert abs(inertia - want) <= 1e-12 * want
    again = ops.kmeans_assign(x, c)[2]
    assert np.float64(inertia).view(np.uint64) == np.float64(float(again)).view(np.uint64)


# ---------------------------------------------------------------------------------------------------- 5. update, exact
def skewed_labels(seed, n, sizes):
    """Labels with the given cluster sizes, scattered over the rows (the update sorts them itself)."""
    labels = np.concatenate([np.full(s, k, dtype=np.int64) for k, s in enumerate(sizes)])
    assert len(labels) == n
    return np.random.default_rng(seed).permutation(labels)


def exact_update(x, labels, c_old):
    want, counts = kr.update(x, labels, c_old)
    out = want.astype(np.float32)
    out[counts == 0] = c_old[counts == 0]
    return out, counts


def test_update_exact_on_skewed_clusters(ops):
    n, d, sizes = 5000, 40, (4990, 9, 1)
    assert sizes[0] > 2 * SEG + 1                                          # the big cluster crosses many segments
    x = kr.int_rows(50, n, d)
    labels = skewed_labels(51, n, sizes)
    c_old = randn(52, 3, d)
    want, counts = exact_update(x, labels, c_old)
    for xt, ct in ((dev(x), dev(c_old)), (padded(x, 8, 1e30), padded(c_old, 12, 1e30))):
        got, got_counts = update(ops, xt, dev(labels), ct)
        assert np.array_equal(got_counts, counts) and list(counts) == list(sizes)
        assert np.array_equal(bits(got), bits(want))


def test_update_empty_clusters_and_ignored_labels(ops):
    n, d, k = 1000, 41, 7                                                  # D % 4 != 0: the last float4 of a row is partial
    x = kr.int_rows(53, n, d)
    labels = skewed_labels(54, n, (0, 300, 0, 63, 65, 572, 0))             # empty first, middle and last clusters
    labels[np.random.default_rng(55).choice(n, 37, replace=False)] = -1
    c_old = randn(56, k, d)
    c_old[2, 5] = np.float32(np.nan)                                       # an empty cluster keeps its bits, whatever they are
    want, counts = exact_update(x, labels, c_old)
    got, got_counts = update(ops, dev(x), dev(labels), dev(c_old))
    assert np.array_equal(got_counts, counts) and counts.sum() == n - 37 and list(counts[[0, 2, 6]]) == [0, 0, 0]
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(got[[0, 2, 6]]), bits(c_old[[0, 2, 6]]))
    # every row ignored: nothing but copies
    got, got_counts = update(ops, dev(x), dev(np.full(n, -1, dtype=np.int64)), dev(c_old))
    assert np.array_equal(bits(got), bits(c_old)) and not got_counts.any()
    # one cluster that is everything, a row count that is no multiple of the segment
    got, got_counts = update(ops, dev(x[:130]), dev(np.zeros(130, dtype=np.int64)), dev(c_old[:1]))
    assert np.array_equal(bits(got), bits((x[:130].astype(np.float64).sum(0) / 130).astype(np.float32)[None])) and got_counts[0] == 130


# ---------------------------------------------------------------------------------------------------- 6. update, randn
def test_update_is_within_one_ulp_of_the_f64_mean(ops):
    n, d, k = 1000, 64, 20
    x = randn(60, n, d)
    labels = np.random.default_rng(61).integers(0, k, n)
    want, counts = kr.update(x, labels, np.zeros((k, d)))
    got, got_counts = update(ops, dev(x), dev(labels), dev(np.zeros((k, d), dtype=np.float32)))
    assert np.array_equal(got_counts, counts) and counts.min() > 0
    err = np.abs(got.astype(np.float64) - want) / kr.ulp32(want)
    print("largest error in ulp", err.max())
    assert err.max() <= 1.0


# ---------------------------------------------------------------------------------------------------- 7. determinism
def test_two_calls_give_equal_tensors(am, ops):
    x, c = dev(kr.int_rows(12, 130, 40)), dev(kr.int_rows(13, 4000, 40))   # ties across chunks
    a, b = ops.kmeans_assign(x, c), ops.kmeans_assign(x, c)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert torch.equal(a[2].view(torch.int64), b[2].view(torch.int64))
    y = dev(randn(70, 5000, 40))
    labels = dev(skewed_labels(71, 5000, (4990, 9, 1)))
    c0 = dev(randn(72, 3, 40))
    a, b = ops.kmeans_update(y, labels, c0), ops.kmeans_update(y, labels, c0)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    z = dev(randn(73, 1000, 64))
    a, b = am.kmeans(z, 20, max_iter=10, seed=3), am.kmeans(z, 20, max_iter=10, seed=3)
    assert torch.equal(a["centroids"].view(torch.int32), b["centroids"].view(torch.int32))
    assert torch.equal(a["labels"], b["labels"]) and torch.equal(a["counts"], b["counts"])
    assert a["inertia_history"] == b["inertia_history"] and a["n_iter"] == b["n_iter"] and a["converged"] == b["converged"]
    other = am.kmeans(z, 20, max_iter=10, seed=4)
    assert not torch.equal(a["centroids"], other["centroids"])             # the seed does draw the start


# ---------------------------------------------------------------------------------------------------- 8. planted blobs
def blobs(seed, per_blob, d, centres):
    """Unit Gaussian blobs around `centres`, rows interleaved (row i belongs to blob i % len(centres))."""
    rng = np.random.default_rng(seed)
    nb = len(centres)
    x = rng.standard_normal((per_blob * nb, d)) + np.asarray(centres)[np.arange(per_blob * nb) % nb]
    return x.astype(np.float32), np.arange(per_blob * nb) % nb


def test_planted_blobs(am):
    d, nb = 40, 4
    centres = np.zeros((nb, d))
    centres[np.arange(nb), np.arange(nb)] = 20.0 / np.sqrt(2.0)            # every pair of centres 20 sigma apart
    x, planted = blobs(80, 250, d, centres)
    run = am.kmeans(dev(x), nb, init=dev(x[:nb]))                          # one row per blob
    assert run["converged"] and run["n_iter"] <= 3 and len(run["inertia_history"]) == run["n_iter"]
    assert np.array_equal(run["labels"].cpu().numpy(), planted)
    assert list(run["counts"].cpu().numpy()) == [250] * nb
    want, _ = kr.update(x, planted, np.zeros((nb, d)))
    got = run["centroids"].cpu().numpy()
    assert np.all(np.abs(got.astype(np.float64) - want) <= kr.ulp32(want))
    # inertia: every row's distance is within b = (2 D + 4) 2^-24 (|x|^2 + |c|^2) of its f64 value
    d2 = kr.sq_distances(x, got)[np.arange(len(x)), planted]
    bound = kr.rounding_bound(x, got, d)[np.arange(len(x)), planted].sum()
    print("inertia", run["inertia"], "f64", d2.sum(), "bound", bound)
    assert abs(run["inertia"] - d2.sum()) <= bound
    assert run["inertia"] == run["inertia_history"][-1]


# ---------------------------------------------------------------------------------------------------- 9. a trajectory
def test_trajectory_against_the_f64_oracle(am, ops):
    n, d, k, steps = 1000, 64, 20, 12
    x = randn(21, n, d)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(21)
    start = x[torch.randperm(n, generator=gen)[:k].numpy()]
    xt, c = dev(x), dev(start)
    history, slack = [], []
    for step in range(steps):
        labels, d2, inertia = assign(ops, xt, c)
        c_host = c.cpu().numpy()                                           # the GPU's centroids go to the oracle
        want_l, want_d, gap, _ = kr.assign(x, c_host)
        b = kr.rounding_bound(x, c_host, d)
        decided = gap > 2.0 * b.max(axis=1)
        excluded = n - int(decided.sum())
        print("step", step, "excluded rows", excluded, "inertia", inertia)
        assert excluded <= n // 100                                        # a condition of the test, not a measurement
        assert np.array_equal(labels[decided], want_l[decided])
        assert np.all(np.abs(d2 - kr.sq_distances(x, c_host)[np.arange(n), labels]) <= b[np.arange(n), labels])
        history.append(inertia)
        slack.append(float(b[np.arange(n), labels].sum()))
        c = ops.kmeans_update(xt, dev(labels), c)[0]
    for step in range(1, steps):
        assert history[step] <= history[step - 1] + slack[step], (step, history)
    assert history[-1] < 0.99 * history[0]                                 # and it does descend
    # kmeans() walks the same trajectory: same start, same number of assigns
    run = am.kmeans(xt, k, max_iter=steps - 1, init=dev(start))
    assert run["inertia_history"] == history[:len(run["inertia_history"])]
    assert len(run["inertia_history"]) == (run["n_iter"] if run["converged"] else run["n_iter"] + 1)
    seeded = am.kmeans(xt, k, max_iter=steps - 1, seed=21)                 # the seeded start is that permutation
    assert seeded["inertia_history"] == run["inertia_history"]


# ---------------------------------------------------------------------------------------------------- 10. mauve_score
def stored(am, rows):
    s = am.AudioMetricsData(True)
    for i in range(0, len(rows), 96):
        s.add(dev(rows[i:i + 96]))
    return s


def test_mauve_score(am):
    d = 40
    centres = np.zeros((4, d))
    centres[np.arange(4), np.arange(4)] = 20.0 / np.sqrt(2.0)
    a, _ = blobs(90, 100, d, centres)
    b, _ = blobs(91, 100, d, centres)
    shifted, _ = blobs(92, 100, d, centres + 5.0)
    sa, sb, sc = stored(am, a), stored(am, b), stored(am, shifted)
    same = am.mauve_score(sa, stored(am, a.copy()))
    assert same["mauve"] == 1.0 and same["mauve_n_clusters"] == 40        # max(2, min(n, m) // 10)
    near = am.mauve_score(sa, sb, return_details=True)
    far = am.mauve_score(sa, sc)
    print("same mixture", near["mauve"], "shifted mixture", far["mauve"])
    assert 0.0 < far["mauve"] < near["mauve"] <= 1.0
    assert sorted(far) == ["mauve", "mauve_kmeans_inertia", "mauve_kmeans_iterations", "mauve_n_clusters"]
    hc, hr = near["mauve_hist_candidate"], near["mauve_hist_reference"]
    assert hc.sum() == len(a) and hr.sum() == len(b) and hc.shape == hr.shape == (40,)
    assert near["mauve"] == am.mauve_from_histograms(hc, hr)
    assert np.array_equal(hc, np.bincount(near["mauve_labels_candidate"].cpu().numpy(), minlength=40))
    assert np.array_equal(hr, np.bincount(near["mauve_labels_reference"].cpu().numpy(), minlength=40))
    assert near["mauve_points"].shape == (27, 2) and near["mauve_kmeans_iterations"] >= 1
    few = am.mauve_score(sa, sb, n_clusters=4, seed=1)
    assert few["mauve_n_clusters"] == 4 and 0.0 < few["mauve"] <= 1.0


# ---------------------------------------------------------------------------------------------------- 11. front ends
def test_front_ends(am):
    x = randn(95, 700, 40)
    a = am.kmeans(stored(am, x), 12, max_iter=8, seed=5)
    b = am.kmeans(dev(x), 12, max_iter=8, seed=5)
    assert torch.equal(a["centroids"].view(torch.int32), b["centroids"].view(torch.int32)) and torch.equal(a["labels"], b["labels"])
    assert a["inertia_history"] == b["inertia_history"]
    assert sorted(a) == ["centroids", "converged", "counts", "inertia", "inertia_history", "labels", "n_iter"]
    assert a["centroids"].is_cuda and a["labels"].is_cuda and isinstance(a["inertia"], float)
    assert int(a["counts"].sum()) == 700 and torch.equal(a["counts"], torch.bincount(a["labels"], minlength=12))
    singles = [am.kmeans(dev(x), 12, max_iter=8, seed=5 + r)["inertia"] for r in range(3)]
    best = am.kmeans(dev(x), 12, max_iter=8, seed=5, n_init=3)
    assert best["inertia"] == min(singles) and len(set(singles)) > 1
