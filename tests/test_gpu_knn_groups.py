"""The leave-group-out nearest-neighbour search on the device (hip_ops.knn_search_groups) and what stands on it
(nearest_neighbors(groups=...), nearest_neighbor_two_sample_test).

  1  bit-exact distances AND indices on exactly representable data with many ties, labels that straddle row blocks, 32-column
     sub-tiles and the 128-column tile edge, every side of the list-length boundaries, contiguous rows and row views;
  2  the same through more than one column chunk, with a label so common that its rows run out of admissible columns;
  3  equivalences with the plain search, bit for bit, and independence of the stored order;
  4  real-valued windowed rows: siblings without labels, none with them, indices right within the derived rounding bound;
  5  non-finite rows, determinism;  6  the front ends."""
import warnings

import numpy as np
import pytest
import torch

import nn_test_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KS = (1, 5, 8, 9, 16, 17, 32)                        # both sides of the 8 / 16 / 32 list lengths


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


def labels(a):
    return dev(np.asarray(a, dtype=np.int32))


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def search(ops, x, y, k, gx, gy, **kw):
    dist, idx = ops.knn_search_groups(x, y, k, gx, gy, **kw)
    assert dist.dtype == torch.float32 and idx.dtype == torch.int64 and dist.is_cuda and idx.is_cuda
    assert tuple(dist.shape) == tuple(idx.shape) == (x.shape[0], k)
    return dist.cpu().numpy(), idx.cpu().numpy()


def plain(ops, x, y, k, **kw):
    dist, idx = ops.knn_search(x, y, k, **kw)
    return dist.cpu().numpy(), idx.cpu().numpy()


def int_rows(seed, n, d):
    return np.random.default_rng(seed).integers(-3, 4, size=(n, d)).astype(np.float32)


def int_oracle(x, y, gx, gy):
    """int64 squared distances (exact: every value is an integer below 2^24), the order by (d2, column) with the columns of
    the row's own label moved behind all others, and the number of admissible columns of every row"""
    xi, yi = x.astype(np.int64), y.astype(np.int64)
    d2 = (xi * xi).sum(1)[:, None] + (yi * yi).sum(1)[None, :] - 2 * xi @ yi.T
    order = np.empty_like(d2)
    cols = np.arange(d2.shape[1])
    valid = np.empty(len(d2), dtype=np.int64)
    for i in range(len(d2)):
        o = np.lexsort((cols, d2[i]))
        own = gy[o] == gx[i]
        order[i] = np.concatenate([o[~own], o[own]])
        valid[i] = (~own).sum()
    return d2, order, valid


def check_exact(got_d, got_i, d2, order, valid, k):
    for i in range(len(d2)):
        kk = min(k, int(valid[i]))
        want_i = order[i, :kk]
        assert np.array_equal(got_i[i, :kk], want_i), i
        assert np.array_equal(bits(got_d[i, :kk]), bits(d2[i, want_i].astype(np.float32))), i
        assert np.all(got_i[i, kk:] == -1) and np.all(np.isposinf(got_d[i, kk:])), i


# ---------------------------------------------------------------------------------------------------- 1. exact data, ties
@pytest.fixture(scope="module")
def exact_case():
    out = {}
    for d in (40, 64):
        rng = np.random.default_rng(d)
        x, y = int_rows(10 + d, 130, d), int_rows(20 + d, 300, d)
        gx, gy = rng.integers(0, 7, 130) * 1000 - 3000, rng.integers(0, 7, 300) * 1000 - 3000      # any int32 values
        out[d] = (x, y, gx, gy) + int_oracle(x, y, gx, gy)
    return out


@pytest.mark.parametrize("d", [40, 64])
def test_exact_distances_and_indices_with_ties(ops, exact_case, d):
    x, y, gx, gy, d2, order, valid = exact_case[d]
    assert d2.max() < 2 ** 24
    assert sum(len(np.unique(row)) < len(row) for row in np.sort(d2, axis=1)[:, :32]) > 100        # full of ties
    # every label has columns in every 32-column sub-tile's neighbourhood and on both sides of the 128-column tile edges
    assert all(len(np.unique(gy[s:s + 32])) > 3 for s in range(0, 288, 32)) and len(np.unique(gx[:128])) == 7 and len(set(gx[128:])) > 1
    xt, yt, gxt, gyt = dev(x), dev(y), labels(gx), labels(gy)
    for k in KS:
        got_d, got_i = search(ops, xt, yt, k, gxt, gyt, squared=True)
        check_exact(got_d, got_i, d2, order, valid, k)
        assert not np.any((got_i >= 0) & (gy[np.maximum(got_i, 0)] == gx[:, None]))


@pytest.mark.parametrize("d", [40, 64])
def test_exact_on_row_views(ops, exact_case, d):
    x, y, gx, gy, d2, order, valid = exact_case[d]
    bx = torch.full((130, d + 8), 1e30, dtype=torch.float32, device=DEV)              # the padding must never be read as data
    by = torch.full((300, d + 24), -1e30, dtype=torch.float32, device=DEV)
    bx[:, :d], by[:, :d] = dev(x), dev(y)
    xt, yt = bx[:, :d], by[:, :d]
    assert xt.stride(0) == d + 8 and yt.stride(0) == d + 24
    gxt, gyt = labels(gx), labels(gy)
    for k in KS:
        got_d, got_i = search(ops, xt, yt, k, gxt, gyt, squared=True)
        check_exact(got_d, got_i, d2, order, valid, k)


# ---------------------------------------------------------------------------------------------------- 2. several column chunks
def test_more_than_one_column_chunk_and_a_label_that_runs_out(ops):
    n, m, d = 130, 4000, 40
    chunks = ops.knn_search_chunks(n, m, d, 5)
    assert chunks > 1
    x, y = int_rows(31, n, d), int_rows(32, m, d)
    # label 0 holds all columns but every 200th: its columns lie in every chunk, and a row of label 0 has 20 admissible columns
    gy = np.zeros(m, dtype=np.int64)
    rare = np.arange(7, m, 200)
    gy[rare] = 1 + (rare // 200) % 3
    gx = np.random.default_rng(33).integers(0, 4, n)
    per_chunk = m // chunks
    assert all((gy[c * per_chunk:(c + 1) * per_chunk] == 0).any() for c in range(chunks)) and len(rare) == 20
    d2, order, valid = int_oracle(x, y, gx, gy)
    assert set(valid[gx == 0]) == {20} and (gx == 0).sum() > 10 and valid[gx != 0].min() > 3900
    xt, yt, gxt, gyt = dev(x), dev(y), labels(gx), labels(gy)
    for k in KS:
        assert ops.knn_search_chunks(n, m, d, k) > 1
        got_d, got_i = search(ops, xt, yt, k, gxt, gyt, squared=True)
        check_exact(got_d, got_i, d2, order, valid, k)
    tail = got_i[gx == 0]                                                  # k = 32: 20 neighbours, then 12 x (+inf, -1)
    assert np.all(tail[:, :20] >= 0) and np.all(tail[:, 20:] == -1)


# ---------------------------------------------------------------------------------------------------- 3. equivalences
def test_equivalences_with_the_plain_search(ops):
    x, y = int_rows(41, 300, 40), int_rows(42, 700, 40)
    xt, yt = dev(x), dev(y)
    own = labels(np.arange(300))
    for k in (1, 5, 17):
        # every row its own label, a set against itself: the row itself is skipped, by index
        got, want = search(ops, xt, xt, k, own, own, squared=True), plain(ops, xt, xt, k, self_offset=0, squared=True)
        assert np.array_equal(got[1], want[1]) and np.array_equal(bits(got[0]), bits(want[0]))
        # disjoint label ranges: nothing is skipped
        got, want = search(ops, xt, yt, k, labels(np.arange(300) % 9), labels(100 + np.arange(700) % 11)), plain(ops, xt, yt, k)
        assert np.array_equal(got[1], want[1]) and np.array_equal(bits(got[0]), bits(want[0]))
        # one label on everything: nobody has a neighbour
        got = search(ops, xt, yt, k, labels(np.full(300, -5)), labels(np.full(700, -5)))
        assert np.all(got[1] == -1) and np.all(np.isposinf(got[0]))


def song_windows(seed, songs, d, windows=16, spread=0.3):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((songs, d))
    rows = np.repeat(centres, windows, axis=0) + spread * rng.standard_normal((songs * windows, d))
    return rows.astype(np.float32), np.repeat(np.arange(songs), windows)


def test_stored_order_does_not_matter(ops):
    """labels in runs of 16 against the same rows and labels under a seeded permutation: the same neighbours"""
    x, g = song_windows(51, 20, 64)
    k = 5
    run_d, run_i = search(ops, dev(x), dev(x), k, labels(g), labels(g), squared=True)
    assert np.all(np.diff(run_d, axis=1) > 0)                              # tie-free: the k nearest are one well-defined list
    perm = np.random.default_rng(52).permutation(len(x))
    mix_d, mix_i = search(ops, dev(x[perm]), dev(x[perm]), k, labels(g[perm]), labels(g[perm]), squared=True)
    assert np.array_equal(perm[mix_i], run_i[perm]) and np.array_equal(bits(mix_d), bits(run_d[perm]))


# ---------------------------------------------------------------------------------------------------- 4. windowed rows
def check_within_rounding(x, y, gx, gy, got_d, got_i, d):
    """every reported pair and every admissible column that is not reported, against float64, within the worst case of an f32
    fmaf chain of D terms under the factor 2 plus the two norm sums (test_gpu_knn_search.py): derived, not tuned"""
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    nx, ny = (x64 * x64).sum(1), (y64 * y64).sum(1)
    d2 = np.maximum(nx[:, None] + ny[None, :] - 2.0 * x64 @ y64.T, 0.0)
    tol = (2 * d + 4) * 2.0 ** -24 * (nx[:, None] + ny[None, :])
    assert got_i.min() >= 0 and got_i.max() < len(y)
    assert not np.any(gy[got_i] == gx[:, None])                            # never a row of the own group
    true = np.take_along_axis(d2, got_i, axis=1)
    assert np.all(np.abs(true - got_d) <= np.take_along_axis(tol, got_i, axis=1))
    assert np.all(np.diff(got_d, axis=1) >= 0) and all(len(set(row)) == got_i.shape[1] for row in got_i)
    rest = d2.copy()
    np.put_along_axis(rest, got_i, np.inf, axis=1)
    rest[gx[:, None] == gy[None, :]] = np.inf                              # the own group is not a candidate
    assert np.all(rest >= got_d[:, -1:].astype(np.float64) - 2.0 * tol)


def test_windows_choose_siblings_unless_the_song_is_left_out(ops):
    d = 64
    x, g = song_windows(61, 20, d)
    xt, gt = dev(x), labels(g)
    _, row_only = plain(ops, xt, xt, 1, self_offset=0)
    assert np.mean(g[row_only[:, 0]] == g) > 0.9                           # the nearest neighbour is a sibling window
    for k in (1, 5, 17):
        got_d, got_i = search(ops, xt, xt, k, gt, gt, squared=True)
        check_within_rounding(x, x, g, g, got_d, got_i, d)                  # ... and with labels it never is


def test_wide_rows_within_rounding(ops):
    d = 512
    y, gy = song_windows(62, 63, d)
    y, gy = y[:1000], gy[:1000]
    rng = np.random.default_rng(63)
    gx = np.repeat(np.arange(19), 16)[:300]                                # further windows of the first 19 songs of y
    centres = np.stack([y[gy == s].mean(axis=0) for s in range(19)])
    x = (centres[gx] + 0.3 * rng.standard_normal((300, d))).astype(np.float32)
    _, unlabelled = plain(ops, dev(x), dev(y), 1)
    assert np.mean(gy[unlabelled[:, 0]] == gx) > 0.9
    got_d, got_i = search(ops, dev(x), dev(y), 5, labels(gx), labels(gy), squared=True)
    check_within_rounding(x, y, gx, gy, got_d, got_i, d)


# ---------------------------------------------------------------------------------------------------- 5. non-finite, determinism
def test_non_finite_rows(ops):
    n, m, d, k = 257, 700, 40, 5
    rng = np.random.default_rng(11)
    x, y = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((m, d)).astype(np.float32)
    gx, gy = rng.integers(0, 9, n), rng.integers(0, 9, m)
    gxt, gyt = labels(gx), labels(gy)
    clean_d, clean_i = search(ops, dev(x), dev(y), k, gxt, gyt)
    victim = int(clean_i[0, 0])                                            # somebody's nearest neighbour
    yb = y.copy()
    yb[victim, 7] = np.nan
    xb = x.copy()
    xb[130, 3] = np.nan
    xb[200, 0] = np.inf
    got_d, got_i = search(ops, dev(xb), dev(yb), k, gxt, gyt)
    assert not np.any(got_i == victim)                                     # a NaN row of y is never reported
    for bad in (130, 200):                                                 # a non-finite row of x has no neighbours
        assert np.all(got_i[bad] == -1) and np.all(np.isposinf(got_d[bad]))
    same = np.ones(n, dtype=bool)
    same[[130, 200]] = False
    same &= ~np.any(clean_i == victim, axis=1)
    assert same.sum() > n // 2
    assert np.array_equal(got_i[same], clean_i[same]) and np.array_equal(bits(got_d[same]), bits(clean_d[same]))
    lost = np.any(clean_i == victim, axis=1)                               # the rows that lost the victim: the clean k + 1 list without it
    lost[[130, 200]] = False
    wide_d, wide_i = search(ops, dev(x), dev(y), k + 1, gxt, gyt)
    for i in np.flatnonzero(lost):
        keep = wide_i[i] != victim
        assert np.array_equal(got_i[i], wide_i[i][keep][:k]) and np.array_equal(bits(got_d[i]), bits(wide_d[i][keep][:k]))


def test_two_calls_give_equal_tensors(ops):
    x, y = dev(int_rows(12, 130, 40)), dev(int_rows(13, 4000, 40))         # ties across chunks
    gx, gy = labels(np.arange(130) % 5), labels(np.arange(4000) % 7)
    a, b = ops.knn_search_groups(x, y, 9, gx, gy), ops.knn_search_groups(x, y, 9, gx, gy)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------- 6. front ends
def stored(am, rows):
    s = am.AudioMetricsData(True)
    for lo in range(0, len(rows), 32):                                     # 32-row adds, like the embedding pipeline
        s.add(dev(rows[lo:lo + 32]))
    return s


def test_nearest_neighbors_with_groups(am, ops):
    x, gx = song_windows(71, 17, 40)
    y, gy = song_windows(72, 30, 40)
    gx, gy = 5 * gx - 20, 5 * gy - 20                                      # compared by VALUE across the sets: 5 * 4 - 20 = 0 meets 0
    a, b = stored(am, x[:257]), stored(am, y)
    gx = gx[:257]
    res = am.nearest_neighbors(a, b, k=5, groups=gx, searched_groups=dev(gy))       # host and device labels
    assert sorted(res) == ["nn_distances", "nn_indices"]
    want_d, want_i = search(ops, dev(x[:257]), dev(y), 5, labels(gx), labels(gy))
    assert res["nn_distances"].dtype == np.float32 and res["nn_indices"].dtype == np.int64
    assert np.array_equal(res["nn_indices"], want_i) and np.array_equal(bits(res["nn_distances"]), bits(want_d))
    own = am.nearest_neighbors(a, a, k=3, groups=gx, squared=True)
    want_d, want_i = search(ops, dev(x[:257]), dev(x[:257]), 3, labels(gx), labels(gx), squared=True)
    assert np.array_equal(own["nn_indices"], want_i) and np.array_equal(bits(own["nn_distances"]), bits(want_d))
    assert not np.any(gx[own["nn_indices"]] == gx[:, None])


def integer_songs(seed, songs, d=8, windows=8, shift=0):
    rng = np.random.default_rng(seed)
    centres = rng.integers(-3, 4, size=(songs, d)) + shift
    rows = np.repeat(centres, windows, axis=0) + rng.integers(-1, 2, size=(songs * windows, d))
    return rows.astype(np.float32), np.repeat(np.arange(songs), windows) * 3 + 100


def same_value(got, want):
    if isinstance(want, np.ndarray):
        return np.array_equal(got, want, equal_nan=True) and got.dtype == want.dtype
    return got == want or (want != want and got != got)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("labelled", [True, False])
def test_two_sample_test_equals_the_reference(am, k, labelled):
    x, gx = integer_songs(81, 12)
    y, gy = integer_songs(82, 10)
    a, b = stored(am, x), stored(am, y)
    kw = dict(groups=gx, ref_groups=gy) if labelled else {}
    got = am.nearest_neighbor_two_sample_test(a, b, k=k, n_permutations=99, seed=5, return_rows=True, **kw)
    want = ref.two_sample_test(x, y, k=k, n_permutations=99, seed=5, **kw)
    assert sorted(got) == sorted(want)
    for key in want:
        assert same_value(got[key], want[key]), (key, got[key], want[key])
    assert got["nn_units"] == ((12, 10) if labelled else (96, 80)) and got["nn_rows_nonfinite"] == 0
    short = am.nearest_neighbor_two_sample_test(a, b, k=k, n_permutations=99, seed=5, **kw)
    assert sorted(short) == sorted(key for key in want if key.startswith("nn_")) and all(same_value(short[key], want[key]) for key in short)


def test_four_searches_give_the_graph_of_one_pooled_search(am, ops):
    x, gx = integer_songs(83, 12)
    y, gy = integer_songs(84, 10)
    got = am.nearest_neighbor_two_sample_test(stored(am, x), stored(am, y), groups=gx, ref_groups=gy, k=3, n_permutations=9,
                                              return_rows=True)
    unit, _ = ref.pooled_units(len(x), len(y), gx, gy)                       # joint labels: the two sides' units kept apart
    pooled = dev(np.concatenate([x, y]))
    _, want = search(ops, pooled, pooled, 3, labels(unit), labels(unit))
    assert np.array_equal(np.concatenate([got["candidate_neighbors"], got["reference_neighbors"]]), want)


def test_shifted_pair_and_non_finite_rows(am):
    x, gx = integer_songs(85, 12, shift=40)
    y, gy = integer_songs(86, 10)
    a, b = stored(am, x), stored(am, y)
    got = am.nearest_neighbor_two_sample_test(a, b, groups=gx, ref_groups=gy, n_permutations=99)
    assert got["nn_accuracy"] == 1.0 and got["nn_p_value"] == 1.0 / 100.0
    xb = x.copy()
    xb[5, 2] = np.nan
    xb[40, 0] = np.inf
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        bad = am.nearest_neighbor_two_sample_test(stored(am, xb), b, groups=gx, ref_groups=gy, n_permutations=99, return_rows=True)
    assert [w.category for w in caught] == [RuntimeWarning] and "2 row(s)" in str(caught[0].message)
    want = ref.two_sample_test(xb, y, groups=gx, ref_groups=gy, n_permutations=99)
    assert bad["nn_rows_nonfinite"] == 2 and all(same_value(bad[key], want[key]) for key in want)
    assert np.all(bad["candidate_neighbors"][[5, 40]] == -1) and np.isnan(bad["candidate_same_share"][[5, 40]]).all()
