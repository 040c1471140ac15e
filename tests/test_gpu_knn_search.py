"""Exact k-nearest-neighbour search on the device (hip_ops.knn_search, nearest_neighbors).

  1  bit-exact distances AND indices on exactly representable data with many ties (the smallest-column rule), every side of
     the list-length boundaries, contiguous rows and row views;
  2  the same through more than one column chunk (the merge kernel; ties do not depend on the chunking);
  3  the same bits as the radii: the C model of the exact kernel and hip_ops.knn_radii;
  4  indices on real-valued rows without assuming an order inside the rounding of the f32 arithmetic;
  5  self exclusion by index (duplicates stay, shards);  6  too few neighbours, non-finite rows;  7  determinism and API."""
import numpy as np
import pytest
import torch

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


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def search(ops, x, y, k, **kw):
    dist, idx = ops.knn_search(x, y, k, **kw)
    assert dist.dtype == torch.float32 and idx.dtype == torch.int64 and dist.is_cuda and idx.is_cuda
    assert tuple(dist.shape) == tuple(idx.shape) == (x.shape[0], k)
    return dist.cpu().numpy(), idx.cpu().numpy()


def int_rows(seed, n, d):
    return np.random.default_rng(seed).integers(-3, 4, size=(n, d)).astype(np.float32)


def int_oracle(x, y, self_offset=None):
    """int64 squared distances (exact: every value is an integer below 2^24) and the order by (d2, column)."""
    xi, yi = x.astype(np.int64), y.astype(np.int64)
    d2 = (xi * xi).sum(1)[:, None] + (yi * yi).sum(1)[None, :] - 2 * xi @ yi.T
    order = np.empty_like(d2)
    cols = np.arange(d2.shape[1])
    for i in range(len(d2)):
        o = np.lexsort((cols, d2[i]))
        if self_offset is not None:
            o = np.concatenate([o[o != i + self_offset], o[o == i + self_offset]])     # the row itself goes last
        order[i] = o
    return d2, order


def check_exact(got_d, got_i, d2, order, k, n_valid=None):
    n, m = d2.shape
    n_valid = m if n_valid is None else n_valid
    kk = min(k, n_valid)
    want_i = order[:, :kk]
    want_d = np.take_along_axis(d2, want_i, axis=1).astype(np.float32)
    assert np.array_equal(got_i[:, :kk], want_i)
    assert np.array_equal(bits(got_d[:, :kk]), bits(want_d))
    assert np.all(got_i[:, kk:] == -1) and np.all(np.isposinf(got_d[:, kk:]))


# ---------------------------------------------------------------------------------------------------- 1. exact data, ties
@pytest.fixture(scope="module")
def exact_case():
    out = {}
    for d in (40, 64):
        x, y = int_rows(10 + d, 130, d), int_rows(20 + d, 300, d)
        out[d] = (x, y) + int_oracle(x, y)
    return out


@pytest.mark.parametrize("d", [40, 64])
def test_exact_distances_and_indices_with_ties(ops, exact_case, d):
    x, y, d2, order = exact_case[d]
    assert d2.max() < 2 ** 24
    # the data is full of ties: the test pins the smallest-column rule
    assert sum(len(np.unique(row)) < len(row) for row in np.sort(d2, axis=1)[:, :32]) > 100
    xt, yt = dev(x), dev(y)
    for k in KS:
        got_d, got_i = search(ops, xt, yt, k, squared=True)
        check_exact(got_d, got_i, d2, order, k)


@pytest.mark.parametrize("d", [40, 64])
def test_exact_on_row_views(ops, exact_case, d):
    x, y, d2, order = exact_case[d]
    bx = torch.full((130, d + 8), 1e30, dtype=torch.float32, device=DEV)              # the padding must never be read as data
    by = torch.full((300, d + 24), -1e30, dtype=torch.float32, device=DEV)
    bx[:, :d], by[:, :d] = dev(x), dev(y)
    xt, yt = bx[:, :d], by[:, :d]
    assert xt.stride(0) == d + 8 and yt.stride(0) == d + 24
    for k in KS:
        got_d, got_i = search(ops, xt, yt, k, squared=True)
        check_exact(got_d, got_i, d2, order, k)


# ---------------------------------------------------------------------------------------------------- 2. several column chunks
def test_more_than_one_column_chunk(ops):
    n, m, d = 130, 4000, 40
    assert ops.knn_search_chunks(n, m, d, 5) > 1
    x, y = int_rows(31, n, d), int_rows(32, m, d)
    d2, order = int_oracle(x, y)
    xt, yt = dev(x), dev(y)
    for k in KS:
        assert ops.knn_search_chunks(n, m, d, k) > 1
        got_d, got_i = search(ops, xt, yt, k, squared=True)
        check_exact(got_d, got_i, d2, order, k)


# ---------------------------------------------------------------------------------------------------- 3 / 4. randn rows
RANDN = [(257, 700, 40), (300, 1000, 512)]


@pytest.fixture(scope="module")
def randn_case(ops):
    """Per shape: host rows, the float64 squared distances, and ONE (k = 17, squared) search shared by the tests."""
    out = {}
    for n, m, d in RANDN:
        rng = np.random.default_rng(n + m + d)
        x, y = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((m, d)).astype(np.float32)
        x64, y64 = x.astype(np.float64), y.astype(np.float64)
        nx, ny = (x64 * x64).sum(1), (y64 * y64).sum(1)
        d2 = np.maximum(nx[:, None] + ny[None, :] - 2.0 * x64 @ y64.T, 0.0)
        xt, yt = dev(x), dev(y)
        got = search(ops, xt, yt, 17, squared=True)
        out[(n, m, d)] = dict(x=x, y=y, xt=xt, yt=yt, d2=d2, nx=nx, ny=ny, got=got)
    return out


@pytest.mark.parametrize("shape", RANDN)
def test_same_bits_as_the_radii(ops, randn_case, shape):
    import oracle
    c = randn_case[shape]
    for k in (1, 5, 16):
        want_r, want_sq = oracle.exact.knn_radii(c["x"], k, columns=c["y"], return_squared=True)     # the C model
        got_sq = search(ops, c["xt"], c["yt"], k + 1, squared=True)[0][:, k]
        assert np.array_equal(bits(got_sq), bits(want_sq)), k
        assert np.array_equal(bits(c["got"][0][:, k]), bits(want_sq)), k                             # a longer list: same prefix
        got_r = search(ops, c["xt"], c["yt"], k + 1)[0][:, k]
        dev_r = ops.knn_radii(c["xt"], k, columns=c["yt"]).cpu().numpy()
        assert np.array_equal(bits(got_r), bits(dev_r)) and np.array_equal(bits(got_r), bits(want_r)), k


@pytest.mark.parametrize("shape", RANDN)
def test_indices_are_right_within_rounding(ops, randn_case, shape):
    n, m, d = shape
    c = randn_case[shape]
    # worst case of an f32 fmaf chain of D terms under the factor 2, plus the two norm sums: derived, not tuned
    tol = (2 * d + 4) * 2.0 ** -24 * (c["nx"][:, None] + c["ny"][None, :])
    for k in (1, 5, 16, 17):
        got_d, got_i = c["got"] if k == 17 else search(ops, c["xt"], c["yt"], k, squared=True)
        kk = got_d.shape[1]
        assert kk == k
        assert got_i.min() >= 0 and got_i.max() < m
        true = np.take_along_axis(c["d2"], got_i, axis=1)
        assert np.all(np.abs(true - got_d) <= np.take_along_axis(tol, got_i, axis=1))                # every reported pair
        assert np.all(np.diff(got_d, axis=1) >= 0)                                                    # non-decreasing
        assert all(len(set(row)) == kk for row in got_i)                                              # distinct
        rest = c["d2"].copy()
        np.put_along_axis(rest, got_i, np.inf, axis=1)                                                # every column NOT reported
        assert np.all(rest >= got_d[:, -1:].astype(np.float64) - 2.0 * tol)


# ---------------------------------------------------------------------------------------------------- 5. self exclusion
def test_self_exclusion_is_by_index(ops):
    n, d, k = 300, 64, 5
    x = np.random.default_rng(5).standard_normal((n, d)).astype(np.float32)
    xt = dev(x)
    ex_d, ex_i = search(ops, xt, xt, k, self_offset=0, squared=True)
    assert not np.any(ex_i == np.arange(n)[:, None])
    full_d, full_i = search(ops, xt, xt, k + 1, squared=True)
    first_is_self = full_i[:, 0] == np.arange(n)
    assert first_is_self.sum() > n // 2                                    # (not all: |x|^2 + |x|^2 - 2 x.x rounds, a neighbour may tie)
    assert np.array_equal(ex_i[first_is_self], full_i[first_is_self, 1:])
    assert np.array_equal(bits(ex_d[first_is_self]), bits(full_d[first_is_self, 1:]))
    # a shard: rows 100 .. 199 against the full set
    sh_d, sh_i = search(ops, xt[100:200], xt, k, self_offset=100, squared=True)
    assert np.array_equal(sh_i, ex_i[100:200]) and np.array_equal(bits(sh_d), bits(ex_d[100:200]))
    # an offset past the columns excludes nothing
    far_d, far_i = search(ops, xt, xt, k + 1, self_offset=n + 7, squared=True)
    assert np.array_equal(far_i, full_i) and np.array_equal(bits(far_d), bits(full_d))


def test_duplicate_rows_stay_neighbours(ops):
    n, d = 300, 64
    x = int_rows(6, n, d)
    x[250] = x[3]                                                          # an exact duplicate, in another row block
    x[17] = x[3]
    d2, order = int_oracle(x, x, self_offset=0)
    got_d, got_i = search(ops, dev(x), dev(x), 5, self_offset=0, squared=True)
    check_exact(got_d, got_i, d2, order, 5, n_valid=n - 1)
    assert list(got_i[3, :2]) == [17, 250] and list(got_d[3, :2]) == [0.0, 0.0]
    assert got_i[17, 0] == 3 and got_i[250, 0] == 3 and got_d[250, 0] == 0.0


# ---------------------------------------------------------------------------------------------------- 6. missing neighbours
def test_fewer_rows_than_k(ops):
    x, y = int_rows(7, 130, 40), int_rows(8, 3, 40)
    d2, order = int_oracle(x, y)
    got_d, got_i = search(ops, dev(x), dev(y), 5, squared=True)
    check_exact(got_d, got_i, d2, order, 5)
    assert np.all(got_i[:, 3:] == -1) and np.all(np.isposinf(got_d[:, 3:])) and np.all(got_i[:, :3] >= 0)
    # with exclusion one candidate fewer
    z = int_rows(9, 4, 40)
    d2, order = int_oracle(z, z, self_offset=0)
    got_d, got_i = search(ops, dev(z), dev(z), 5, self_offset=0)
    assert np.array_equal(got_i[:, :3], order[:, :3]) and np.all(got_i[:, 3:] == -1) and np.all(np.isposinf(got_d[:, 3:]))


def test_non_finite_rows(ops):
    n, m, d, k = 257, 700, 40, 5
    rng = np.random.default_rng(11)
    x, y = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((m, d)).astype(np.float32)
    clean_d, clean_i = search(ops, dev(x), dev(y), k)
    victim = int(clean_i[0, 0])                                            # somebody's nearest neighbour
    yb = y.copy()
    yb[victim, 7] = np.nan
    xb = x.copy()
    xb[130, 3] = np.nan
    xb[200, 0] = np.inf
    got_d, got_i = search(ops, dev(xb), dev(yb), k)
    assert not np.any(got_i == victim)                                     # a NaN row of y is never reported
    for bad in (130, 200):                                                 # a non-finite row of x has no neighbours
        assert np.all(got_i[bad] == -1) and np.all(np.isposinf(got_d[bad]))
    # rows that neither are bad nor had the victim among their neighbours: bit-identical to the clean run
    same = np.ones(n, dtype=bool)
    same[[130, 200]] = False
    same &= ~np.any(clean_i == victim, axis=1)
    assert same.sum() > n // 2
    assert np.array_equal(got_i[same], clean_i[same]) and np.array_equal(bits(got_d[same]), bits(clean_d[same]))
    # the rows that lost the victim: the clean k + 1 list without it
    lost = np.any(clean_i == victim, axis=1)
    lost[[130, 200]] = False
    wide_d, wide_i = search(ops, dev(x), dev(y), k + 1)
    for i in np.flatnonzero(lost):
        keep = wide_i[i] != victim
        assert np.array_equal(got_i[i], wide_i[i][keep][:k]) and np.array_equal(bits(got_d[i]), bits(wide_d[i][keep][:k]))


# ---------------------------------------------------------------------------------------------------- 7. determinism, API
def test_two_calls_give_equal_tensors(ops):
    x, y = dev(int_rows(12, 130, 40)), dev(int_rows(13, 4000, 40))         # ties across chunks
    a, b = ops.knn_search(x, y, 9), ops.knn_search(x, y, 9)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_nearest_neighbors_front_end(am, ops):
    rng = np.random.default_rng(14)
    x, y = rng.standard_normal((257, 40)).astype(np.float32), rng.standard_normal((700, 40)).astype(np.float32)
    a, b = am.AudioMetricsData(True), am.AudioMetricsData(True)
    for rows, dst in ((x, a), (y, b)):
        for s in range(0, len(rows), 32):                                  # 32-row adds, like the embedding pipeline
            dst.add(dev(rows[s:s + 32]))
    res = am.nearest_neighbors(a, b, k=5)
    assert sorted(res) == ["nn_distances", "nn_indices"]
    dist, idx = res["nn_distances"], res["nn_indices"]
    assert isinstance(dist, np.ndarray) and dist.dtype == np.float32 and dist.shape == (257, 5)
    assert isinstance(idx, np.ndarray) and idx.dtype == np.int64 and idx.shape == (257, 5)
    want_d, want_i = search(ops, dev(x), dev(y), 5)                        # stored order = the order of the adds
    assert np.array_equal(idx, want_i) and np.array_equal(bits(dist), bits(want_d))
    sq = am.nearest_neighbors(a, b, k=5, squared=True)
    assert np.array_equal(sq["nn_indices"], want_i)
    assert np.array_equal(bits(sq["nn_distances"]), bits(search(ops, dev(x), dev(y), 5, squared=True)[0]))
    own = am.nearest_neighbors(a, a, k=3, exclude_self=True)
    want_d, want_i = search(ops, dev(x), dev(x), 3, self_offset=0)
    assert np.array_equal(own["nn_indices"], want_i) and np.array_equal(bits(own["nn_distances"]), bits(want_d))
    assert not np.any(own["nn_indices"] == np.arange(257)[:, None])
    short = am.nearest_neighbors(b, a, k=32)["nn_indices"]
    assert short.shape == (700, 32) and short.min() >= 0
