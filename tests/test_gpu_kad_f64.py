"""Kernel Audio Distance on float64 rows (csrc/kad_f64.hip: am_pairwise_select_f64, am_mmd_rbf_f64, am_mmd_rbf_groups_f64)
against the float64 oracles of tests/kad_reference.py and tests/kad_groups_reference.py.

The exact data here is WIDE: 18-bit integers times a power of two, so a dot product adds 34-bit products.  Norms, dot
products and squared distances are exact in f64 in any order, while an f32 accumulation of them is not - the fixtures show,
on the CPU, that the emulated f32 form misses the bound of these tests by more than a factor of 100: an implementation that
narrows the rows to the f32 kernels fails.

  G1-G4  hip_ops.pairwise_select_sq on float64 rows: bit-exact on exact data (every rank kind, an odd row stride, duplicates,
         a NaN row, 64-bit counts), within the worst-case f64 summation error on real-valued rows
  G5-G6  hip_ops.mmd_rbf_sums: 1e-12 x mean |K| on exact data, same bits, device-fed bandwidth, symmetry, block mask; the f64
         summation bound on real-valued rows
  G7     hip_ops.mmd_rbf_group_sums: groups that straddle the 64-row tiles behind a permutation, list-order bits, row sums,
         the partition of the whole-set cross sum, an out-of-range index
  G8     kernel_audio_distance, kernel_audio_distance_per_group and AudioMetrics(metrics=[..., "kad"]) on float64 sets"""
import warnings

import numpy as np
import pytest
import torch

import inputs as gi
import kad_groups_reference as kg
import kad_reference as ka
import kd_reference as kr

pytestmark = pytest.mark.gpu

EXACT = 1e-12
DEV = "cuda:0"
SIGMA = 10.0
GAMMA = 1.0 / (2.0 * SIGMA * SIGMA)


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
    return np.asarray(v, dtype=np.float32).view(np.uint32)


def select(ops, xt, rank=None):
    assert xt.dtype == torch.float64
    out = ops.pairwise_select_sq(xt, rank)
    assert out.dtype == torch.float32 and out.dim() == 0 and out.is_cuda
    return np.float32(out.item())


def ranks_of(pairs, seed):
    rng = np.random.default_rng(seed)
    return sorted({0, pairs - 1, ka.lower_median_rank(pairs), *(int(r) for r in rng.integers(0, pairs, 2))})


WIDE_NOISE_BITS = 15


def wide_exact_rows(rng, n, d, sigma):
    """float64 rows of integers in [-2^17, 2^17] times a per-row power of two 2^(c + e), e in {-1, 0, 1}.  The integers are a
    column offset shared by every set of width d (embeddings have a non-zero mean; it makes the dot products large beside
    the distances, which is where an f32 accumulation loses most) plus noise in [-2^15, 2^15]; c is chosen as in
    kd_reference.rbf_rows: the noise of an element has rms sigma / sqrt(d), so squared distances are of the order of
    2 sigma^2 and more.  A dot product is a power of two times an integer below 512 * 2^34 < 2^53 (d <= 512): norms, dots
    and d2 are exact in f64 whatever the order of the additions; an f32 accumulation of the 34-bit products is not."""
    half = 2 ** WIDE_NOISE_BITS
    c = int(np.round(np.log2(sigma * np.sqrt(3.0) / (np.sqrt(d) * half))))
    offset = np.random.default_rng(515 + d).integers(-(2 ** 17 - half), 2 ** 17 - half + 1, size=(1, d))
    ints = (offset + rng.integers(-half, half + 1, size=(n, d))).astype(np.float64)
    assert np.abs(ints).max() <= 2 ** 17
    e = rng.integers(-1, 2, size=(n, 1)).astype(np.float64)
    return ints * np.exp2(c + e)


def summation_tol(d, *sets):
    """2 (4 D + 4) 2^-53 max_i |x_i|^2: the worst-case f64 summation error of the two norms, the dot product and the final
    fma of one squared distance, once for the device and once for numpy (derived, not measured)."""
    biggest = max(float(ka.sq_norms(s).max()) for s in sets)
    return 2.0 * (4 * d + 4) * 2.0 ** -53 * biggest


# ---------------------------------------------------------------------------------------------------- G1. select, exact data
@pytest.mark.parametrize("n, d", [(2, 5), (65, 16), (129, 100), (300, 64), (257, 33)])
def test_select_is_exact_on_wide_exact_data(ops, n, d):
    x = wide_exact_rows(np.random.default_rng(2000 + n + d), n, d, SIGMA)
    assert x.dtype == np.float64
    want = ka.pair_values(x)
    pairs = n * (n - 1) // 2
    assert len(want) == pairs
    xt = dev(x)
    for rank in ranks_of(pairs, n):
        got = select(ops, xt, rank)
        assert bits(got) == bits(ka.as_key(want[rank])), (n, d, rank, got, want[rank])
    assert bits(select(ops, xt)) == bits(ka.as_key(want[ka.lower_median_rank(pairs)]))          # rank=None: the lower median


# ---------------------------------------------------------------------------------------------------- G2. select, edge cases
def test_select_on_a_strided_view_with_an_odd_stride(ops):
    n, d, ld = 300, 100, 113
    x = wide_exact_rows(np.random.default_rng(7), n, d, SIGMA)
    buf = torch.full((n, ld), 1e300, dtype=torch.float64, device=DEV)                            # the padding must never be read as data
    buf[:, :d] = dev(x)
    view = buf[:, :d]
    assert view.stride(0) == ld and ld % 2 == 1
    want = ka.pair_values(x)
    for rank in ranks_of(len(want), 3):
        assert bits(select(ops, view, rank)) == bits(ka.as_key(want[rank])), rank


def test_select_with_many_duplicate_rows(ops):
    rng = np.random.default_rng(11)
    points = wide_exact_rows(rng, 3, 64, SIGMA)
    counts = [250, 30, 20]                                       # 31 750 of the 44 850 pairs coincide: the median is exactly 0
    x = np.repeat(points, counts, axis=0)[rng.permutation(300)]
    xt = dev(x)
    pairs = 300 * 299 // 2
    assert select(ops, xt) == 0.0 and select(ops, xt, 0) == 0.0
    top = ka.d2_matrix(points, points).max()
    assert bits(select(ops, xt, pairs - 1)) == bits(ka.as_key(top))
    want = ka.pair_values(x)
    for rank in (31_749, 31_750, pairs - 2):                      # last zero, first non-zero
        assert bits(select(ops, xt, rank)) == bits(ka.as_key(want[rank])), rank


def test_select_with_a_nan_row(ops):
    n, d = 50, 33
    x = wide_exact_rows(np.random.default_rng(13), n, d, SIGMA)
    x[17, 5] = np.nan
    xt = dev(x)
    want = ka.pair_values(x)                                      # the 49 pairs of row 17 sort last, as +inf
    pairs = n * (n - 1) // 2
    assert np.isinf(want[pairs - 49:]).all() and np.isfinite(want[:pairs - 49]).all()
    for rank in (pairs - 1, pairs - 49):
        assert select(ops, xt, rank) == np.inf
    finite = ka.pair_values(np.delete(x, 17, axis=0))
    assert bits(select(ops, xt, pairs - 50)) == bits(ka.as_key(finite[-1]))
    med = select(ops, xt)
    assert np.isfinite(med) and bits(med) == bits(ka.as_key(want[ka.lower_median_rank(pairs)]))


# ---------------------------------------------------------------------------------------------------- G3. 64-bit counts
def test_select_counts_in_64_bits(ops):
    """93 000 rows drawn from 7 points: P = 4.3e9 > 2^32 pairs, all of them in 22 distinct keys (the contention worst case)."""
    n, d, groups = 93_000, 16, 7
    rng = np.random.default_rng(17)
    points = wide_exact_rows(rng, groups, d, SIGMA)
    counts = rng.multinomial(n - groups, np.full(groups, 1.0 / groups)) + 1
    x = np.repeat(points, counts, axis=0)[rng.permutation(n)]
    pairs = n * (n - 1) // 2
    assert pairs > 2 ** 32
    values, weights = ka.group_pairs(points, counts)
    assert sum(weights) == pairs
    xt = dev(x)
    for rank in (0, ka.lower_median_rank(pairs), pairs - 1, 2 ** 32 + 12_345):
        want = ka.weighted_order_statistic(values, weights, rank)
        assert bits(select(ops, xt, rank)) == bits(ka.as_key(want)), (rank, want)


# ---------------------------------------------------------------------------------------------------- G4. select, real-valued rows
@pytest.mark.parametrize("kind, d", [("unit", 64), ("randn", 64), ("unit", 100), ("randn", 100)])
def test_select_on_real_valued_rows(ops, kind, d):
    """Moving every value by at most eps moves every order statistic by at most eps: the device's d2 and numpy's each carry
    the f64 summation error of the norms, the dot product and the final fma, and the key is that value rounded to float32
    (one ulp of the oracle value covers it)."""
    n = 1000
    x = gi.pair(kind, 700 + d, n, 2, d)[0].astype(np.float64)
    want = ka.pair_values(x)
    tol_d2 = summation_tol(d, x)
    xt = dev(x)
    pairs = n * (n - 1) // 2
    for rank in ranks_of(pairs, d):
        got = float(select(ops, xt, rank))
        tol = tol_d2 + float(np.spacing(np.float32(want[rank])))
        print(f"{kind} D={d} rank={rank}: got {got!r} oracle {want[rank]!r} |diff| {abs(got - want[rank]):.3e} tol {tol:.3e}")
        assert abs(got - want[rank]) <= tol, (kind, d, rank, got, want[rank], tol)


# ---------------------------------------------------------------------------------------------------- G5. sums, exact data
SUM_SHAPES = [(2, 2, 5), (65, 129, 16), (129, 300, 100), (1000, 257, 64)]


@pytest.fixture(scope="module")
def exact_sets():
    out = {}
    for n, m, d in SUM_SHAPES:
        rng = np.random.default_rng(n * 7 + m * 3 + d)
        x, y = wide_exact_rows(rng, n, d, SIGMA), wide_exact_rows(rng, m, d, SIGMA)
        means, scale = ka.mmd_parts(x, y, GAMMA)
        # the same statistic from f32 dot products misses the bound of these tests by far: narrowing to the f32 kernels fails
        narrowed, _ = ka.mmd_parts(x, y, GAMMA, dots=kr.emulated_dots("f32"))
        assert np.abs(narrowed - means).max() > 100.0 * EXACT * scale, (n, m, d, narrowed, means)
        out[(n, m, d)] = (x, y, means, scale)
    return out


@pytest.mark.parametrize("shape", SUM_SHAPES)
def test_sums_on_wide_exact_data(ops, exact_sets, shape):
    n, m, d = shape
    x, y, want, scale = exact_sets[shape]
    assert 0.01 < scale < 0.99                                      # K spreads over (0, 1)
    xt, yt = dev(x), dev(y)
    assert xt.dtype == torch.float64
    sums = ops.mmd_rbf_sums(xt, yt, gamma=GAMMA)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (3,)
    got = ka.device_means(sums.cpu().numpy(), n, m)
    err = np.abs(got - want)
    print(f"{shape}: |err| {err} limit {EXACT * scale:.3e}")
    assert (err <= EXACT * scale).all(), (shape, got, want, scale)
    # two calls: the same bits
    again = ops.mmd_rbf_sums(xt, yt, gamma=GAMMA)
    assert torch.equal(sums, again)
    # the bandwidth from device memory: gamma = 0.5 / (double)bw2 formed on the device = the same host expression
    bw2 = np.float32(SIGMA * SIGMA * 1.0009765625)
    fed = ops.mmd_rbf_sums(xt, yt, bw2=torch.tensor(bw2, dtype=torch.float32, device=DEV))
    host = ops.mmd_rbf_sums(xt, yt, gamma=0.5 / float(bw2))
    assert torch.equal(fed, host)
    # swapping the sets swaps Sxx / Syy exactly; Sxy is the same sum in another order
    a, b = sums.cpu().numpy(), ops.mmd_rbf_sums(yt, xt, gamma=GAMMA).cpu().numpy()
    assert a[0] == b[1] and a[1] == b[0]
    assert abs(a[2] - b[2]) <= 1e-15 * abs(a[2]), (a[2], b[2])


@pytest.mark.parametrize("blocks", [1, 2, 4, 3, 5, 6])
def test_block_mask_writes_only_what_it_names(ops, exact_sets, blocks):
    x, y, _, _ = exact_sets[(129, 300, 100)]
    xt, yt = dev(x), dev(y)
    full = ops.mmd_rbf_sums(xt, yt, gamma=GAMMA)
    sentinel = -12345.5
    out = torch.full((3,), sentinel, dtype=torch.float64, device=DEV)
    ret = ops.mmd_rbf_sums(xt, yt, gamma=GAMMA, blocks=blocks, out=out)
    assert ret is out
    for slot in range(3):
        if blocks & (1 << slot):
            assert out[slot].item() == full[slot].item(), slot          # and the value does not depend on the mask
        else:
            assert out[slot].item() == sentinel, slot


# ---------------------------------------------------------------------------------------------------- G6. sums, real-valued rows
@pytest.mark.parametrize("kind, d", [("randn", 64), ("unit", 100)])
def test_sums_on_real_valued_rows(ops, kind, d):
    """|dK| <= gamma |d d2| (K <= 1): each normalised sum within gamma x the f64 summation bound of one squared distance
    plus the exact-data bound (exp and the sums themselves); mmd^2 = xx + yy - 2 xy gets the combination of the limits."""
    n = m = 1000
    y, x = (s.astype(np.float64) for s in gi.pair(kind, 800 + d, m, n, d))
    pairs = ka.pair_values(y)
    gamma = 0.5 / float(pairs[ka.lower_median_rank(len(pairs))])     # the kernel width KAD itself would take
    want, scale = ka.mmd_parts(x, y, gamma)
    got = ka.device_means(ops.mmd_rbf_sums(dev(x), dev(y), gamma=gamma).cpu().numpy(), n, m)
    limit = gamma * summation_tol(d, x, y) + EXACT * scale
    stats = [(name, g, w, limit) for name, g, w in zip(("xx", "yy", "xy"), got, want)]
    stats.append(("mmd2", ka.mmd2(got), ka.mmd2(want), 4.0 * limit))
    for name, g, w, lim in stats:
        print(f"{kind} D={d} {name}: device {g!r} oracle {w!r} |err| {abs(g - w):.3e} limit {lim:.3e}")
    for name, g, w, lim in stats:
        assert abs(g - w) <= lim, (kind, d, name, g, w, lim)


# ---------------------------------------------------------------------------------------------------- G7. groups
GROUP_CASES = {"straddle": ([1, 2, 63, 64, 65, 105], 257, 33), "even": ([50] * 20, 300, 64)}


@pytest.fixture(scope="module")
def group_cases():
    """Per case: the rows in LIST order, a shuffled store with the permutation that finds them, the reference rows and the
    oracle (computed once, shared)."""
    out = {}
    for name, (sizes, m, d) in GROUP_CASES.items():
        rng = np.random.default_rng(9000 + len(sizes) + d)
        n = sum(sizes)
        x_list, y = wide_exact_rows(rng, n, d, SIGMA), wide_exact_rows(rng, m, d, SIGMA)
        idx = rng.permutation(n).astype(np.int64)
        store = np.empty_like(x_list)
        store[idx] = x_list                                           # list position p is stored row idx[p]
        offs = kg.offsets_of(sizes)
        want = kg.group_sums(x_list, offs, y, GAMMA)
        narrowed = kg.group_sums(x_list, offs, y, GAMMA, dots=kr.emulated_dots("f32"))
        assert np.abs(narrowed["mean_xy"] - want["mean_xy"]).max() > 100.0 * EXACT * want["scale"]
        out[name] = dict(sizes=sizes, m=m, d=d, x_list=x_list, y=y, idx=idx, store=store, offs=offs, want=want)
    return out


def group_sums(ops, store, idx, offs, y, rows=True, **width):
    res = ops.mmd_rbf_group_sums(store, idx, [int(o) for o in offs], y, rows=rows, **width)
    res[-1]()
    out = res[0]
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(offs) - 1, 2) and out.is_cuda
    return out.cpu().numpy(), res[1].cpu().numpy() if rows else None


@pytest.mark.parametrize("case", sorted(GROUP_CASES))
def test_groups_on_wide_exact_data(ops, group_cases, case):
    c = group_cases[case]
    want, sizes, m, offs = c["want"], c["sizes"], c["m"], c["offs"]
    assert 0.01 < want["scale"] < 0.99
    assert sum(sizes) == {"straddle": 300, "even": 1000}[case] and not (c["idx"] == np.arange(len(c["idx"]))).all()
    store, idx, yt = dev(c["store"]), dev(c["idx"]), dev(c["y"])
    assert store.dtype == torch.float64 and yt.dtype == torch.float64
    got, got_rows = group_sums(ops, store, idx, offs, yt, gamma=GAMMA)
    limit = EXACT * want["scale"]
    xx, xy = kg.device_means(got, sizes, m)
    single = np.asarray(sizes) == 1
    print(f"{case}: xx {np.nanmax(np.abs(xx - want['mean_xx'])):.3e} xy {np.abs(xy - want['mean_xy']).max():.3e} limit {limit:.3e}")
    assert (np.abs(xx - want["mean_xx"])[~single] <= limit).all() and (np.abs(xy - want["mean_xy"]) <= limit).all()
    assert (got[single, 0] == 0.0).all()                              # a group of one row has no within pairs
    # the row sums, position by position
    rw, rc = kg.row_means(got_rows, offs, m)
    per_row = np.repeat(sizes, sizes)
    want_w = np.where(per_row > 1, want["w"] / np.maximum(per_row - 1.0, 1.0), np.nan)
    assert (np.abs(rc - want["c"] / m) <= limit).all()
    assert (np.abs(rw - want_w)[per_row > 1] <= limit).all()
    # the result depends on the list order only: the groups in stored order give the same bits, and so does a second call
    stored, stored_rows = group_sums(ops, dev(c["x_list"]), None, offs, yt, gamma=GAMMA)
    assert np.array_equal(stored, got) and np.array_equal(stored_rows, got_rows)
    again, again_rows = group_sums(ops, store, idx, offs, yt, gamma=GAMMA)
    assert np.array_equal(again, got) and np.array_equal(again_rows, got_rows)
    # the groups partition the list: their cross sums add up to the whole-set one
    whole = ops.mmd_rbf_sums(dev(c["x_list"]), yt, gamma=GAMMA, blocks=ops.MMD_XY)[2].item()
    assert abs(got[:, 1].sum() - whole) <= 1e-13 * abs(whole), (got[:, 1].sum(), whole)
    # the bandwidth from device memory
    bw2 = np.float32(SIGMA * SIGMA * 1.0009765625)
    fed, _ = group_sums(ops, store, idx, offs, yt, rows=False, bw2=torch.tensor(bw2, dtype=torch.float32, device=DEV))
    host, _ = group_sums(ops, store, idx, offs, yt, rows=False, gamma=0.5 / float(bw2))
    assert np.array_equal(fed, host)


def test_an_out_of_range_index_is_reported(ops, group_cases):
    c = group_cases["straddle"]
    offs = [int(o) for o in c["offs"]]
    store, yt = dev(c["store"]), dev(c["y"])
    clean, _ = group_sums(ops, store, dev(c["idx"]), offs, yt, rows=False, gamma=GAMMA)
    victim = 3                                                        # the group of 64 rows
    for bad_value in (len(c["store"]), -1, 2 ** 40):
        idx = c["idx"].copy()
        pos = offs[victim] + 9
        idx[pos] = bad_value
        out, check = ops.mmd_rbf_group_sums(store, dev(idx), offs, yt, gamma=GAMMA)
        with pytest.raises(ValueError, match=r"idx\[%d\] = %d is outside \[0, %d\)" % (pos, bad_value, len(c["store"]))):
            check()
        got = out.cpu().numpy()
        others = [b for b in range(len(c["sizes"])) if b != victim]
        assert np.array_equal(got[others], clean[others])
        x_zero = c["x_list"].copy()                                   # the row counts as zeros
        x_zero[pos] = 0.0
        want = kg.group_sums(x_zero, c["offs"], c["y"], GAMMA)
        xx, xy = kg.device_means(got, c["sizes"], c["m"])
        assert abs(xx[victim] - want["mean_xx"][victim]) <= EXACT * want["scale"]
        assert abs(xy[victim] - want["mean_xy"][victim]) <= EXACT * want["scale"]


# ---------------------------------------------------------------------------------------------------- G8. end to end
def data_of(am, rows, step=97):
    s = am.AudioMetricsData(True, device=DEV)
    for k in range(0, len(rows), step):
        s.add(dev(rows[k:k + step]))
    assert s.embeddings.dtype == torch.float64
    return s


def oracle_kad(x, y, bw2=None):
    if bw2 is None:
        p = ka.pair_values(y)
        bw2 = float(ka.as_key(p[ka.lower_median_rank(len(p))]))
    means, scale = ka.mmd_parts(x, y, 0.5 / bw2)
    return ka.mmd2(means), scale, bw2


def test_kernel_audio_distance_on_float64_sets(am, monkeypatch):
    rng = np.random.default_rng(31)
    x, y, more = (wide_exact_rows(rng, n, 64, SIGMA) for n in (150, 400, 130))
    calls = {"select": 0, "yy": 0}
    real_select, real_sums = am.hip_ops.pairwise_select_sq, am.hip_ops.mmd_rbf_sums

    def counting_select(*a, **k):
        calls["select"] += 1
        return real_select(*a, **k)

    def counting_sums(*a, **k):
        calls["yy"] += 1 if k.get("blocks", 7) & 2 else 0
        return real_sums(*a, **k)
    monkeypatch.setattr(am.hip_ops, "pairwise_select_sq", counting_select)
    monkeypatch.setattr(am.hip_ops, "mmd_rbf_sums", counting_sums)
    cand, ref = data_of(am, x), data_of(am, y)
    want, scale, bw2 = oracle_kad(x, y)
    first = am.kernel_audio_distance(cand, ref)
    assert list(first) == ["kad", "kad_mmd2", "kad_bandwidth"]
    assert first["kad_bandwidth"] == np.sqrt(bw2)                     # sqrt(float(rn32(median)))
    print(f"mmd2 {first['kad_mmd2']!r} oracle {want!r} limit {3 * EXACT * scale:.3e}")
    assert abs(first["kad_mmd2"] - want) <= 3 * EXACT * scale and first["kad"] == 100.0 * first["kad_mmd2"]
    assert calls == {"select": 1, "yy": 1}
    second = am.kernel_audio_distance(cand, ref)
    assert calls == {"select": 1, "yy": 1} and second == first       # neither the median nor Syy again
    ref.add(dev(more))
    grown = am.kernel_audio_distance(cand, ref)
    assert calls == {"select": 2, "yy": 2}                           # both recomputed for the grown set
    want, scale, bw2 = oracle_kad(x, np.concatenate([y, more]))
    assert grown["kad_bandwidth"] == np.sqrt(bw2) and abs(grown["kad_mmd2"] - want) <= 3 * EXACT * scale
    # a fixed bandwidth is honoured
    want3, scale3, _ = oracle_kad(x, np.concatenate([y, more]), bw2=81.0)
    fixed = am.kernel_audio_distance(cand, ref, bandwidth=9.0, scale=1.0)
    assert fixed["kad_bandwidth"] == 9.0 and abs(fixed["kad_mmd2"] - want3) <= 3 * EXACT * scale3 and fixed["kad"] == fixed["kad_mmd2"]
    # a mixed pair is still refused, either way round
    x32 = am.AudioMetricsData(True, device=DEV)
    x32.add(dev(x.astype(np.float32)))
    with pytest.raises(NotImplementedError, match="float64"):
        am.kernel_audio_distance(x32, ref)
    with pytest.raises(NotImplementedError, match="float64"):
        am.kernel_audio_distance(cand, x32)


def test_per_group_on_float64_sets(am):
    rng = np.random.default_rng(4700)
    n, m, d = 400, 257, 33
    x, y = wide_exact_rows(rng, n, d, SIGMA), wide_exact_rows(rng, m, d, SIGMA)
    labels = rng.choice(np.array([-5, 3, 11, 12, 40, 1000]), size=n, p=[0.3, 0.05, 0.3, 0.2, 0.1, 0.05])
    labels[123] = 77                                                  # one group of a single row
    assert (labels == 77).sum() == 1
    cand, ref = data_of(am, x), data_of(am, y)
    p = ka.pair_values(y)
    bw2 = float(ka.as_key(p[ka.lower_median_rank(len(p))]))
    order = np.argsort(labels, kind="stable")
    uniq, sizes = np.unique(labels, return_counts=True)
    g = kg.group_sums(x[order], kg.offsets_of(sizes), y, 0.5 / bw2)
    mean_yy = ka.mmd_parts(y[:2], y, 0.5 / bw2)[0][1]
    want = kg.mmd2_per_group(g["mean_xx"], g["mean_xy"], mean_yy)
    cross = np.empty(n)
    cross[order] = g["c"] / m
    with pytest.warns(RuntimeWarning, match="1 of 7 groups hold a single row") as rec:
        got = am.kernel_audio_distance_per_group(cand, ref, labels, return_rows=True)
    assert len([r for r in rec if issubclass(r.category, RuntimeWarning)]) == 1
    assert list(got) == ["kad_per_group", "kad_mmd2_per_group", "group_labels", "group_sizes", "kad_bandwidth", "row_cross_mean"]
    assert got["group_labels"].tolist() == uniq.tolist() and got["group_sizes"].tolist() == sizes.tolist()
    assert got["kad_bandwidth"] == np.sqrt(bw2)
    single = sizes == 1
    assert single.sum() == 1 and np.isnan(got["kad_mmd2_per_group"][single]).all()
    err = np.abs(got["kad_mmd2_per_group"] - want)[~single]
    print(f"per group mmd2 max |err| {err.max():.3e} limit {3 * EXACT * g['scale']:.3e}")
    assert (err <= 3 * EXACT * g["scale"]).all()
    assert got["row_cross_mean"].shape == (n,) and (np.abs(got["row_cross_mean"] - cross) <= EXACT * g["scale"]).all()   # stored order
    whole = am.kernel_audio_distance(cand, ref)                       # the same reference-side cache
    assert whole["kad_bandwidth"] == got["kad_bandwidth"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        keep = labels != 77
        plain = am.kernel_audio_distance_per_group(data_of(am, x[keep]), ref, labels[keep], scale=1.0)
    assert "row_cross_mean" not in plain and np.array_equal(plain["kad_per_group"], plain["kad_mmd2_per_group"])


class Float64Embedder(gi.NumpyEmbedder):
    """the host-side test embedder with its float64 values handed on as they are"""

    def forward(self, data, sr=None):
        audio = np.asarray(data["audio"], dtype=np.float64)
        if audio.ndim == 1:
            audio = audio[None]
        n = audio.shape[1] // self.frame * self.frame
        frames = audio[:, :n].reshape(len(audio), -1, self.frame)
        h = np.tanh(3.0 * frames @ self.w)
        emb = np.concatenate([h.mean(1)[:, : self.w.shape[1] // 2], h.std(1)[:, self.w.shape[1] // 2:]], axis=1)
        return {"embedding": torch.as_tensor(emb)}


def test_a_float64_embedder_through_audio_metrics(am):
    c = gi.E2E

    def make(metrics):
        return am.AudioMetrics(metrics=metrics, embedder=Float64Embedder(c["dim"], c["sr"]), mix_function=gi.e2e_mix,
                               win_dur=c["win_dur"], device_indices=[0])
    ref = [x[:, 1] for x in gi.e2e_pairs(c["seed"], c["n_ref"], c["seconds"], c["sr"])]
    cand = [x[:, 1] for x in gi.e2e_pairs(c["seed"] + 1, c["n_cand"], c["seconds"], c["sr"], stem_gain=1.3)]
    m_kad = make(["fad", "kad"])
    m_kad.add_reference(ref)
    with_kad = m_kad.evaluate(cand)
    assert m_kad.stem_reference.embeddings.dtype == torch.float64
    # the SAME object without "kad", not a second one built with metrics=["fad"]: a set that stores its rows (any row
    # metric: "kd", "prdc", "kad") gets the one-shot statistics of add_reference's recompute_stats(), a set that does not
    # keeps the batch-merged ones, and the two differ in the last bits of float64 rows whatever the row metric is
    m_kad.metrics = ["fad"]
    plain = m_kad.evaluate(cand)
    m_kad.metrics = ["fad", "kad"]
    kad_keys = ["kad", "kad_mmd2", "kad_bandwidth"]
    assert [k for k in with_kad if k not in kad_keys] == list(plain)
    for key, value in plain.items():
        assert with_kad[key] == value, key                               # bit-equal: no existing path changed
    assert all(np.isfinite(with_kad[k]) for k in kad_keys)
    direct = am.kernel_audio_distance(m_kad._embed(cand, "candidate")[am.ItemCategory.stem], m_kad.stem_reference)
    assert {k: with_kad[k] for k in kad_keys} == direct
