"""Kernel Audio Distance on the device against float64 oracles (tests/kad_reference.py).

  1-3  hip_ops.pairwise_select_sq: bit-exact on data whose squared distances are exact in f64 (every rank kind, row views,
       duplicate-heavy sets, a NaN row, 64-bit pair counts), within the priced rounding of the f32 dot products otherwise;
  4-5  hip_ops.mmd_rbf_sums: 1e-12 x mean |K| on exact data (the bound of tests/test_gpu_kd.py), MARGIN x the emulated
       error of the same statistic on real-valued rows; block mask, device-fed bandwidth, repeatability, symmetry;
  6    kernel_audio_distance and the "kad" metric of AudioMetrics: values, the reference-side cache and its invalidation."""
import numpy as np
import pytest
import torch

import inputs as gi
import kad_reference as ka
import kd_reference as kr

pytestmark = pytest.mark.gpu

EXACT = 1e-12
DEV = "cuda:0"


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
    out = ops.pairwise_select_sq(xt, rank)
    assert out.dtype == torch.float32 and out.dim() == 0 and out.is_cuda
    return np.float32(out.item())


def ranks_of(pairs, seed):
    rng = np.random.default_rng(seed)
    return sorted({0, pairs - 1, ka.lower_median_rank(pairs), *(int(r) for r in rng.integers(0, pairs, 2))})


# ---------------------------------------------------------------------------------------------------- 1. select, exact data
@pytest.mark.parametrize("n, d", [(2, 32), (129, 32), (300, 100), (257, 512), (1000, 64)])
def test_select_is_exact_on_exact_data(ops, n, d):
    x = kr.exact_rows(np.random.default_rng(1000 + n + d), n, d)
    want = ka.pair_values(x)
    pairs = n * (n - 1) // 2
    assert len(want) == pairs
    xt = dev(x)
    for rank in ranks_of(pairs, n):
        got = select(ops, xt, rank)
        assert bits(got) == bits(ka.as_key(want[rank])), (n, d, rank, got, want[rank])
    assert bits(select(ops, xt)) == bits(ka.as_key(want[ka.lower_median_rank(pairs)]))          # rank=None: the lower median


def test_select_on_a_strided_view(ops):
    n, d, ld = 300, 100, 112
    x = kr.exact_rows(np.random.default_rng(7), n, d)
    buf = torch.full((n, ld), 1e30, dtype=torch.float32, device=DEV)                             # the padding must never be read as data
    buf[:, :d] = dev(x)
    view = buf[:, :d]
    assert view.stride(0) == ld
    want = ka.pair_values(x)
    for rank in ranks_of(len(want), 3):
        assert bits(select(ops, view, rank)) == bits(ka.as_key(want[rank])), rank


def test_select_with_many_duplicate_rows(ops):
    rng = np.random.default_rng(11)
    points = kr.exact_rows(rng, 3, 64)
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
    n, d = 50, 32
    x = kr.exact_rows(np.random.default_rng(13), n, d)
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
    assert med == ka.as_key(finite[ka.lower_median_rank(pairs)])                                  # the finite pairs' own order


# ---------------------------------------------------------------------------------------------------- 2. 64-bit counts
def test_select_counts_in_64_bits(ops):
    """93 000 rows drawn from 7 points: P = 4.3e9 > 2^32 pairs, all of them in 22 distinct keys (the contention worst case)."""
    n, d, groups = 93_000, 32, 7
    rng = np.random.default_rng(17)
    points = kr.exact_rows(rng, groups, d)
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


# ---------------------------------------------------------------------------------------------------- 3. select, real-valued rows
@pytest.mark.parametrize("kind, d", [("unit", 64), ("randn", 64), ("unit", 512), ("randn", 512)])
def test_select_on_real_valued_rows(ops, kind, d):
    """Moving every value by at most eps moves every order statistic by at most eps: the device's d2 differs from the f64
    one by 2 |f32 dot - f64 dot| (priced by the emulation, times MARGIN for the matrix cores' own accumulation order), and
    the key is that value rounded to float32 (one ulp of the oracle value covers it)."""
    n = 1000
    x, _ = gi.pair(kind, 700 + d, n, 2, d)
    exact = x.astype(np.float64) @ x.astype(np.float64).T
    shift = float(np.max(np.abs(2.0 * (kr.emulated_dots("f32")(x, x) - exact))))
    want = ka.pair_values(x)
    xt = dev(x)
    pairs = n * (n - 1) // 2
    for rank in ranks_of(pairs, d):
        got = float(select(ops, xt, rank))
        tol = kr.MARGIN * shift + float(np.spacing(np.float32(want[rank])))
        print(f"{kind} D={d} rank={rank}: got {got!r} oracle {want[rank]!r} |diff| {abs(got - want[rank]):.3e} tol {tol:.3e}")
        assert abs(got - want[rank]) <= tol, (kind, d, rank, got, want[rank], tol)


# ---------------------------------------------------------------------------------------------------- 4. sums, exact data
SIGMA = 10.0
GAMMA = 1.0 / (2.0 * SIGMA * SIGMA)
SUM_SHAPES = [(2, 2, 32), (129, 300, 100), (1000, 257, 512), (128, 128, 64)]


@pytest.fixture(scope="module")
def exact_sets():
    out = {}
    for n, m, d in SUM_SHAPES:
        rng = np.random.default_rng(n * 7 + m * 3 + d)
        x, y = kr.rbf_rows(rng, n, d, SIGMA), kr.rbf_rows(rng, m, d, SIGMA)
        means, scale = ka.mmd_parts(x, y, GAMMA)
        out[(n, m, d)] = (x, y, means, scale)
    return out


@pytest.mark.parametrize("shape", SUM_SHAPES)
def test_sums_on_exact_data(ops, exact_sets, shape):
    n, m, d = shape
    x, y, want, scale = exact_sets[shape]
    assert n == 2 or 0.01 < scale < 0.99                            # K spreads over (0, 1)
    xt, yt = dev(x), dev(y)
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


# ---------------------------------------------------------------------------------------------------- 5. sums, real-valued rows
@pytest.mark.parametrize("kind, d", [("randn", 64), ("unit", 512)])
def test_sums_on_real_valued_rows(ops, kind, d):
    """Each normalised sum within MARGIN x the emulated error of the same sum (the f32 dot products rounded once per
    32-element slab, kd_reference.emulated_dots; MARGIN covers the matrix cores' rounding after every product).  mmd^2 is
    their combination xx + yy - 2 xy and gets the combination of their limits: the three blocks' rounding errors are
    independent of each other, so a cancellation between them in the emulated run (randn, D = 64: 6.7e-13, 1.1e-12 and
    7.5e-13 cancel to 3.0e-13 in mmd^2) is an accident of that run and says nothing about the device's."""
    n = m = 1000
    y, x = gi.pair(kind, 800 + d, m, n, d)
    pairs = ka.pair_values(y)
    gamma = 0.5 / float(pairs[ka.lower_median_rank(len(pairs))])     # the kernel width KAD itself would take
    want, _ = ka.mmd_parts(x, y, gamma)
    emulated, _ = ka.mmd_parts(x, y, gamma, dots=kr.emulated_dots("f32"))
    got = ka.device_means(ops.mmd_rbf_sums(dev(x), dev(y), gamma=gamma).cpu().numpy(), n, m)
    limits = kr.MARGIN * np.abs(emulated - want)
    stats = [(name, g, w, lim) for name, g, w, lim in zip(("xx", "yy", "xy"), got, want, limits)]
    stats.append(("mmd2", ka.mmd2(got), ka.mmd2(want), float(limits[0] + limits[1] + 2.0 * limits[2])))
    for name, g, w, lim in stats:
        print(f"{kind} D={d} {name}: device {g!r} oracle {w!r} |err| {abs(g - w):.3e} limit {lim:.3e}")
    for name, g, w, lim in stats:
        assert abs(g - w) <= lim, (kind, d, name, g, w, lim)


# ---------------------------------------------------------------------------------------------------- 6. end to end
def data_of(am, rows, step=97):
    s = am.AudioMetricsData(True, device=DEV)
    for k in range(0, len(rows), step):
        s.add(dev(rows[k:k + step]))
    return s


def oracle_kad(x, y, bw2=None):
    if bw2 is None:
        p = ka.pair_values(y)
        bw2 = float(ka.as_key(p[ka.lower_median_rank(len(p))]))
    means, scale = ka.mmd_parts(x, y, 0.5 / bw2)
    return ka.mmd2(means), scale, bw2


def test_kernel_audio_distance_on_exact_data(am):
    rng = np.random.default_rng(23)
    x, y = kr.rbf_rows(rng, 300, 100, SIGMA), kr.rbf_rows(rng, 513, 100, SIGMA)
    want, scale, bw2 = oracle_kad(x, y)
    got = am.kernel_audio_distance(data_of(am, x), data_of(am, y), scale=1000.0)
    assert list(got) == ["kad", "kad_mmd2", "kad_bandwidth"]
    assert got["kad_bandwidth"] == np.sqrt(bw2)
    print(f"mmd2 {got['kad_mmd2']!r} oracle {want!r} limit {3 * EXACT * scale:.3e}")
    assert abs(got["kad_mmd2"] - want) <= 3 * EXACT * scale          # three statistics, each within the bound of case 4
    assert got["kad"] == 1000.0 * got["kad_mmd2"]
    assert am.kernel_audio_distance(data_of(am, x), data_of(am, y))["kad"] == 100.0 * got["kad_mmd2"]
    # a fixed bandwidth is honoured
    want3, scale3, _ = oracle_kad(x, y, bw2=9.0)
    fixed = am.kernel_audio_distance(data_of(am, x), data_of(am, y), bandwidth=3.0)
    assert fixed["kad_bandwidth"] == 3.0 and abs(fixed["kad_mmd2"] - want3) <= 3 * EXACT * scale3


def test_identical_sets_match_the_oracle_not_zero(am):
    x = kr.rbf_rows(np.random.default_rng(29), 200, 64, SIGMA)
    want, scale, _ = oracle_kad(x, x)
    got = am.kernel_audio_distance(data_of(am, x), data_of(am, x))["kad_mmd2"]
    print(f"identical sets: mmd2 {got!r} oracle {want!r}")
    assert want < 0.0                                                # the unbiased estimate of 0 drops the diagonal of Kxx / Kyy only
    assert abs(got - want) <= 1e-12


def test_reference_side_is_cached_and_recomputed_after_an_append(am, monkeypatch):
    rng = np.random.default_rng(31)
    x, y, more = (kr.rbf_rows(rng, n, 64, SIGMA) for n in (150, 400, 130))
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
    first = am.kernel_audio_distance(cand, ref)
    assert calls == {"select": 1, "yy": 1}
    second = am.kernel_audio_distance(cand, ref)
    assert calls == {"select": 1, "yy": 1} and second == first       # neither the median nor Syy again
    other = am.kernel_audio_distance(data_of(am, more), ref)          # another candidate set, the same reference
    assert calls == {"select": 1, "yy": 1}
    assert abs(other["kad_mmd2"] - oracle_kad(more, y)[0]) <= 3 * EXACT * oracle_kad(more, y)[1]
    assert "_kad_cache" not in ref.serialize() and set(ref.serialize()) == set(am.AudioMetricsData(True, device=DEV).serialize())
    ref.add(dev(more))
    grown = am.kernel_audio_distance(cand, ref)
    assert calls == {"select": 2, "yy": 2}                           # both recomputed for the grown set
    fresh = am.kernel_audio_distance(data_of(am, x), data_of(am, np.concatenate([y, more])))
    assert grown == fresh
    want, scale, bw2 = oracle_kad(x, np.concatenate([y, more]))
    assert grown["kad_bandwidth"] == np.sqrt(bw2) and abs(grown["kad_mmd2"] - want) <= 3 * EXACT * scale


def test_degenerate_bandwidths_raise(am):
    rng = np.random.default_rng(37)
    x = kr.rbf_rows(rng, 40, 32, SIGMA)
    dup = np.repeat(kr.rbf_rows(rng, 2, 32, SIGMA), [35, 5], axis=0)
    with pytest.raises(ValueError, match="coincide"):
        am.kernel_audio_distance(data_of(am, x), data_of(am, dup))
    bad = x.copy()
    bad[::2, 0] = np.nan                                             # half of the rows: more than half of the pairs
    with pytest.raises(ValueError, match="non-finite"):
        am.kernel_audio_distance(data_of(am, x), data_of(am, bad))
    with pytest.raises(ValueError, match="at least 2 rows"):
        am.kernel_audio_distance(data_of(am, x[:1]), data_of(am, x))
    with pytest.raises(NotImplementedError, match="float64"):
        am.kernel_audio_distance(data_of(am, x.astype(np.float64)), data_of(am, x))


def test_through_audio_metrics(am):
    c = gi.E2E

    def make(metrics, **kw):
        return am.AudioMetrics(metrics=metrics, embedder=gi.NumpyEmbedder(c["dim"], c["sr"]), mix_function=gi.e2e_mix,
                               win_dur=c["win_dur"], device_indices=[0], **kw)
    ref = [x[:, 1] for x in gi.e2e_pairs(c["seed"], c["n_ref"], c["seconds"], c["sr"])]
    cand = [x[:, 1] for x in gi.e2e_pairs(c["seed"] + 1, c["n_cand"], c["seconds"], c["sr"], stem_gain=1.3)]
    results = []
    for metrics, kw in ((["fad", "kd", "prdc"], {}), (["fad", "kd", "prdc", "kad"], {}), (["kad"], {"kad_scale": 1.0, "kad_bandwidth": 3.0})):
        m = make(metrics, **kw)
        m.add_reference(ref)
        results.append((m.evaluate(cand), m))
    (plain, _), (with_kad, m_kad), (alone, _) = results
    kad_keys = ["kad", "kad_mmd2", "kad_bandwidth"]
    assert [k for k in with_kad if k not in kad_keys] == list(plain)
    for key, value in plain.items():
        assert with_kad[key] == value, key                               # bit-equal: no existing path changed
    assert all(np.isfinite(with_kad[k]) for k in kad_keys)
    direct = am.kernel_audio_distance(m_kad._embed(cand, "candidate")[am.ItemCategory.stem], m_kad.stem_reference)
    assert {k: with_kad[k] for k in kad_keys} == direct
    assert list(alone) == kad_keys and alone["kad_bandwidth"] == 3.0 and alone["kad"] == alone["kad_mmd2"]
