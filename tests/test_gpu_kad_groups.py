"""Per-group Kernel Audio Distance on the device (am_mmd_rbf_groups_f32 through hip_ops.mmd_rbf_group_sums, and
kernel_audio_distance_per_group) against the float64 oracle of tests/kad_groups_reference.py.

  1  exact data, gathered rows, groups that straddle the 128-row tiles: 1e-12 x mean |K| per group and per row
  2  the chunk seams: more than 16 reference tiles, a group of more than 16 tiles
  3  consistency with the whole-set kernels (one group = mmd_rbf_sums; the per-group cross sums add up to the whole-set one)
  4  bits: repeatability, stored order against list order, device-fed bandwidth
  5  real-valued rows against the emulated f32 dot products
  6  isolation of a NaN row and of an out-of-range index
  7  kernel_audio_distance_per_group end to end: values, label order, sizes, stored-order rows, the reference cache"""
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
SIZES = [2, 3, 31, 32, 33, 127, 128, 129, 300]          # 785 rows: groups end before, on and after the tile edges


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


def shuffled_store(x_list, seed):
    """(store, idx): the list-ordered rows scattered over a store by a seeded permutation; store[idx] == x_list."""
    idx = np.random.default_rng(seed).permutation(len(x_list)).astype(np.int64)
    store = np.empty_like(x_list)
    store[idx] = x_list
    return store, idx


def group_sums(ops, store, idx, offs, y, rows=True, **width):
    """the device call, checked and read back: (out_groups [B, 2], out_rows [n, 2] or None)"""
    res = ops.mmd_rbf_group_sums(store, idx, [int(o) for o in offs], y, rows=rows, **width)
    res[-1]()
    out = res[0]
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(offs) - 1, 2) and out.is_cuda
    if rows:
        assert res[1].dtype == torch.float64 and tuple(res[1].shape) == (int(offs[-1]), 2)
    return out.cpu().numpy(), res[1].cpu().numpy() if rows else None


def assert_within(got_groups, got_rows, offs, m, want, limit, what):
    """every normalised per-group sum and every normalised row sum within `limit` of the oracle"""
    sizes = np.diff(offs)
    xx, xy = kg.device_means(got_groups, sizes, m)
    many = sizes > 1
    err_xx, err_xy = np.abs(xx - want["mean_xx"])[many], np.abs(xy - want["mean_xy"])
    print(f"{what}: max |err| xx {err_xx.max() if many.any() else 0.0:.3e} xy {err_xy.max():.3e} limit {limit:.3e}")
    assert (err_xx <= limit).all() and (err_xy <= limit).all(), (what, xx, want["mean_xx"], xy, want["mean_xy"], limit)
    assert (got_groups[~many, 0] == 0.0).all()                        # a group of one row has no pair
    if got_rows is not None:
        per_row = np.repeat(sizes, sizes)
        wr, cr = kg.row_means(got_rows, offs, m)
        want_w, want_c = kg.row_means(np.stack([want["w"], want["c"]], axis=1), offs, m)
        err_w, err_c = np.abs(wr - want_w)[per_row > 1], np.abs(cr - want_c)
        print(f"{what}: rows max |err| w {err_w.max() if len(err_w) else 0.0:.3e} c {err_c.max():.3e}")
        assert (err_w <= limit).all() and (err_c <= limit).all(), what


# ---------------------------------------------------------------------------------------------------- 1. exact data
@pytest.fixture(scope="module")
def exact_cases():
    out = {}
    for d in (32, 100, 512):
        rng = np.random.default_rng(4100 + d)
        x_list, y = kr.rbf_rows(rng, sum(SIZES), d, SIGMA), kr.rbf_rows(rng, 300, d, SIGMA)
        offs = kg.offsets_of(SIZES)
        store, idx = shuffled_store(x_list, 4200 + d)
        out[d] = dict(x_list=x_list, y=y, offs=offs, store=store, idx=idx, want=kg.group_sums(x_list, offs, y, GAMMA))
    return out


@pytest.mark.parametrize("d", [32, 100, 512])
def test_exact_data_through_a_true_gather(ops, exact_cases, d):
    c = exact_cases[d]
    assert 0.01 < c["want"]["scale"] < 0.99                          # K spreads over (0, 1)
    assert not (c["idx"] == np.arange(len(c["idx"]))).all()
    groups, rows = group_sums(ops, dev(c["store"]), dev(c["idx"]), c["offs"], dev(c["y"]), gamma=GAMMA)
    assert_within(groups, rows, c["offs"], 300, c["want"], EXACT * c["want"]["scale"], f"D={d}")
    # without out_rows: the same group records
    only, none = group_sums(ops, dev(c["store"]), dev(c["idx"]), c["offs"], dev(c["y"]), rows=False, gamma=GAMMA)
    assert none is None and np.array_equal(only, groups)


# ---------------------------------------------------------------------------------------------------- 2. chunk seams
def test_chunk_seams(ops):
    """2 100 reference rows are 17 tiles, so every row's cross sum is put together from the partials of several chunks, and
    a group of 2 100 rows makes a within range of 17 tiles - more than one chunk of 16 - beside P tiles whose range is a
    single tile."""
    d, m, sizes = 32, 2100, [2, 2100, 50]
    rng = np.random.default_rng(4300)
    x_list, y = kr.rbf_rows(rng, sum(sizes), d, SIGMA), kr.rbf_rows(rng, m, d, SIGMA)
    offs = kg.offsets_of(sizes)
    want = kg.group_sums(x_list, offs, y, GAMMA)
    store, idx = shuffled_store(x_list, 4301)
    groups, rows = group_sums(ops, dev(store), dev(idx), offs, dev(y), gamma=GAMMA)
    assert_within(groups, rows, offs, m, want, EXACT * want["scale"], "chunk seams")


# ---------------------------------------------------------------------------------------------------- 3. consistency
def test_one_group_equals_the_whole_set_sums(am, ops, exact_cases):
    c = exact_cases[100]
    n, m = len(c["x_list"]), 300
    xt, yt = dev(c["x_list"]), dev(c["y"])
    scale = c["want"]["scale"]
    whole = ops.mmd_rbf_sums(xt, yt, gamma=GAMMA).cpu().numpy()
    one, _ = group_sums(ops, xt, None, [0, n], yt, rows=False, gamma=GAMMA)
    xx, xy = kg.device_means(one, [n], m)
    ref = ka.device_means(whole, n, m)
    print(f"one group: xx {xx[0]!r} / {ref[0]!r}, xy {xy[0]!r} / {ref[2]!r}, limit {EXACT * scale:.3e}")
    assert abs(xx[0] - ref[0]) <= EXACT * scale and abs(xy[0] - ref[2]) <= EXACT * scale
    # any grouping: the cross sums of the groups add up to the whole-set one
    groups, _ = group_sums(ops, xt, None, c["offs"], yt, rows=False, gamma=GAMMA)
    assert abs(groups[:, 1].sum() / (float(n) * m) - ref[2]) <= EXACT * scale
    # the front end with one label for every row = kernel_audio_distance on the same sets
    def data(rows):
        s = am.AudioMetricsData(True, device=DEV)
        s.add(dev(rows))
        return s
    ref_set = data(c["y"])
    kad = am.kernel_audio_distance(data(c["x_list"]), ref_set, scale=1000.0)
    per = am.kernel_audio_distance_per_group(data(c["x_list"]), ref_set, np.full(n, 7), scale=1000.0)
    print(f"kad {kad['kad']!r} per group {per['kad_per_group'][0]!r}")
    assert per["kad_bandwidth"] == kad["kad_bandwidth"] and per["group_labels"].tolist() == [7] and per["group_sizes"].tolist() == [n]
    bw_scale = kg.group_sums(c["x_list"], [0, n], c["y"], 0.5 / kad["kad_bandwidth"] ** 2)["scale"]
    assert abs(per["kad_per_group"][0] - kad["kad"]) <= EXACT * bw_scale * 1000.0
    assert per["kad_per_group"][0] == 1000.0 * per["kad_mmd2_per_group"][0]


# ---------------------------------------------------------------------------------------------------- 4. bits
def test_bits(ops, exact_cases):
    c = exact_cases[100]
    store, idx, yt = dev(c["store"]), dev(c["idx"]), dev(c["y"])
    offs = [int(o) for o in c["offs"]]
    first = ops.mmd_rbf_group_sums(store, idx, offs, yt, gamma=GAMMA, rows=True)
    again = ops.mmd_rbf_group_sums(store, idx, offs, yt, gamma=GAMMA, rows=True)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    # the result depends on the list order only: the same list as stored rows in group order, no index list
    ordered = ops.mmd_rbf_group_sums(dev(c["x_list"]), None, offs, yt, gamma=GAMMA, rows=True)
    assert torch.equal(first[0], ordered[0]) and torch.equal(first[1], ordered[1])
    # ... and as a row view with another leading dimension
    wide = torch.full((len(c["store"]), 112), 1e30, dtype=torch.float32, device=DEV)      # the padding must never be read as data
    wide[:, :100] = store
    view = ops.mmd_rbf_group_sums(wide[:, :100], idx, offs, yt, gamma=GAMMA, rows=True)
    assert torch.equal(first[0], view[0]) and torch.equal(first[1], view[1])
    # the bandwidth from device memory: gamma = 0.5 / (double)bw2 formed on the device = the same host expression
    bw2 = np.float32(SIGMA * SIGMA * 1.0009765625)
    fed = ops.mmd_rbf_group_sums(store, idx, offs, yt, bw2=torch.tensor(bw2, dtype=torch.float32, device=DEV), rows=True)
    host = ops.mmd_rbf_group_sums(store, idx, offs, yt, gamma=0.5 / float(bw2), rows=True)
    assert torch.equal(fed[0], host[0]) and torch.equal(fed[1], host[1])
    assert not torch.equal(fed[0], first[0])
    for r in (first, again, ordered, view, fed, host):
        r[-1]()


# ---------------------------------------------------------------------------------------------------- 5. real-valued rows
@pytest.mark.parametrize("kind, d", [("randn", 64), ("unit", 512)])
def test_real_valued_rows(ops, kind, d):
    """Each normalised per-group sum within MARGIN x the LARGEST emulated error of that statistic over the groups (the
    rounding_tolerance form of kd_reference: the f32 dot products rounded once per 32-element slab; MARGIN covers the
    matrix cores' rounding after every product; a single group's emulated error can cancel by accident).  1 000 candidate
    rows: 17 groups of 50, one of 128 and the 22 rows that remain."""
    n = m = 1000
    sizes = [50] * 9 + [128] + [50] * 8 + [22]
    assert sum(sizes) == n
    y, x = gi.pair(kind, 900 + d, m, n, d)
    pairs = ka.pair_values(y)
    gamma = 0.5 / float(pairs[ka.lower_median_rank(len(pairs))])     # the kernel width KAD itself would take
    offs = kg.offsets_of(sizes)
    want = kg.group_sums(x, offs, y, gamma)
    emulated = kg.group_sums(x, offs, y, gamma, dots=kr.emulated_dots("f32"))
    groups, _ = group_sums(ops, dev(x), None, offs, dev(y), rows=False, gamma=gamma)
    xx, xy = kg.device_means(groups, sizes, m)
    failures = []
    for name, got, key in (("xx", xx, "mean_xx"), ("xy", xy, "mean_xy")):
        limit = kr.MARGIN * float(np.max(np.abs(emulated[key] - want[key])))
        for b in range(len(sizes)):
            err = abs(got[b] - want[key][b])
            print(f"{kind} D={d} {name} group {b} (n={sizes[b]}): device {got[b]!r} oracle {want[key][b]!r} |err| {err:.3e} limit {limit:.3e}")
            if not err <= limit:
                failures.append((name, b, got[b], want[key][b], err, limit))
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------- 6. isolation
def test_a_nan_row_stays_in_its_group(ops, exact_cases):
    c = exact_cases[100]
    offs = [int(o) for o in c["offs"]]
    yt, idx = dev(c["y"]), dev(c["idx"])
    clean, clean_rows = group_sums(ops, dev(c["store"]), idx, offs, yt, gamma=GAMMA)
    victim = 5                                                        # the group of 127 rows
    pos = offs[victim] + 60
    bad = c["store"].copy()
    bad[c["idx"][pos], 17] = np.nan
    got, got_rows = group_sums(ops, dev(bad), idx, offs, yt, gamma=GAMMA)
    assert np.isnan(got[victim]).all()
    others = [b for b in range(len(SIZES)) if b != victim]
    assert np.array_equal(got[others], clean[others])                # bit-identical: float64 == on finite values
    inside = np.arange(offs[victim], offs[victim + 1])
    outside = np.setdiff1d(np.arange(offs[-1]), inside)
    assert np.array_equal(got_rows[outside], clean_rows[outside])
    assert np.isnan(got_rows[pos]).all() and np.isnan(got_rows[inside, 0]).all()       # every row of the group has the NaN row as a partner
    assert np.array_equal(np.delete(got_rows[inside, 1], 60), np.delete(clean_rows[inside, 1], 60))   # ... but not in its cross sum


def test_an_out_of_range_index_is_reported_and_isolated(ops, exact_cases):
    c = exact_cases[100]
    offs = [int(o) for o in c["offs"]]
    store, yt = dev(c["store"]), dev(c["y"])
    clean, _ = group_sums(ops, store, dev(c["idx"]), offs, yt, rows=False, gamma=GAMMA)
    victim = 4                                                        # the group of 33 rows
    for bad_value in (len(c["store"]), -1, 2 ** 40):
        idx = c["idx"].copy()
        pos = offs[victim] + 9
        idx[pos] = bad_value
        out, check = ops.mmd_rbf_group_sums(store, dev(idx), offs, yt, gamma=GAMMA)
        with pytest.raises(ValueError, match=r"idx\[%d\] = %d is outside \[0, %d\)" % (pos, bad_value, len(c["store"]))):
            check()
        got = out.cpu().numpy()
        others = [b for b in range(len(SIZES)) if b != victim]
        assert np.array_equal(got[others], clean[others])
        # the row counts as zeros: the oracle on the list with that row zeroed
        x_zero = c["x_list"].copy()
        x_zero[pos] = 0.0
        want = kg.group_sums(x_zero, c["offs"], c["y"], GAMMA)
        xx, xy = kg.device_means(got, SIZES, 300)
        assert abs(xx[victim] - want["mean_xx"][victim]) <= EXACT * want["scale"] and abs(xy[victim] - want["mean_xy"][victim]) <= EXACT * want["scale"]


# ---------------------------------------------------------------------------------------------------- 7. end to end
def data_of(am, rows, steps=(97, 31, 150)):
    """an AudioMetricsData filled in batches of uneven size"""
    s = am.AudioMetricsData(True, device=DEV)
    k, i = 0, 0
    while k < len(rows):
        s.add(dev(rows[k:k + steps[i % len(steps)]]))
        k += steps[i % len(steps)]
        i += 1
    return s


def oracle_per_group(x, labels, y, bw2=None):
    """oracle values in ascending label order: (labels, sizes, mmd2 [B], c / m per STORED row, scale, bw2)"""
    if bw2 is None:
        p = ka.pair_values(y)
        bw2 = float(ka.as_key(p[ka.lower_median_rank(len(p))]))
    order = np.argsort(labels, kind="stable")
    uniq, sizes = np.unique(labels, return_counts=True)
    offs = kg.offsets_of(sizes)
    g = kg.group_sums(x[order], offs, y, 0.5 / bw2)
    means, _ = ka.mmd_parts(y[:2], y, 0.5 / bw2)
    cross = np.empty(len(x))
    cross[order] = g["c"] / len(y)
    return uniq, sizes, kg.mmd2_per_group(g["mean_xx"], g["mean_xy"], means[1]), cross, g["scale"], bw2


def test_per_group_end_to_end(am, monkeypatch):
    rng = np.random.default_rng(4700)
    n, m, d = 400, 513, 100
    x, y, more = kr.rbf_rows(rng, n, d, SIGMA), kr.rbf_rows(rng, m, d, SIGMA), kr.rbf_rows(rng, 130, d, SIGMA)
    labels = rng.choice(np.array([-5, 3, 11, 12, 40, 1000]), size=n, p=[0.3, 0.05, 0.3, 0.2, 0.1, 0.05])
    labels[123] = 77                                                  # one group of a single row
    assert (labels == 77).sum() == 1
    calls = {"select": 0, "yy": 0, "groups": 0}
    real_select, real_sums, real_groups = am.hip_ops.pairwise_select_sq, am.hip_ops.mmd_rbf_sums, am.hip_ops.mmd_rbf_group_sums

    def counting_select(*a, **k):
        calls["select"] += 1
        return real_select(*a, **k)

    def counting_sums(*a, **k):
        calls["yy"] += 1 if k.get("blocks", 7) & 2 else 0
        return real_sums(*a, **k)

    def counting_groups(*a, **k):
        calls["groups"] += 1
        return real_groups(*a, **k)
    monkeypatch.setattr(am.hip_ops, "pairwise_select_sq", counting_select)
    monkeypatch.setattr(am.hip_ops, "mmd_rbf_sums", counting_sums)
    monkeypatch.setattr(am.hip_ops, "mmd_rbf_group_sums", counting_groups)
    cand, ref = data_of(am, x), data_of(am, y)

    def checked(got, want_x, want_y, want_labels):
        uniq, sizes, mmd2, cross, scale, bw2 = oracle_per_group(want_x, want_labels, want_y)
        assert list(got) == ["kad_per_group", "kad_mmd2_per_group", "group_labels", "group_sizes", "kad_bandwidth", "row_cross_mean"]
        assert got["group_labels"].tolist() == uniq.tolist() and got["group_sizes"].tolist() == sizes.tolist()
        assert got["group_sizes"].dtype == np.int64 and got["kad_per_group"].dtype == np.float64
        assert got["kad_bandwidth"] == np.sqrt(bw2)
        single = sizes == 1
        assert single.sum() == 1 and np.isnan(got["kad_mmd2_per_group"][single]).all() and np.isnan(got["kad_per_group"][single]).all()
        err = np.abs(got["kad_mmd2_per_group"] - mmd2)[~single]
        print(f"per group mmd2 max |err| {err.max():.3e} limit {3 * EXACT * scale:.3e}")
        assert (err <= 3 * EXACT * scale).all()                       # three statistics, each within the exact-data bound
        assert np.array_equal(got["kad_per_group"][~single], 100.0 * got["kad_mmd2_per_group"][~single])
        assert got["row_cross_mean"].shape == (len(want_x),) and (np.abs(got["row_cross_mean"] - cross) <= EXACT * scale).all()

    with pytest.warns(RuntimeWarning, match="1 of 7 groups hold a single row") as rec:
        first = am.kernel_audio_distance_per_group(cand, ref, labels, return_rows=True)
    assert len([r for r in rec if issubclass(r.category, RuntimeWarning)]) == 1
    checked(first, x, y, labels)
    assert calls == {"select": 1, "yy": 1, "groups": 1}
    # a second call, labels as a device tensor: neither the median nor Syy again, the same values
    with pytest.warns(RuntimeWarning):
        second = am.kernel_audio_distance_per_group(cand, ref, torch.as_tensor(labels).to(DEV), return_rows=True)
    assert calls == {"select": 1, "yy": 1, "groups": 2}
    for key in first:
        assert np.array_equal(np.asarray(first[key]), np.asarray(second[key]), equal_nan=True), key
    # the cache is the one kernel_audio_distance uses
    whole = am.kernel_audio_distance(cand, ref)
    assert calls["select"] == 1 and calls["yy"] == 1 and whole["kad_bandwidth"] == first["kad_bandwidth"]
    # without the single row and without return_rows: no warning, no row key
    keep = labels != 77
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        plain = am.kernel_audio_distance_per_group(data_of(am, x[keep]), ref, labels[keep], scale=1.0)
    assert "row_cross_mean" not in plain and np.array_equal(plain["kad_per_group"], plain["kad_mmd2_per_group"])
    assert calls["select"] == 1 and calls["yy"] == 1
    # a fixed bandwidth is honoured (its own Syy, no select)
    fixed = am.kernel_audio_distance_per_group(data_of(am, x[keep]), ref, labels[keep], bandwidth=3.0)
    uniq, sizes, mmd2, _, scale, _ = oracle_per_group(x[keep], labels[keep], y, bw2=9.0)
    assert fixed["kad_bandwidth"] == 3.0 and (np.abs(fixed["kad_mmd2_per_group"] - mmd2) <= 3 * EXACT * scale).all()
    assert calls["select"] == 1 and calls["yy"] == 2
    # an append to the reference: both recomputed for the grown set
    ref.add(dev(more))
    with pytest.warns(RuntimeWarning):
        grown = am.kernel_audio_distance_per_group(cand, ref, labels, return_rows=True)
    assert calls["select"] == 2 and calls["yy"] == 3
    checked(grown, x, np.concatenate([y, more]), labels)
