"""The pair-dependence sweep on the device (csrc/pair_dependence.hip through hip_ops.pair_dependence) and its two front ends.

  1  values: the five row sums and their totals within 1e-12 x mean |value| of the f64 oracle (tests/dependence_reference.py)
     on exact data, for the three kinds, at the shapes that cross the engine's edges (a single tile of 4 rows, row and
     inner-dimension tails on either side, Dx != Dy both ways, a plan of two Q tiles per chunk); within MARGIN x the
     emulated error on real-valued rows
  2  cross-checks through the existing kernels: sum A_i is the XX sum of mmd_multi_sums, the Gaussian A_i the XX row sums of
     mmd_rbf_row_sums, sum H_i of two Gaussian kernels the XX sum of mmd_rbf_sums on the concatenated rows
  3  determinism and independence: two calls give the same bits, swapping the sets swaps the columns exactly, perm = identity
     is no perm, a seeded perm is a call on the gathered copy - all bit for bit
  4  non-finite rows and bad perm entries are counted and make the figures NaN
  5  distance_correlation and kernel_alignment end to end against the oracle, the `groups` null against a host recomputation"""
import warnings

import numpy as np
import pytest
import torch

import dependence_reference as dr
import inputs as gi
import kad_reference as ka
import kd_reference as kr

pytestmark = pytest.mark.gpu

EXACT = 1e-12
DEV = "cuda:0"
SIGMA = 10.0
BW2 = SIGMA * SIGMA
# (n, Dx, Dy); the last: 17 tiles -> 9 chunks of 2 Q tiles, the last one of a single tile
SHAPES = [(4, 32, 32), (129, 100, 36), (128, 64, 64), (257, 64, 512), (300, 512, 100), (2100, 32, 40)]


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


def exact_pair(n, dx, dy):
    rng = np.random.default_rng(n * 7 + dx * 3 + dy)
    return kr.rbf_rows(rng, n, dx, SIGMA), kr.rbf_rows(rng, n, dy, SIGMA)


@pytest.fixture(scope="module")
def exact_sets():
    """shape -> (x, y): computed once, read by every test that needs them."""
    return {s: exact_pair(*s) for s in SHAPES}


def call(ops, xt, yt, kind, bw2x=BW2, bw2y=BW2, perm=None):
    return ops.pair_dependence(xt, yt, kind, bw2x=bw2x, bw2y=bw2y, perm=perm)


# ---------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("shape", SHAPES)
def test_row_sums_on_exact_data(ops, exact_sets, shape):
    n = shape[0]
    x, y = exact_sets[shape]
    xt, yt = dev(x), dev(y)
    for kind in dr.KINDS:
        rows, sums = (t.cpu().numpy() for t in call(ops, xt, yt, kind))
        want = dr.row_sums(dr.pair_matrix(x, kind, BW2), dr.pair_matrix(y, kind, BW2))
        assert rows.shape == (n, 5) and sums.shape == (8,) and sums[6] == n and sums[7] == 0
        scale = np.abs(want).mean(0)
        err = np.abs(rows - want).max(0)
        tot_want = np.array([*want.sum(0), want[:, 0] @ want[:, 1]])
        tot_err = np.abs(sums[:6] - tot_want)
        print(f"{shape} {kind}: mean |row sum| {scale} largest |err| {err} = {err / scale / EXACT} of the limit; totals {tot_err / np.abs(tot_want) / EXACT}")
        assert (scale > 0).all() and (err <= EXACT * scale).all(), (shape, kind, err, scale)
        assert (tot_err <= EXACT * np.abs(tot_want)).all(), (shape, kind, sums[:6], tot_want)


@pytest.fixture(scope="module")
def real_sets():
    """(rows, d) -> (x, y, bw2x, bw2y, per kind: f64 row sums, emulated row sums): computed once."""
    out = {}
    for rows, seed, d in (("randn", 864, 64), ("unit", 1312, 512)):   # the sets of test_gpu_kad.py's test_sums_on_real_valued_rows
        y, x = gi.pair(rows, seed, 1000, 1000, d)
        bw = []
        for s in (x, y):
            pairs = ka.pair_values(s)
            bw.append(float(ka.as_key(pairs[ka.lower_median_rank(len(pairs))])))
        sums = {}
        for kind in dr.KINDS:
            want = dr.row_sums(dr.pair_matrix(x, kind, bw[0]), dr.pair_matrix(y, kind, bw[1]))
            emu = dr.row_sums(dr.pair_matrix(x, kind, bw[0], kr.emulated_dots("f32")), dr.pair_matrix(y, kind, bw[1], kr.emulated_dots("f32")))
            sums[kind] = (want, emu)
        out[(rows, d)] = (x, y, bw[0], bw[1], sums)
    return out


@pytest.mark.parametrize("rows, d", [("randn", 64), ("unit", 512)])
def test_row_sums_on_real_valued_rows(ops, real_sets, rows, d):
    """Each of the five row sums (as a share of its column's mean |value|) and each total (relative) within MARGIN x the
    LARGEST of the five emulated errors of its kind (the f32 dot products rounded once per 32-element slab,
    kd_reference.emulated_dots; MARGIN covers the matrix cores' rounding after every product) - the largest of the five, not
    each sum's own, as test_sums_on_real_valued_rows of test_gpu_mmd_multi.py argues: a single sum's emulated error can cancel
    by accident.  The measured shares are printed and kept in profiles/dependence/accuracy.txt."""
    x, y, bwx, bwy, sums = real_sets[(rows, d)]
    xt, yt = dev(x), dev(y)
    report = []
    for kind in dr.KINDS:
        want, emu = sums[kind]
        got_rows, got_sums = (t.cpu().numpy() for t in call(ops, xt, yt, kind, bwx, bwy))
        scale = np.abs(want).mean(0)
        limit = kr.MARGIN * float((np.abs(emu - want).max(0) / scale).max())
        err = np.abs(got_rows - want).max(0) / scale
        tot_limit = kr.MARGIN * float((np.abs(emu.sum(0) - want.sum(0)) / np.abs(want.sum(0))).max())
        tot_err = np.abs(got_sums[:5] - want.sum(0)) / np.abs(want.sum(0))
        print(f"{rows} D={d} {kind}: row sums {kr.MARGIN * err / limit} of the {kr.MARGIN:.0f} allowed (limit {limit:.3e}); totals "
              f"{kr.MARGIN * tot_err / tot_limit} of the {kr.MARGIN:.0f} allowed (limit {tot_limit:.3e})")
        report.append((kind, err, limit, tot_err, tot_limit))
    for kind, err, limit, tot_err, tot_limit in report:
        assert (err <= limit).all(), (rows, d, kind, err, limit)
        assert (tot_err <= tot_limit).all(), (rows, d, kind, tot_err, tot_limit)


# ---------------------------------------------------------------------------------------------------- 2. cross-checks
@pytest.mark.parametrize("shape", [(129, 100, 36), (300, 512, 100), (2100, 32, 40)])
def test_totals_and_gaussian_rows_through_the_existing_kernels(ops, exact_sets, shape):
    x, y = exact_sets[shape]
    xt, yt = dev(x), dev(y)
    for kind in dr.KINDS:
        rows, sums = call(ops, xt, yt, kind)
        sums = sums.cpu().numpy()
        for side, t in ((0, xt), (1, yt)):
            xx = ops.mmd_multi_sums(t, t, kind, (1.0,), bw2=BW2, blocks=ops.MMD_XX)[0, 0].item()
            xx = -xx if kind == "energy" else xx                          # the kernel sums' energy kernel is -d
            assert abs(sums[side] - xx) <= 1e-14 * abs(xx), (shape, kind, side, sums[side], xx)     # the same values in another order
        if kind == "gaussian":
            for side, t in ((0, xt), (1, yt)):
                w = ops.mmd_rbf_row_sums(t, t, gamma=0.5 / BW2, blocks=ops.MMD_XX)[0][:, 0].cpu().numpy()
                got = rows[:, side].cpu().numpy()
                assert (np.abs(got - w) <= 1e-14 * np.abs(w)).all(), (shape, side, np.abs(got - w).max())


def test_gaussian_product_is_one_gaussian_on_concatenated_rows(ops, real_sets):
    """exp(-d2x g_x) exp(-d2y g_y) = exp(-|z_i - z_j|^2 / 2) on z = [x sqrt(2 g_x) | y sqrt(2 g_y)].  bw2 = 64 on both sides
    makes sqrt(2 g) = 1 / 8: the scaled rows are exact.  Both values are device values in the f32-dot arithmetic; they agree
    within MARGIN x the largest relative emulated error of the five totals at these bandwidths."""
    x, y = real_sets[("randn", 64)][:2]
    xt, yt = dev(x), dev(y)
    _, sums = call(ops, xt, yt, "gaussian", 64.0, 64.0)
    z = torch.cat([xt * 0.125, yt * 0.125], dim=1).contiguous()
    whole = ops.mmd_rbf_sums(z, z, gamma=0.5, blocks=ops.MMD_XX)[0].item()
    want = dr.row_sums(dr.pair_matrix(x, "gaussian", 64.0), dr.pair_matrix(y, "gaussian", 64.0)).sum(0)
    emu = dr.row_sums(dr.pair_matrix(x, "gaussian", 64.0, kr.emulated_dots("f32")), dr.pair_matrix(y, "gaussian", 64.0, kr.emulated_dots("f32"))).sum(0)
    limit = kr.MARGIN * float((np.abs(emu - want) / np.abs(want)).max())
    got = sums[2].item()
    print(f"sum H {got!r} concatenated {whole!r} oracle {want[2]!r}: relative difference {abs(got - whole) / abs(whole):.3e} limit {limit:.3e} "
          f"= {kr.MARGIN * abs(got - whole) / abs(whole) / limit:.2f} of the {kr.MARGIN:.0f} allowed")
    assert abs(got - whole) <= limit * abs(whole), (got, whole, limit)


# ---------------------------------------------------------------------------------------------------- 3. determinism
@pytest.mark.parametrize("shape", [(129, 100, 36), (257, 64, 512), (2100, 32, 40)])
def test_bits(ops, exact_sets, shape):
    n = shape[0]
    x, y = exact_sets[shape]
    xt, yt = dev(x), dev(y)
    rng = np.random.default_rng(n)
    perm = dev(rng.permutation(n).astype(np.int64))
    gathered = yt[perm].contiguous()
    for kind in dr.KINDS:
        rows, sums = call(ops, xt, yt, kind, BW2, 1.5 * BW2)
        again = call(ops, xt, yt, kind, BW2, 1.5 * BW2)
        assert torch.equal(rows, again[0]) and torch.equal(sums, again[1]), (shape, kind, "two calls")
        srows, ssums = call(ops, yt, xt, kind, 1.5 * BW2, BW2)
        assert torch.equal(srows, rows[:, [1, 0, 2, 4, 3]]), (shape, kind, "swapped rows")
        assert torch.equal(ssums, sums[[1, 0, 2, 4, 3, 5, 6, 7]]), (shape, kind, "swapped sums")
        ident = call(ops, xt, yt, kind, BW2, 1.5 * BW2, perm=torch.arange(n, device=DEV))
        assert torch.equal(ident[0], rows) and torch.equal(ident[1], sums), (shape, kind, "identity perm")
        through = call(ops, xt, yt, kind, BW2, 1.5 * BW2, perm=perm)
        copied = call(ops, xt, gathered, kind, BW2, 1.5 * BW2)
        assert torch.equal(through[0], copied[0]) and torch.equal(through[1], copied[1]), (shape, kind, "perm")
        assert not torch.equal(through[0][:, 2], rows[:, 2])
        # the bandwidth fed from the device or from the host: the same bits
        if kind != "energy":
            fed = ops.pair_dependence(xt, yt, kind, bw2x=torch.tensor(BW2, dtype=torch.float32, device=DEV),
                                      bw2y=torch.tensor(1.5 * BW2, dtype=torch.float32, device=DEV))
            assert torch.equal(fed[0], rows) and torch.equal(fed[1], sums)


def test_duplicated_rows_stay_each_others_pairs(ops):
    """i = j is dropped by index, not by distance: two equal rows are a pair at distance 0 (k = 1)."""
    rng = np.random.default_rng(5)
    x = kr.rbf_rows(rng, 6, 32, SIGMA)
    x[3] = x[1]
    y = kr.rbf_rows(rng, 6, 32, SIGMA)
    rows, _ = call(ops, dev(x), dev(y), "gaussian")
    want = dr.row_sums(dr.pair_matrix(x, "gaussian", BW2), dr.pair_matrix(y, "gaussian", BW2))
    assert (np.abs(rows.cpu().numpy() - want) <= EXACT * np.abs(want).mean(0)).all()
    assert dr.pair_matrix(x, "gaussian", BW2)[1, 3] == 1.0


# ---------------------------------------------------------------------------------------------------- 4. non-finite rows
def test_non_finite_rows_are_counted(am, ops, exact_sets):
    x, y = exact_sets[(129, 100, 36)]
    bad_x, bad_y = x.copy(), y.copy()
    bad_x[5, 99] = np.nan
    bad_y[128, 0] = np.inf
    for kind in dr.KINDS:
        rows, sums = call(ops, dev(bad_x), dev(bad_y), kind)
        assert sums[6].item() == 127 and sums[7].item() == 2, (kind, sums)
        assert torch.isnan(rows).all() and torch.isnan(sums[:6]).all(), kind     # every row pairs with the bad rows
    # an entry of perm outside [0, n) is never dereferenced: it counts as a non-finite row of the y side (what only x enters stays finite)
    perm = torch.arange(129, device=DEV)
    perm[3], perm[77] = 129, -1
    rows, sums = call(ops, dev(x), dev(y), "energy", perm=perm)
    assert sums[7].item() == 2 and torch.isnan(sums[[1, 2, 4, 5]]).all() and torch.isfinite(sums[[0, 3]]).all()
    assert torch.equal(rows[:, [0, 3]], call(ops, dev(x), dev(y), "energy")[0][:, [0, 3]])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = am.distance_correlation(dev(bad_x), dev(y), n_permutations=2)
        hs = am.kernel_alignment(dev(x), dev(bad_y), bandwidth_x=SIGMA, bandwidth_y=SIGMA)
    assert len(w) == 2 and all(issubclass(i.category, RuntimeWarning) and "1 of 129" in str(i.message) for i in w), [str(i.message) for i in w]
    assert got["dcor_rows_nonfinite"] == 1 and all(np.isnan(got[k]) for k in ("dcov2", "dvar_x", "dvar_y", "dcor", "dcor_v", "dcor_p_value",
                                                                             "dcor_p_value_permutation"))
    assert hs["hsic_rows_nonfinite"] == 1 and np.isnan(hs["hsic"]) and np.isnan(hs["cka"])


# ---------------------------------------------------------------------------------------------------- 5. front ends
def data_of(am, rows, step=97):
    s = am.AudioMetricsData(True, device=DEV)
    for k in range(0, len(rows), step):
        s.add(dev(rows[k:k + step]))
    return s


def terms_size(a, b):
    n = a.shape[0]
    return np.abs(a * b).sum() / (n * (n - 3.0))


def test_distance_correlation_against_the_oracle(am, exact_sets):
    """U is a sum of three terms of about one size: S within EXACT of it, C and T_a T_b - products of two sums each within
    EXACT - within 2 EXACT: 5 EXACT x the size of the terms."""
    shape = (300, 512, 100)
    n = shape[0]
    x, y = exact_sets[shape]
    y = (y + x[:, :100] * np.float32(0.5)).astype(np.float32)              # dependent on purpose (exact: halves of exact values)
    a, b = dr.pair_matrix(x, "energy"), dr.pair_matrix(y, "energy")
    want = dr.statistics(a, b)
    groups = np.repeat(np.arange(30), 10)
    got = am.distance_correlation(data_of(am, x), data_of(am, y), groups=groups, n_permutations=9, seed=4, return_rows=True)
    for key, w, size in (("dcov2", want["u_ab"], terms_size(a, b)), ("dvar_x", want["u_aa"], terms_size(a, a)),
                         ("dvar_y", want["u_bb"], terms_size(b, b))):
        print(f"{key}: {got[key]!r} oracle {w!r} limit {5 * EXACT * size:.3e}")
        assert abs(got[key] - w) <= 5 * EXACT * size
    ratio = want["u_ab"] / np.sqrt(want["u_aa"] * want["u_bb"])
    assert abs(got["dcor"] - ratio) <= 1e-9 and 0.0 < got["dcor"] < 1.0
    from scipy import stats                                               # the t-test from the ORACLE's ratio
    dof = n * (n - 3) / 2.0 - 1.0
    t = np.sqrt(dof) * ratio / np.sqrt(1.0 - ratio * ratio)
    want_p = float(stats.t.sf(t, dof))
    print(f"dcor {got['dcor']!r} oracle {ratio!r}; t {got['dcor_t']!r} oracle {t!r}; p {got['dcor_p_value']!r} oracle {want_p!r}")
    assert abs(got["dcor_t"] - t) <= 1e-8 * t and abs(got["dcor_p_value"] - want_p) <= 1e-6 * want_p
    assert abs(got["dcor_v"] - want["v_ab"] / np.sqrt(want["v_aa"] * want["v_bb"])) <= 1e-9
    assert got["dcor_rows"] == n and got["dcor_rows_nonfinite"] == 0 and got["dcor_dof"] == n * (n - 3) / 2.0 - 1.0
    assert abs(got["row_dependence"].mean() - got["dcov2"]) <= 1e-12 * terms_size(a, b)
    assert (np.abs(got["row_sums"] - dr.row_sums(a, b)) <= EXACT * np.abs(dr.row_sums(a, b)).mean(0)).all()
    # the song-level null against a host recomputation of every labelling
    perms, movable, fixed = am.dependence_permutations(n, groups, 9, seed=4)
    null = np.array([dr.u_statistic(a, b[np.ix_(p, p)]) for p in perms])
    assert (got["units_movable"], got["units_fixed"], got["dcor_n_permutations"]) == (30, 0, 9) == (movable, fixed, 9)
    assert got["dcor_p_value_permutation"] == (1.0 + np.count_nonzero(null >= want["u_ab"])) / 10.0 == 0.1
    assert abs(got["dcor_null_mean"] - null.mean()) <= 5 * EXACT * terms_size(a, b)
    assert abs(got["dcor_null_std"] - null.std(ddof=1)) <= 1e-9 * null.std(ddof=1)
    # tensors are taken as they are
    plain = am.distance_correlation(dev(x), dev(y))
    assert plain["dcov2"] == got["dcov2"] and plain["dcor"] == got["dcor"] and "dcor_p_value_permutation" not in plain


@pytest.mark.parametrize("kernel", ["gaussian", "laplacian"])
def test_kernel_alignment_against_the_oracle(am, exact_sets, kernel):
    shape = (257, 64, 512)
    x, y = exact_sets[shape]
    bw2 = []
    for s in (x, y):
        pairs = ka.pair_values(s)
        bw2.append(float(ka.as_key(pairs[ka.lower_median_rank(len(pairs))])))
    cases = (({}, bw2), ({"bandwidth_x": 12.0, "bandwidth_y": 7.0}, [144.0, 49.0]), ({"bandwidth_y": 7.0}, [bw2[0], 49.0]))
    for kw, (bx, by) in cases:
        a, b = dr.pair_matrix(x, kernel, bx), dr.pair_matrix(y, kernel, by)
        want = dr.statistics(a, b)
        got = am.kernel_alignment(data_of(am, x), data_of(am, y), kernel=kernel, **kw)
        assert got["hsic_bandwidth_x"] == np.sqrt(bx) and got["hsic_bandwidth_y"] == np.sqrt(by) and got["hsic_kernel"] == kernel
        for key, w, size in (("hsic", want["u_ab"], terms_size(a, b)), ("hsic_xx", want["u_aa"], terms_size(a, a)),
                             ("hsic_yy", want["u_bb"], terms_size(b, b))):
            print(f"{kernel} {kw} {key}: {got[key]!r} oracle {w!r} limit {5 * EXACT * size:.3e}")
            assert abs(got[key] - w) <= 5 * EXACT * size
        assert abs(got["cka"] - want["u_ab"] / np.sqrt(want["u_aa"] * want["u_bb"])) <= 1e-8
    # the median of a set is computed once per content: the second call finds it on the set
    xs, ys = data_of(am, x), data_of(am, y)
    first = am.kernel_alignment(xs, ys, kernel=kernel, n_permutations=3, seed=1)
    calls = {"select": 0}
    real = am.hip_ops.pairwise_select_sq

    def counting(*a, **k):
        calls["select"] += 1
        return real(*a, **k)
    am.hip_ops.pairwise_select_sq = counting
    try:
        second = am.kernel_alignment(xs, ys, kernel=kernel, n_permutations=3, seed=1)
    finally:
        am.hip_ops.pairwise_select_sq = real
    assert calls["select"] == 0 and first == second and 0.0 < first["hsic_p_value_permutation"] <= 1.0 and first["units_movable"] == 257
