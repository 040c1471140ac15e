"""Multi-scale kernel sums on the device (csrc/mmd_multi.hip through hip_ops.mmd_multi_sums) and their two front ends.

  1  Gaussian bits: every scale of a call equals hip_ops.mmd_rbf_sums at gamma = 0.5 / (bw2 c c) bit for bit, the bandwidth
     fed from the device or from the host, on exact and on real-valued rows, at the shapes that cross the engine's edges and
     on a plan of two Q chunks; there the Laplacian and energy sums are additive over a split of the reference
  2  independence and determinism: a scale's sums depend neither on the other scales of the call, nor on their order, nor on
     where the grid is cut into calls; two calls give the same bits; the block mask writes only what it names
  3  values: 1e-12 x mean |K| on exact data against the f64 oracle (tests/mmd_multi_reference.py), MARGIN x the emulated
     error on real-valued rows; swapping the sets swaps XX and YY
  4  kernel_audio_distance_multiscale and energy_distance: the value of kernel_audio_distance at scale 1, the oracle, the
     reference-side cache and its invalidation, the errors"""
import numpy as np
import pytest
import torch

import inputs as gi
import kad_reference as ka
import kd_reference as kr
import mmd_multi_reference as mr

pytestmark = pytest.mark.gpu

EXACT = 1e-12
DEV = "cuda:0"
SIGMA = 10.0
BW2 = SIGMA * SIGMA
SHAPES = [(2, 2, 32), (129, 300, 100), (128, 128, 64), (257, 1000, 512)]
# (kind, scales) of the value tests
EXACT_GRIDS = [("gaussian", (0.5, 1.0, 2.0, 4.0)), ("laplacian", (0.5, 1.0, 2.0)), ("energy", (1.0,))]
REAL_GRIDS = [("gaussian", (0.25, 0.5, 1.0, 2.0, 4.0)), ("laplacian", (0.5, 1.0, 2.0)), ("energy", (1.0,))]


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


def exact_pair(n, m, d):
    rng = np.random.default_rng(n * 7 + m * 3 + d)                    # the sets of test_gpu_kad.py's exact_sets
    return kr.rbf_rows(rng, n, d, SIGMA), kr.rbf_rows(rng, m, d, SIGMA)


def randn_pair(n, m, d):
    rng = np.random.default_rng(n + 5 * m + 11 * d)
    return rng.standard_normal((n, d)).astype(np.float32), (rng.standard_normal((m, d)) * 1.1 + 0.1).astype(np.float32)


@pytest.fixture(scope="module")
def exact_sets():
    """shape -> (x, y, the three f64 d2 matrices): computed once, read by every test that needs them."""
    out = {}
    for n, m, d in SHAPES:
        x, y = exact_pair(n, m, d)
        out[(n, m, d)] = (x, y, mr.distances(x, y))
    return out


def gamma_of(bw2, c):
    return 0.5 / (bw2 * (c * c))


def means_of(sums, n, m):
    """[3, S] device sums -> [S, 3] normalised host means"""
    s = sums.cpu().numpy()
    return np.stack([ka.device_means(s[:, j], n, m) for j in range(s.shape[1])])


# ---------------------------------------------------------------------------------------------------- 1. Gaussian bits
@pytest.mark.parametrize("rows", ["exact", "randn"])
@pytest.mark.parametrize("shape", SHAPES)
def test_gaussian_sums_are_the_bits_of_mmd_rbf_sums(ops, shape, rows):
    n, m, d = shape
    x, y = exact_pair(n, m, d) if rows == "exact" else randn_pair(n, m, d)
    xt, yt = dev(x), dev(y)
    scales = (0.5, 1.0, 2.0, 4.0)
    bw2 = np.float32(BW2 * 1.0009765625)
    fed = ops.mmd_multi_sums(xt, yt, "gaussian", scales, bw2=torch.tensor(bw2, dtype=torch.float32, device=DEV))
    host = ops.mmd_multi_sums(xt, yt, "gaussian", scales, bw2=float(bw2))
    assert fed.dtype == torch.float64 and tuple(fed.shape) == (3, 4) and fed.is_cuda
    for j, c in enumerate(scales):
        want = ops.mmd_rbf_sums(xt, yt, gamma=gamma_of(float(bw2), c))
        for b in range(3):
            assert torch.equal(fed[b, j], want[b]), (shape, rows, "device bandwidth", c, b, fed[b, j].item(), want[b].item())
            assert torch.equal(host[b, j], want[b]), (shape, rows, "host bandwidth", c, b, host[b, j].item(), want[b].item())
    # c = 1 is the device's own expression of am_mmd_rbf_f32: 0.5 / (double)bw2
    own = ops.mmd_rbf_sums(xt, yt, bw2=torch.tensor(bw2, dtype=torch.float32, device=DEV))
    assert torch.equal(fed[:, 1], own)


def test_a_plan_of_two_chunks(ops):
    """65 x 65 tiles: kad_chunk gives 2 Q tiles per workgroup, 33 chunks, the last one of a single tile."""
    n = m = 8200
    rng = np.random.default_rng(41)
    xt, yt = dev(rng.standard_normal((n, 32)).astype(np.float32)), dev(rng.standard_normal((m, 32)).astype(np.float32))
    bw2, scales, xy = 64.0, (0.5, 1.0, 2.0, 4.0), ops.MMD_XY
    got = ops.mmd_multi_sums(xt, yt, "gaussian", scales, bw2=bw2, blocks=xy)
    for j, c in enumerate(scales):
        want = ops.mmd_rbf_sums(xt, yt, gamma=gamma_of(bw2, c), blocks=xy)
        assert torch.equal(got[2, j], want[2]), (c, got[2, j].item(), want[2].item())
    assert torch.isnan(got[:2]).all()
    for kind, grid in (("laplacian", (0.5, 1.0, 2.0)), ("energy", (1.0,))):
        whole = ops.mmd_multi_sums(xt, yt, kind, grid, bw2=bw2, blocks=xy)[2].cpu().numpy()
        halves = sum(ops.mmd_multi_sums(xt, part, kind, grid, bw2=bw2, blocks=xy)[2].cpu().numpy() for part in (yt[:4100], yt[4100:]))
        print(f"{kind}: whole {whole} halves {halves} relative {np.abs(whole - halves) / np.abs(whole)}")
        assert np.isfinite(whole).all() and (np.abs(whole) > 1.0).all()
        assert (np.abs(whole - halves) <= 1e-13 * np.abs(whole)).all(), (kind, whole, halves)


# ---------------------------------------------------------------------------------------------------- 2. independence
@pytest.mark.parametrize("kind", ["gaussian", "laplacian"])
def test_a_scale_does_not_depend_on_its_neighbours(ops, exact_sets, kind):
    x, y, _ = exact_sets[(129, 300, 100)]
    xt, yt = dev(x), dev(y)
    grid = (0.25, 0.5, 1.0, 2.0, 4.0, 8.0)
    full = ops.mmd_multi_sums(xt, yt, kind, grid, bw2=BW2)                  # two library calls: 4 + 2 scales
    assert tuple(full.shape) == (3, 6) and torch.isfinite(full).all()
    assert torch.equal(full, ops.mmd_multi_sums(xt, yt, kind, grid, bw2=BW2))       # two calls: the same bits
    for j, c in enumerate(grid):
        alone = ops.mmd_multi_sums(xt, yt, kind, (c,), bw2=BW2)
        assert torch.equal(alone[:, 0], full[:, j]), (kind, c, alone[:, 0].tolist(), full[:, j].tolist())
    back = ops.mmd_multi_sums(xt, yt, kind, grid[::-1], bw2=BW2)           # other neighbours, another cut: (8, 4, 2, 1) + (0.5, 0.25)
    assert torch.equal(back.flip(1), full)
    three = ops.mmd_multi_sums(xt, yt, kind, grid[1:4], bw2=BW2)            # the three-scale instantiation
    pair = ops.mmd_multi_sums(xt, yt, kind, grid[4:], bw2=BW2)              # and the two-scale one
    assert torch.equal(three, full[:, 1:4]) and torch.equal(pair, full[:, 4:])
    # the values differ between the scales: a column is its own scale's, not a copy
    assert len({full[2, j].item() for j in range(6)}) == 6


def test_energy_sums_repeat(ops, exact_sets):
    x, y, _ = exact_sets[(129, 300, 100)]
    xt, yt = dev(x), dev(y)
    first = ops.mmd_multi_sums(xt, yt, "energy", (1.0,))
    assert tuple(first.shape) == (3, 1) and torch.isfinite(first).all() and (first < 0).all()
    assert torch.equal(first, ops.mmd_multi_sums(xt, yt, "energy", (1.0,)))
    assert torch.equal(first, ops.mmd_multi_sums(xt, yt, "energy", (3.0,), bw2=7.0))      # neither the scale nor a bandwidth enters


@pytest.mark.parametrize("blocks", [1, 2, 4, 3, 5, 6])
def test_block_mask_writes_only_what_it_names(ops, exact_sets, blocks):
    x, y, _ = exact_sets[(129, 300, 100)]
    xt, yt = dev(x), dev(y)
    sentinel = -12345.5
    for kind, grid in (("gaussian", (0.5, 2.0)), ("laplacian", (0.5, 2.0)), ("energy", (1.0,))):
        full = ops.mmd_multi_sums(xt, yt, kind, grid, bw2=BW2)
        out = torch.full((3, len(grid)), sentinel, dtype=torch.float64, device=DEV)
        assert ops.mmd_multi_sums(xt, yt, kind, grid, bw2=BW2, blocks=blocks, out=out) is out
        for b in range(3):
            if blocks & (1 << b):
                assert torch.equal(out[b], full[b]), (kind, b)             # and the value does not depend on the mask
            else:
                assert (out[b] == sentinel).all(), (kind, b)


# ---------------------------------------------------------------------------------------------------- 3. values
@pytest.mark.parametrize("shape", SHAPES)
def test_sums_on_exact_data(ops, exact_sets, shape):
    n, m, d = shape
    x, y, d2 = exact_sets[shape]
    xt, yt = dev(x), dev(y)
    for kind, grid in EXACT_GRIDS:
        sums = ops.mmd_multi_sums(xt, yt, kind, grid, bw2=BW2)
        got = means_of(sums, n, m)
        swapped = ops.mmd_multi_sums(yt, xt, kind, grid, bw2=BW2)
        for j, c in enumerate(grid):
            want, scale = mr.parts_from_distances(d2, kind, BW2, c)
            err = np.abs(got[j] - want)
            print(f"{shape} {kind} c={c}: mean |K| {scale:.4f} |err| {err} limit {EXACT * scale:.3e}")
            assert n == 2 or (13.0 < scale < 20.0 if kind == "energy" else 0.04 < scale < 0.94), (shape, kind, c, scale)
            assert (err <= EXACT * scale).all(), (shape, kind, c, got[j], want, scale)
            # swapping the sets swaps Sxx / Syy exactly; Sxy is the same sum in another order
            a, b = sums[:, j].cpu().numpy(), swapped[:, j].cpu().numpy()
            assert a[0] == b[1] and a[1] == b[0], (shape, kind, c)
            assert abs(a[2] - b[2]) <= 1e-15 * abs(a[2]), (shape, kind, c, a[2], b[2])


@pytest.fixture(scope="module")
def real_sets():
    """(kind, d) -> (x, y, bw2 = the float32 median of the reference, f64 d2 matrices, emulated d2 matrices)."""
    out = {}
    for kind, seed, d in (("randn", 864, 64), ("unit", 1312, 512)):   # the sets of test_gpu_kad.py's test_sums_on_real_valued_rows
        y, x = gi.pair(kind, seed, 1000, 1000, d)
        pairs = ka.pair_values(y)
        bw2 = float(ka.as_key(pairs[ka.lower_median_rank(len(pairs))]))
        out[(kind, d)] = (x, y, bw2, mr.distances(x, y), mr.distances(x, y, dots=kr.emulated_dots("f32")))
    return out


@pytest.mark.parametrize("rows, d", [("randn", 64), ("unit", 512)])
def test_sums_on_real_valued_rows(ops, real_sets, rows, d):
    """Each normalised sum within MARGIN x the LARGEST of the three emulated errors of its kernel and scale (the f32 dot
    products rounded once per 32-element slab, kd_reference.emulated_dots; MARGIN covers the matrix cores' rounding after
    every product), mmd^2 = xx + yy - 2 xy within 4 x that.  The largest of the three, not each sum's own: a single sum's
    emulated error cancels by accident (unit, D = 512, Laplacian 0.5: 2.0e-14 for YY, where a rounding model that rounds
    after every 2 elements lands 370 times higher), and that says nothing about the device's; against the largest of the
    three the same finer model stays at or below 7.7 of the 16 allowed over all 18 cases.  Measured on the MI355X: the
    largest ratio is 13.2 of the 16 (randn, D = 64, Gaussian 0.25, XY), 11.2 for the Laplacian kernel and 9.6 for the energy
    kernel; unit, D = 512 stays below 6.8."""
    x, y, bw2, d2, d2_emulated = real_sets[(rows, d)]
    n, m = len(x), len(y)
    xt, yt = dev(x), dev(y)
    report = []
    for kind, grid in REAL_GRIDS:
        got = means_of(ops.mmd_multi_sums(xt, yt, kind, grid, bw2=bw2), n, m)
        for j, c in enumerate(grid):
            want, _ = mr.parts_from_distances(d2, kind, bw2, c)
            emulated, _ = mr.parts_from_distances(d2_emulated, kind, bw2, c)
            limit = kr.MARGIN * float(np.max(np.abs(emulated - want)))
            stats = [(name, g, w, limit) for name, g, w in zip(("xx", "yy", "xy"), got[j], want)]
            stats.append(("mmd2", ka.mmd2(got[j]), ka.mmd2(want), 4.0 * limit))
            for name, g, w, lim in stats:
                print(f"{rows} D={d} {kind} c={c} {name}: device {g!r} oracle {w!r} |err| {abs(g - w):.3e} limit {lim:.3e} "
                      f"= {kr.MARGIN * abs(g - w) / lim:.2f} of the {kr.MARGIN:.0f} allowed")
            report += [(kind, c, *s) for s in stats]
    for kind, c, name, g, w, lim in report:
        assert abs(g - w) <= lim, (rows, d, kind, c, name, g, w, lim)


# ---------------------------------------------------------------------------------------------------- 4. front ends
def data_of(am, rows, step=97):
    s = am.AudioMetricsData(True, device=DEV)
    for k in range(0, len(rows), step):
        s.add(dev(rows[k:k + step]))
    return s


@pytest.fixture(scope="module")
def front_sets():
    rng = np.random.default_rng(23)
    x, y = kr.rbf_rows(rng, 300, 100, SIGMA), kr.rbf_rows(rng, 513, 100, SIGMA)
    pairs = ka.pair_values(y)
    return x, y, float(ka.as_key(pairs[ka.lower_median_rank(len(pairs))])), mr.distances(x, y)


def test_scale_one_is_kernel_audio_distance(am, front_sets):
    x, y, bw2, _ = front_sets
    for kw in ({}, {"bandwidth": 3.0}, {"bandwidth": 7.3, "scale": 1000.0}):
        plain = am.kernel_audio_distance(data_of(am, x), data_of(am, y), **kw)
        multi = am.kernel_audio_distance_multiscale(data_of(am, x), data_of(am, y), scales=(1.0,), **kw)    # its own sets: nothing shared
        assert list(multi) == ["kad_multiscale", "kad_per_scale", "kad_mmd2_per_scale", "kad_scales", "kad_bandwidth", "kad_kernel"]
        assert multi["kad_per_scale"][0] == plain["kad"] and multi["kad_mmd2_per_scale"][0] == plain["kad_mmd2"], (kw, multi, plain)
        assert multi["kad_bandwidth"] == plain["kad_bandwidth"] and multi["kad_kernel"] == "gaussian"
        assert multi["kad_multiscale"] == plain["kad"]
        # the same scale inside a longer grid, against one reference that both functions use
        ref, cand = data_of(am, y), data_of(am, x)
        grid = am.kernel_audio_distance_multiscale(cand, ref, scales=(0.25, 0.5, 1.0, 2.0, 4.0), **kw)
        assert grid["kad_per_scale"][2] == plain["kad"] == am.kernel_audio_distance(cand, ref, **kw)["kad"]
    assert am.kernel_audio_distance_multiscale(data_of(am, x), data_of(am, y), scales=(1.0,))["kad_bandwidth"] == np.sqrt(bw2)


@pytest.mark.parametrize("kernel", ["gaussian", "laplacian"])
def test_multiscale_against_the_oracle(am, front_sets, kernel):
    x, y, bw2_median, d2 = front_sets
    scales = (0.25, 0.5, 1.0, 2.0, 4.0)
    for kw, bw2 in (({}, bw2_median), ({"bandwidth": 12.0, "scale": 7.0}, 144.0)):
        got = am.kernel_audio_distance_multiscale(data_of(am, x), data_of(am, y), scales=scales, kernel=kernel, **kw)
        assert got["kad_bandwidth"] == np.sqrt(bw2) and got["kad_kernel"] == kernel
        assert got["kad_scales"].dtype == np.float64 and got["kad_scales"].tolist() == list(scales)
        factor = kw.get("scale", 100.0)
        for j, c in enumerate(scales):
            want, unit = mr.parts_from_distances(d2, kernel, bw2, c)
            print(f"{kernel} c={c}: mmd2 {got['kad_mmd2_per_scale'][j]!r} oracle {ka.mmd2(want)!r} limit {3 * EXACT * unit:.3e}")
            assert abs(got["kad_mmd2_per_scale"][j] - ka.mmd2(want)) <= 3 * EXACT * unit        # three statistics, each within the bound of case 3
        assert got["kad_mmd2_per_scale"].dtype == np.float64 and got["kad_mmd2_per_scale"].shape == (5,)
        assert (got["kad_per_scale"] == factor * got["kad_mmd2_per_scale"]).all()
        assert got["kad_multiscale"] == factor * float(np.mean(got["kad_mmd2_per_scale"]))
    # a grid of 16 scales, the most the front end takes: four library calls
    wide = am.kernel_audio_distance_multiscale(data_of(am, x), data_of(am, y), scales=[2.0 ** (e / 2.0) for e in range(-8, 8)],
                                               kernel=kernel, bandwidth=10.0)
    assert wide["kad_mmd2_per_scale"].shape == (16,) and np.isfinite(wide["kad_mmd2_per_scale"]).all()
    assert wide["kad_mmd2_per_scale"][8] == am.kernel_audio_distance_multiscale(
        data_of(am, x), data_of(am, y), scales=(1.0,), kernel=kernel, bandwidth=10.0)["kad_mmd2_per_scale"][0]


def test_energy_distance_against_the_oracle(am, front_sets):
    x, y, _, d2 = front_sets
    want, unit = mr.parts_from_distances(d2, "energy")
    got = am.energy_distance(data_of(am, x), data_of(am, y))
    assert list(got) == ["energy_distance", "energy_mean_xy", "energy_mean_xx", "energy_mean_yy"]
    for key, w in (("energy_mean_xx", -want[0]), ("energy_mean_yy", -want[1]), ("energy_mean_xy", -want[2])):
        print(f"{key}: {got[key]!r} oracle {w!r} limit {EXACT * unit:.3e}")
        assert abs(got[key] - w) <= EXACT * unit
    assert got["energy_distance"] == 2.0 * got["energy_mean_xy"] - got["energy_mean_xx"] - got["energy_mean_yy"]
    assert abs(got["energy_distance"] - mr.energy_from_means(want)) <= 4 * EXACT * unit
    # a shifted copy is far from its original: the distance is positive there (between two draws of one distribution the
    # unbiased estimate may fall on either side of 0)
    shifted = am.energy_distance(data_of(am, x + np.float32(2.0)), data_of(am, x))
    assert shifted["energy_distance"] > 0.0
    # identical sets: the unbiased estimate of 0 drops the diagonals only
    same = am.energy_distance(data_of(am, x), data_of(am, x))
    assert same["energy_distance"] < 0.0 and same["energy_mean_xx"] == same["energy_mean_yy"]


def test_reference_side_is_cached_and_recomputed_after_an_append(am, monkeypatch):
    rng = np.random.default_rng(31)
    x, y, more = (kr.rbf_rows(rng, n, 64, SIGMA) for n in (150, 400, 130))
    calls = {"select": 0, "blocks": [], "rbf": 0}
    real_select, real_multi, real_rbf = am.hip_ops.pairwise_select_sq, am.hip_ops.mmd_multi_sums, am.hip_ops.mmd_rbf_sums

    def counting_select(*a, **k):
        calls["select"] += 1
        return real_select(*a, **k)

    def counting_multi(*a, **k):
        calls["blocks"].append(k.get("blocks", 7))
        return real_multi(*a, **k)

    def counting_rbf(*a, **k):
        calls["rbf"] += 1 if k.get("blocks", 7) & 2 else 0
        return real_rbf(*a, **k)
    monkeypatch.setattr(am.hip_ops, "pairwise_select_sq", counting_select)
    monkeypatch.setattr(am.hip_ops, "mmd_multi_sums", counting_multi)
    monkeypatch.setattr(am.hip_ops, "mmd_rbf_sums", counting_rbf)
    multi, grid = am.kernel_audio_distance_multiscale, (0.5, 1.0, 2.0)
    cand, ref = data_of(am, x), data_of(am, y)
    first = multi(cand, ref, scales=grid)
    assert calls["select"] == 1 and calls["blocks"] == [7]
    second = multi(cand, ref, scales=grid)
    assert calls["select"] == 1 and calls["blocks"] == [7, 5]                  # neither the median nor YY again
    assert all(np.array_equal(first[k], second[k]) for k in first)
    other = multi(data_of(am, more), ref, scales=grid)                        # another candidate set, the same reference
    assert calls["select"] == 1 and calls["blocks"] == [7, 5, 5]
    fresh = multi(data_of(am, more), data_of(am, y), scales=grid)
    assert all(np.array_equal(other[k], fresh[k]) for k in other)
    # another kernel, or a scale the cache has not seen: YY again, the median not
    multi(cand, ref, scales=grid, kernel="laplacian")
    multi(cand, ref, scales=grid, kernel="laplacian")
    multi(cand, ref, scales=(1.0, 3.0))
    assert calls["select"] == 2 and calls["blocks"] == [7, 5, 5, 7, 7, 5, 7]   # (select == 2: the fresh reference above)
    # kernel_audio_distance on the same reference: the median is there, and so is Syy at scale 1 - the same bits
    plain = am.kernel_audio_distance(cand, ref)
    assert calls["select"] == 2 and calls["rbf"] == 0
    assert plain["kad"] == first["kad_per_scale"][1] == am.kernel_audio_distance(data_of(am, x), data_of(am, y))["kad"]
    assert calls["select"] == 3 and calls["rbf"] == 1
    # the energy distance keeps its own entry
    calls["blocks"].clear()
    e1, e2 = am.energy_distance(cand, ref), am.energy_distance(cand, ref)
    assert calls["blocks"] == [7, 5] and e1 == e2 and calls["select"] == 3
    assert "_kad_cache" not in ref.serialize()
    # an append: the median and YY are recomputed for the grown set
    calls["blocks"].clear()
    ref.add(dev(more))
    grown = multi(cand, ref, scales=grid)
    assert calls["select"] == 4 and calls["blocks"] == [7]
    whole = multi(data_of(am, x), data_of(am, np.concatenate([y, more])), scales=grid)
    assert all(np.array_equal(grown[k], whole[k]) for k in grown)
    assert am.energy_distance(cand, ref) == am.energy_distance(data_of(am, x), data_of(am, np.concatenate([y, more])))
    assert calls["blocks"] == [7, 7, 7, 7]


def test_errors_that_need_the_device(am):
    rng = np.random.default_rng(37)
    x = kr.rbf_rows(rng, 40, 32, SIGMA)
    dup = np.repeat(kr.rbf_rows(rng, 2, 32, SIGMA), [35, 5], axis=0)
    multi = am.kernel_audio_distance_multiscale
    with pytest.raises(ValueError, match="coincide"):
        multi(data_of(am, x), data_of(am, dup))
    half = x.copy()
    half[::2, 0] = np.nan                                            # half of the rows: more than half of the pairs
    with pytest.raises(ValueError, match="non-finite"):
        multi(data_of(am, x), data_of(am, half))
    one = x.copy()
    one[7, 3] = np.inf                                               # one row: the median stays finite, the sums do not
    for bad_x, bad_y in ((one, x), (x, one)):
        with pytest.raises(ValueError, match="non-finite rows"):
            multi(data_of(am, bad_x), data_of(am, bad_y))
        with pytest.raises(ValueError, match="non-finite rows"):
            multi(data_of(am, bad_x), data_of(am, bad_y), kernel="laplacian", bandwidth=5.0)
        with pytest.raises(ValueError, match="non-finite rows"):
            am.energy_distance(data_of(am, bad_x), data_of(am, bad_y))
    with pytest.raises(NotImplementedError, match="float64"):
        multi(data_of(am, x.astype(np.float64)), data_of(am, x))
    with pytest.raises(NotImplementedError, match="float64"):
        am.energy_distance(data_of(am, x), data_of(am, x.astype(np.float64)))
