"""Parity of the HIP path (through the Python mirror -> ctypes -> C ABI) against
the oracle, the reference's golden vectors and the plain-C model of the device
arithmetic.  Tolerances (BASELINE.json north_star): 1e-4 relative on f32 inputs
for FAD / KD / PRDC / APA; PRDC radii, thresholds and membership counts are
additionally BIT-EXACT against oracle/exact_c."""
import numpy as np
import pytest
import torch

import inputs as gi

pytestmark = pytest.mark.gpu

REL = 1e-4
KD_ABS_FLOOR = 5e-7        # f32 noise floor of the reference's own KD
EPS32 = 2.0 ** -24


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    audio_metrics_amd._lib.load()          # fail loudly if the HIP library is missing
    return audio_metrics_amd


def dev(x):
    return torch.as_tensor(x).to("cuda:0")


def knob_env(base, knobs):
    """Environment of an A/B subprocess: development knobs exist only in the -DAM_DEV_KNOBS build of the library
    (libaudio_metrics_hip_dev.so, selected with AM_HIP_LIBRARY=dev); a run WITHOUT knobs exercises the shipped library."""
    env = dict(base, **knobs)
    if any(key.startswith("AM_") for key in knobs):
        env["AM_HIP_LIBRARY"] = "dev"
    return env


def amd_of(am, x, store=True, splits=None):
    d = am.AudioMetricsData(store)
    t = dev(x)
    if splits is None:
        d.add(t)
    else:
        s = 0
        for b in splits:
            d.add(t[s:s + b])
            s += b
    return d


# ----------------------------------------------------------------- PRDC
@pytest.mark.parametrize("name", list(gi.PRDC_CASES))
def test_prdc_bit_exact_and_golden(am, golden, name):
    from oracle import exact
    g = golden("prdc")
    kind, seed, nr, nc, d, k = gi.PRDC_CASES[name]
    ref, cand = gi.pair(kind, seed, nr, nc, d)
    a, b = amd_of(am, ref), amd_of(am, cand)
    res = am.prdc(a, b, k)
    _, aux = exact.prdc(ref, cand, k)
    ops = am.hip_ops
    col, rany, rcov, rmin = ops.prdc_counts(a.embeddings, b.embeddings, a.get_radii(k), b.get_radii(k), want_min=True)
    col3, rany3, rcov3 = ops.prdc_counts(a.embeddings, b.embeddings, a.get_radii(k), b.get_radii(k))
    assert torch.equal(col, col3) and torch.equal(rany, rany3) and torch.equal(rcov, rcov3)   # with / without the optional minimum
    # bit-exact against the C model of the device arithmetic
    assert np.array_equal(a.get_radii(k).cpu().numpy().view(np.uint32), aux["r_ref"].view(np.uint32))
    assert np.array_equal(b.get_radii(k).cpu().numpy().view(np.uint32), aux["r_cand"].view(np.uint32))
    assert np.array_equal(col.cpu().numpy(), aux["col_count"])
    assert np.array_equal(rany.cpu().numpy(), aux["row_any"])
    assert np.array_equal(rmin.cpu().numpy().view(np.uint32), aux["row_min"].view(np.uint32))
    assert np.array_equal(rcov.cpu().numpy().astype(bool), aux["row_min"] < aux["r_ref"])
    # against the reference's own outputs
    np.testing.assert_allclose(a.get_radii(k).cpu().numpy(), g[f"{name}/r_ref"], rtol=3e-5, atol=1e-6)
    flips = int(np.abs(col.cpu().numpy().astype(np.int64) - g[f"{name}/col_count"]).sum())
    assert flips <= max(1, 1e-4 * int(g[f"{name}/col_count"].sum()))
    for key in ("precision", "recall", "density", "coverage"):
        want = float(g[f"{name}/{key}"])
        assert abs(res[key] - want) <= max(REL * abs(want), 1.0 / min(nr, nc)), (key, res[key], want)
    assert list(res) == ["precision", "recall", "density", "coverage"]


@pytest.mark.parametrize("k", [1, 7, 16, 31])
def test_knn_other_k_bit_exact(am, k):
    from oracle import exact
    x = gi.randn(61, 700, 40)
    r = am.nearest_neighbour_distances(dev(x), k).cpu().numpy()
    assert np.array_equal(r.view(np.uint32), exact.knn_radii(x, k).view(np.uint32))


@pytest.mark.parametrize("k", [32, 40, 100, 699])
def test_knn_beyond_the_list_kernels_bit_exact(am, k):
    """nearest_k > AM_MAX_K (31): the reference takes any k (prdc.py:18), the tile kernels hold k + 1 <= 32 values per
    lane - larger k run row by row (am_knn_path == 4) and must give the C model's bits too, for the set against itself and
    against other columns; prdc() with such a k against the oracle."""
    from oracle import exact
    import oracle
    x, y = gi.randn(61, 700, 40), gi.randn(64, 901, 40)
    ops = am.hip_ops
    assert ops.knn_path(700, 700, 40, k) == 4
    r = am.nearest_neighbour_distances(dev(x), k).cpu().numpy()
    assert np.array_equal(r.view(np.uint32), exact.knn_radii(x, k).view(np.uint32))
    r2 = ops.knn_radii(dev(x), k, columns=dev(y)).cpu().numpy()
    assert np.array_equal(r2.view(np.uint32), exact.knn_radii(x, k, columns=y).view(np.uint32))
    if k <= 100:
        a, b = amd_of(am, x), amd_of(am, y[:650])
        got = am.prdc(a, b, k)
        want = oracle.prdc_from_features(torch.as_tensor(x), torch.as_tensor(y[:650]), oracle.knn_radii(x, k), oracle.knn_radii(y[:650], k), k)
        for key in want:
            assert abs(got[key] - want[key]) <= max(REL * abs(want[key]), 2.0 / 650), (key, got[key], want[key])


@pytest.mark.parametrize("k", [16, 20, 31])
def test_knn_long_lists_on_mid_sized_sets_bit_exact(am, k):
    """k + 1 > 16 below the f16 filter sweep's threshold: the exact symmetric kernel would need 32 list registers per row
    and lane and spills - such shapes take the general kernel (am_knn_path == 0); same bits as the C model."""
    from oracle import exact
    x = gi.randn(65, 7000, 128)
    assert am.hip_ops.knn_path(7000, 7000, 128, k) == 0
    assert am.hip_ops.knn_path(9000, 9000, 128, k) == 2             # with the f16 filter sweep the lists only steer: 128-row engine
    assert am.hip_ops.knn_path(9000, 9000, 128, 10) == 3
    r = am.nearest_neighbour_distances(dev(x), k).cpu().numpy()
    assert np.array_equal(r.view(np.uint32), exact.knn_radii(x, k).view(np.uint32))


@pytest.mark.parametrize("n,d,k,kind", [(17000, 64, 5, "randn"), (12100, 40, 10, "randn"), (6200, 256, 5, "randn"),
                                        (8300, 130, 3, "randn"), (12100, 64, 5, "unit"), (6200, 512, 10, "unit"),
                                        (8300, 128, 5, "unit"), (17000, 8, 5, "randn"), (16500, 24, 10, "unit"),
                                        (16400, 12, 2, "randn")])
def test_knn_filter_sweep_at_its_lower_thresholds_bit_exact(am, n, d, k, kind):
    """The f16 filter sweep + exact verification just above the row counts where it takes over (6144 rows for D >= 256,
    8192 for 128 <= D < 256, 12 000 for 32 <= D < 128 and 16 384 below - the narrow rows n_pca leaves: round 4,
    tools/threshold_sweep.py on randn AND unit-norm (CLAP-shaped) sets) - radii bit-identical to the C model of the exact arithmetic, no row falls back."""
    from oracle import exact
    ops = am.hip_ops
    x = gi.randn(66, n, d) if kind == "randn" else gi.unit_norm(66, n, d)
    assert ops.knn_path(n, n, d, k) == 3
    ops.filter_stats_enable("cuda:0", True)
    r = am.nearest_neighbour_distances(dev(x), k).cpu().numpy()
    stats = ops.filter_stats_read("cuda:0")
    ops.filter_stats_enable("cuda:0", False)
    assert stats["knn_calls"] == 1 and stats["knn_fallback_rows"] == 0, stats
    assert np.array_equal(r.view(np.uint32), exact.knn_radii(x, k).view(np.uint32))


@pytest.mark.parametrize("n,d,k", [(20000, 128, 5), (9000, 512, 5), (16500, 64, 10)])
def test_knn_filter_gives_way_on_data_it_cannot_separate(am, n, d, k):
    """Tightly clustered rows (50 centres, spread 1e-3): every member of a row's cluster lies inside the f16 error band of its
    (k+1)-th neighbour - hundreds of undecidable pairs per row (measured before the guard: 283 ms against 7.5 ms for the exact
    kernels at 20 000 x 512, k = 5).  The device-side checks of the filter path (knn_fast_predict_kernel) must hand the whole
    set to the exact general kernel: every row is reported as a fallback row, and the radii are the C model's bits."""
    from oracle import exact
    ops = am.hip_ops
    rng = np.random.default_rng(5)
    centres = rng.standard_normal((50, d)).astype(np.float32)
    x = (centres[rng.integers(0, 50, n)] + 1e-3 * rng.standard_normal((n, d)).astype(np.float32)).astype(np.float32)
    assert ops.knn_path(n, n, d, k) == 3                     # the shapes alone still choose the filter path
    ops.filter_stats_enable("cuda:0", True)
    r = am.nearest_neighbour_distances(dev(x), k).cpu().numpy()
    stats = ops.filter_stats_read("cuda:0")
    ops.filter_stats_enable("cuda:0", False)
    assert stats["knn_calls"] == 1 and stats["knn_fallback_rows"] == n, stats
    assert np.array_equal(r.view(np.uint32), exact.knn_radii(x, k).view(np.uint32))
    # well-separated data of the same shape keeps the filter path (no fallback row)
    y = gi.randn(67, n, d)
    ops.filter_stats_enable("cuda:0", True)
    am.nearest_neighbour_distances(dev(y), k)
    stats = ops.filter_stats_read("cuda:0")
    ops.filter_stats_enable("cuda:0", False)
    assert stats["knn_fallback_rows"] == 0, stats


@pytest.mark.parametrize("n,d,k,block", [(20000, 128, 5, 700), (20000, 128, 10, 1500), (12000, 512, 5, 40), (33000, 64, 3, 3000)])
def test_a_block_of_identical_rows_goes_through_the_batched_fix_up(am, n, d, k, block):
    """Silent windows of a stem dataset embed to one and the same vector: a block of identical rows.  Each of them has all the
    others at distance zero - more than a row's candidate buffer holds once the block is larger than it (384 / 704 entries) -
    and was recomputed one row at a time (42 us per row at 100 000 x 512).  Now the sample pass recognises such rows (identical
    rows give identical approximate values), takes them out of the sweep and hands them to the batched fix-up: the exact
    GENERAL kernel on a gathered copy.  Exactly the block's rows fall back (a block that fits the buffers: none), everybody
    else stays on the filter path, and every radius is the C model's bits."""
    from oracle import exact
    ops = am.hip_ops
    x = gi.unit_norm(81, n, d)
    rng = np.random.default_rng(block)
    rows = rng.choice(n, block, replace=False)
    x[rows] = x[rows[0]]
    assert ops.knn_path(n, n, d, k) == 3
    ops.filter_stats_enable("cuda:0", True)
    r = am.nearest_neighbour_distances(dev(x), k).cpu().numpy()
    stats = ops.filter_stats_read("cuda:0")
    ops.filter_stats_enable("cuda:0", False)
    cap = max(256, 64 * (k + 1))
    if block > cap:
        assert block <= stats["knn_fallback_rows"] <= block + n // 200, stats           # the block, and hardly anybody else
    else:
        assert stats["knn_fallback_rows"] <= n // 200, stats
    assert np.array_equal(r.view(np.uint32), exact.knn_radii(x, k).view(np.uint32))


def test_membership_filter_gives_way_when_both_sets_share_tight_clusters(am):
    """Reference and candidate rows drawn around the SAME 50 tight clusters: every candidate of a reference row's cluster lies
    inside the f16 error band of that row's radius - hundreds of undecidable pairs per row (before the guard: 96 ms against
    7.6 ms for the exact kernel at 20 000 x 512).  The filter must raise its fail flag and leave the call to the exact kernel:
    one fallback call in the statistics, counts and flags equal to the C model's bit for bit."""
    from oracle import exact
    ops = am.hip_ops
    n, d, k = 12000, 128, 5
    rng = np.random.default_rng(6)
    centres = rng.standard_normal((50, d)).astype(np.float32)
    ref = (centres[rng.integers(0, 50, n)] + 1e-3 * rng.standard_normal((n, d))).astype(np.float32)
    cand = (centres[rng.integers(0, 50, n)] + 1e-3 * rng.standard_normal((n, d))).astype(np.float32)
    assert ops.prdc_path(n, n, d) == 3
    r_ref, r_cand = exact.knn_radii(ref, k), exact.knn_radii(cand, k)
    ops.filter_stats_enable("cuda:0", True)
    col, rany, rcov = ops.prdc_counts(dev(ref), dev(cand), dev(r_ref), dev(r_cand))
    stats = ops.filter_stats_read("cuda:0")
    ops.filter_stats_enable("cuda:0", False)
    assert stats["prdc_calls"] == 1 and stats["prdc_fallback_calls"] == 1, stats
    ecol, eany, emin = exact.prdc_counts(ref, cand, r_ref, r_cand)
    assert np.array_equal(col.cpu().numpy(), ecol) and np.array_equal(rany.cpu().numpy(), eany)
    assert int(col.sum()) > n                                # (the clusters really are shared: every ball holds candidates)
    # well-separated sets of the same shape stay on the filter path
    a, b = gi.pair("shifted", 77, n, n, d)
    ra, rb = (am.hip_ops.knn_radii(dev(x), k) for x in (a, b))
    ops.filter_stats_enable("cuda:0", True)
    ops.prdc_counts(dev(a), dev(b), ra, rb)
    stats = ops.filter_stats_read("cuda:0")
    ops.filter_stats_enable("cuda:0", False)
    assert stats["prdc_fallback_calls"] == 0, stats


def test_dense_low_dimensional_sets_take_the_exact_kernel_on_their_own(am):
    """16 400 random points in THREE dimensions: neighbours are closer than the f16 error band (which scales with the squared
    norms, not with the neighbour distances), so the filter cannot separate them - the shapes choose the filter path, the
    device-side check hands the call to the exact kernel, the radii are the C model's bits."""
    from oracle import exact
    ops = am.hip_ops
    n, d, k = 16400, 3, 2
    x = gi.randn(66, n, d)
    assert ops.knn_path(n, n, d, k) == 3
    ops.filter_stats_enable("cuda:0", True)
    r = am.nearest_neighbour_distances(dev(x), k).cpu().numpy()
    stats = ops.filter_stats_read("cuda:0")
    ops.filter_stats_enable("cuda:0", False)
    assert stats["knn_fallback_rows"] == n, stats
    assert np.array_equal(r.view(np.uint32), exact.knn_radii(x, k).view(np.uint32))


def test_non_finite_rows_do_not_poison_the_finite_ones(am):
    """One NaN row and one row with an infinite element in a set large enough for the f16 filter path (the scale of the f16 copy
    cannot be derived from a non-finite maximum: the device-side checks must route the call to the exact kernel).  Like
    torch.kthvalue in the reference (prdc.py:13), a NaN distance never counts among a row's k + 1 smallest: every finite row
    keeps the radius it has in torch's own computation; nothing hangs, nothing is NaN that should not be."""
    n, d, k = 9000, 128, 5
    x = gi.randn(71, n, d)
    x[123] = np.nan
    x[4567, 7] = np.inf
    assert am.hip_ops.knn_path(n, n, d, k) == 3
    r = am.nearest_neighbour_distances(dev(x), k).cpu()
    xt = torch.as_tensor(x)
    want = torch.kthvalue(torch.cdist(xt, xt), k + 1, dim=-1)[0]
    finite = torch.ones(n, dtype=torch.bool)
    finite[123] = finite[4567] = False
    assert torch.isfinite(r[finite]).all()
    assert float((r[finite] - want[finite]).abs().max()) <= 3e-5 * float(want[finite].max())
    # ... and the four PRDC values of (this set, a clean candidate set) equal the reference formulation's on the same rows
    import oracle
    y = gi.randn(72, n, d) * 1.05 + 0.05
    a, b = am.AudioMetricsData(True), am.AudioMetricsData(True)
    a.add(dev(x))
    b.add(dev(y))
    assert am.hip_ops.prdc_path(n, n, d) == 3
    got = am.prdc(a, b, k)
    oa, ob = oracle.OracleData(True).add(torch.as_tensor(x)), oracle.OracleData(True).add(torch.as_tensor(y))
    want_prdc = oracle.prdc(oa, ob, k)
    for key, w in want_prdc.items():
        assert abs(got[key] - w) <= max(1e-4 * abs(w), 2.0 / n), (key, got[key], w)


def test_knn_rows_vs_other_columns(am):
    """row shard against a larger column set (the multi-GPU calling pattern)."""
    from oracle import exact
    x, y = gi.randn(62, 333, 72), gi.randn(63, 901, 72)
    r = am.hip_ops.knn_radii(dev(x), 4, columns=dev(y)).cpu().numpy()
    assert np.array_equal(r.view(np.uint32), exact.knn_radii(x, 4, columns=y).view(np.uint32))


def test_knn_k_out_of_range(am):
    x = dev(gi.randn(1, 5, 8))
    with pytest.raises(am._lib.HipLibraryError):
        am.nearest_neighbour_distances(x, 5)          # k + 1 > N: torch.kthvalue raises in the reference
    with pytest.raises(am._lib.HipLibraryError):
        am.nearest_neighbour_distances(dev(gi.randn(1, 64, 8)), 64)   # k + 1 > N
    with pytest.raises(am._lib.HipLibraryError):
        am.hip_ops.stats(torch.zeros(4, 4))            # host tensor: no CPU fallback


def test_prdc_self_consistency_full_size(am):
    """2 x 100k x 512 (BASELINE config 3 shape), size-independent property: for
    identical sets every row has exactly k columns strictly inside its radius
    (itself + k-1 neighbours) unless its k-th and (k-1)-th neighbours tie in f32, so
    precision = recall = coverage = 1 and the count total is N*k minus a few ties."""
    torch.manual_seed(0)
    x = torch.randn(100000, 512, device="cuda:0")
    a = am.AudioMetricsData(True)
    a.add(x)
    res = am.prdc(a, a, 5)
    assert (res["precision"], res["recall"], res["coverage"]) == (1.0, 1.0, 1.0)
    total = round(res["density"] * 5 * 100000)
    assert 500000 - 50 <= total <= 500000, total


# ----------------------------------------------------------------- stats
@pytest.mark.parametrize("name", list(gi.STATS_CASES))
def test_stats_vs_golden(am, golden, name):
    g = golden("stats")
    seed, d, splits = gi.STATS_CASES[name]
    x = gi.randn(seed, sum(splits), d, 1.3, 0.2)
    a = amd_of(am, x, True, splits)
    assert a.n == int(g[f"{name}/n"]) and len(a) == a.n
    np.testing.assert_allclose(a.mean.cpu().numpy(), g[f"{name}/mean"], rtol=1e-6, atol=1e-6)
    c = a.cov.cpu().numpy()
    if d <= 128:
        np.testing.assert_allclose(c, g[f"{name}/cov"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(np.trace(c), float(g[f"{name}/cov_trace"]), rtol=1e-6)
    np.testing.assert_allclose(c[::37, ::41], g[f"{name}/cov_sample"], rtol=1e-5, atol=2e-6)
    assert np.array_equal(c, c.T)
    a.recompute_stats()
    np.testing.assert_allclose(a.mean.cpu().numpy(), g[f"{name}/re_mean"], rtol=1e-6, atol=1e-6)
    assert tuple(a.cov.shape) == tuple(g[f"{name}/re_cov_shape"])       # incl. the (1, 1) quirk for n == 1
    assert a.embeddings.shape == (sum(splits), d)
    np.testing.assert_array_equal(a.embeddings.cpu().numpy(), x)


def test_incremental_equals_oneshot(am):
    """Device analogue of the reference's tests/test_data.py:6-31 (1e-6)."""
    x = gi.randn(7, 1101, 8)
    a = amd_of(am, x, True, [1, 100, 1000])
    b = amd_of(am, x, True, [1101])
    np.testing.assert_allclose(a.mean.cpu().numpy(), b.mean.cpu().numpy(), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(a.cov.cpu().numpy(), b.cov.cpu().numpy(), rtol=1e-6, atol=1e-6)
    c = amd_of(am, x[:500], True) + amd_of(am, x[500:], True)
    np.testing.assert_allclose(c.cov.cpu().numpy(), b.cov.cpu().numpy(), rtol=1e-6, atol=1e-6)
    assert c.embeddings.shape == (1101, 8)


@pytest.mark.parametrize("n,d", [(1, 8), (2, 5), (33, 8), (1000, 24), (5000, 130), (20000, 512), (777, 33)])
def test_float64_rows_keep_float64_statistics(am, n, d):
    """The reference computes an add()'s statistics in the dtype of the embeddings it is given (data.py:39-44): float64 rows
    (its own test embedder, the output of its PCA projection) must not pass through float32 on the way to mean / covariance.
    am_stats_f64 against torch's f64 mean / cov on the device and against the CPU oracle fed the same f64 rows."""
    import oracle
    rng = np.random.default_rng(40 + n)
    x = rng.standard_normal((n, d)) * 1.3 + 0.2 + 1e-9 * rng.standard_normal((n, d))      # (not representable in f32)
    xd = torch.as_tensor(x).to("cuda:0")
    mean, cov = am.hip_ops.stats_f64(xd)
    want_mean = xd.mean(0)
    want_cov = torch.cov(xd.T) if n > 1 else torch.zeros((d, d), dtype=torch.float64, device=xd.device)
    scale = float(want_cov.abs().max()) if n > 1 else 1.0
    assert float((mean - want_mean).abs().max()) <= 1e-13 * max(1.0, float(want_mean.abs().max()))
    assert float((cov - want_cov.reshape(d, d)).abs().max()) <= 1e-12 * max(scale, 1e-30)
    assert torch.equal(cov, cov.T)                                                      # exactly symmetric
    # through the container, in 32-row adds like the pipeline's, against the oracle's dtype ladder on the same rows
    a, o = am.AudioMetricsData(store_embeddings=False), oracle.OracleData(False)
    for lo in range(0, n, 32):
        a.add(xd[lo:lo + 32])
        o.add(torch.as_tensor(x[lo:lo + 32]))
    np.testing.assert_allclose(a.mean.cpu().numpy(), o.mean.numpy(), rtol=1e-12, atol=1e-13)
    if n > 1:
        np.testing.assert_allclose(a.cov.cpu().numpy(), o.cov.numpy(), rtol=1e-10, atol=1e-12 * scale)
    # the f32 route on the same values is visibly coarser: the f64 route is not a relabelled narrowing
    if n >= 1000:
        m32, _ = am.hip_ops.stats(xd.to(torch.float32))
        assert float((m32 - want_mean).abs().max()) > 50 * float((mean - want_mean).abs().max())


@pytest.mark.parametrize("d,splits", [(512, [32] * 40), (21, [1, 7, 1, 32, 128, 3]), (128, [128, 5, 64]), (40, [1, 1, 1, 16])])
def test_one_launch_add_matches_the_chain(am, d, splits):
    """am_stats_push_f32 (one launch per small add: batch statistics + Chan merge + row append, data.py:37-47, 68-94)
    against the separate entry points (am_stats_f32 -> am_stats_merge_f64 -> copy) on the same batches, and both against an
    f64 one-shot evaluation; odd widths, single-row batches, a first batch of one row, unaligned row views."""
    ops = am.hip_ops
    x = gi.randn(17, sum(splits), d, 1.3, 0.2)
    t = dev(x)
    pushed, chained = am.AudioMetricsData(True), am.AudioMetricsData(True)
    s = 0
    for b in splits:
        e = t[s:s + b]
        assert b <= ops.stats_push_max_rows()
        pushed.add(e)                                             # one launch
        mean, cov = ops.stats(ops.as_matrix(e))                   # the chain, spelled out
        chained._update_stats(mean, cov, b)
        chained._update_embeddings(e)
        s += b
    assert pushed.n == chained.n == sum(splits)
    assert torch.equal(pushed.embeddings, t) and torch.equal(chained.embeddings, t)
    x64 = x.astype(np.float64)
    want_mean, want_cov = x64.mean(0), np.cov(x64.T)
    for got in (pushed, chained):
        np.testing.assert_allclose(got.mean.cpu().numpy(), want_mean, rtol=0, atol=1e-12)
        assert np.linalg.norm(got.cov.cpu().numpy() - want_cov) <= 3e-7 * np.linalg.norm(want_cov)
    # the two paths differ only in how the <= 128 products of a batch entry are summed (fma in row order here, the
    # order of am_stats_f32 there: f64 as well below 128 columns, an f32 MFMA chain from 128 up)
    assert float((pushed.cov - chained.cov).norm() / chained.cov.norm()) <= 2e-7
    # stats-only sets take the same path without touching a store
    lean = am.AudioMetricsData(False)
    s = 0
    for b in splits:
        lean.add(t[s:s + b])
        s += b
    assert lean.embeddings is None and torch.equal(lean.cov, pushed.cov) and torch.equal(lean.mean, pushed.mean)


def test_prepared_set_follows_the_stored_rows(am):
    """The cached PreparedSet (norms, f16 copy) is tied to a content version, not to a pointer: appends, assignments to
    .embeddings and invalidate_prepared() all force a fresh one."""
    a = am.AudioMetricsData(True)
    a.add(dev(gi.randn(3, 300, 24)))
    p0 = a.prepared()
    assert a.prepared() is p0
    a.add(dev(gi.randn(4, 20, 24)))
    p1 = a.prepared()
    assert p1 is not p0 and p1.norms.numel() == 320
    a.embeddings = a.embeddings.clone()
    assert a.prepared() is not p1
    p2 = a.prepared()
    a.embeddings.mul_(2.0)
    a.invalidate_prepared()
    p3 = a.prepared()
    assert p3 is not p2 and torch.allclose(p3.norms, 4.0 * p2.norms, rtol=1e-6)


def test_stats_full_size_vs_f64(am):
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((100000, 512)) * 1.05 + 0.05).astype(np.float32)
    mean, cov = am.hip_ops.stats(dev(x))
    x64 = x.astype(np.float64)
    np.testing.assert_allclose(mean.cpu().numpy(), x64.mean(0), rtol=0, atol=1e-12)
    xc = x64 - x64.mean(0)
    want = xc.T @ xc / (len(x) - 1)
    got = cov.cpu().numpy()
    assert np.linalg.norm(got - want) / np.linalg.norm(want) < 2e-7
    assert abs(np.trace(got) - np.trace(want)) / np.trace(want) < 1e-7


def test_strided_and_odd_width_inputs(am):
    x = gi.randn(8, 300, 21)                                        # D % 4 != 0
    big = dev(np.concatenate([x, x], axis=1))[:, :21]               # non-contiguous view, odd row stride
    m1, c1 = am.hip_ops.stats(big)
    x64 = x.astype(np.float64)
    np.testing.assert_allclose(m1.cpu().numpy(), x64.mean(0), atol=1e-12)
    np.testing.assert_allclose(c1.cpu().numpy(), np.cov(x64.T), rtol=1e-5, atol=1e-6)


# ----------------------------------------------------------------- FAD / APA
def fad_exact_f64(ref, cand):
    """The quantity fad.py:28-31 defines, evaluated in f64 end to end with torch on the host: mean / covariance of the f32
    inputs in f64, tr sqrt(Sx Sy) through the symmetric PSD form sqrt(Sx) Sy sqrt(Sx) (eigvalsh; negative rounding
    noise clamped).  No f32 statistics, no general eigensolver: this is what the reference would return without its own
    rounding noise."""
    def stats(x):
        x = torch.as_tensor(x, dtype=torch.float64)
        mu = x.mean(0)
        xc = x - mu
        return mu, xc.T @ xc / max(len(x) - 1, 1)
    (mx, sx), (my, sy) = stats(cand), stats(ref)
    w, v = torch.linalg.eigh(sx)
    root = (v * w.clamp_min(0).sqrt()) @ v.T
    lam = torch.linalg.eigvalsh(root @ sy @ root)
    tr_sqrt = lam.clamp_min(0).sqrt().sum()
    return float(((mx - my) ** 2).sum() + sx.trace() + sy.trace() - 2.0 * tr_sqrt)


FAD_EXACT_REL = 1e-6      # device value against the f64 evaluation of the definition ...
FAD_TERMS_REL = 1e-7      # ... plus the f32 rounding of the centred inputs in the device covariance (DESIGN "Stats numerics":
                          # 1e-7 relative Frobenius), relative to tr Sx + tr Sy - the terms the distance is a difference of


def fad_exact_tol(exact, scale):
    return FAD_EXACT_REL * abs(exact) + FAD_TERMS_REL * scale


@pytest.mark.parametrize("name", list(gi.FAD_CASES))
def test_fad_vs_golden(am, golden, name):
    """Two separate statements (N < D included, no widened formula):
    (1) the device value equals the f64 PSD evaluation of the definition - recomputed here with torch on the same
        inputs, and the copy make_goldens.py stored - to 1e-6 relative (+ 1e-7 of tr Sx + tr Sy);
    (2) it agrees with the reference's own output to 1e-4 relative or the reference's MEASURED noise on that case
        (|reference - f64 evaluation|, stored by make_goldens.py as `ref_noise`: 2.6e-4 relative for the 40-row set,
        3.6e-4 for 100 CLAP-shaped rows against 4096 - spurious eigenvalues of its f32 torch.cov in the null directions,
        fad.py:30) plus (1)'s 1e-6, whichever is larger."""
    g = golden("fad")
    kind, seed, nr, nc, d = gi.FAD_CASES[name]
    ref, cand = gi.pair(kind, seed, nr, nc, d)
    a, b = amd_of(am, cand, False), amd_of(am, ref, False)
    fad, swapped = am.frechet_distance(a, b), am.frechet_distance(b, a)
    assert isinstance(fad, float)
    exact = fad_exact_f64(ref, cand)
    scale = float(a.cov.trace() + b.cov.trace())                       # the terms the distance is a difference of
    # (the stored copy came from numpy's eigh, this one from torch's: on rank-deficient inputs the square roots of their
    # rounding-noise eigenvalues differ by a few 1e-9 of the terms)
    assert abs(exact - float(g[f"{name}/fad_exact_f64"])) <= 2e-8 * scale
    for got in (fad, swapped):
        assert abs(got - exact) <= fad_exact_tol(exact, scale), (got, exact, scale)
    noise = float(g[f"{name}/ref_noise"])
    for got, key in ((fad, "fad"), (swapped, "fad_swapped")):
        want = float(g[f"{name}/{key}"])
        tol = max(REL * abs(want), noise + fad_exact_tol(exact, scale))
        assert abs(got - want) <= tol, (key, got, want, noise)
    if min(nr, nc) > d:                                                # full rank: the reference itself is exact to ~1e-7
        assert noise <= 1e-6 * abs(exact), noise
    else:
        # Fewer rows than dimensions: the widened tolerance above is justified by DATA, not asserted - make_goldens.py
        # gen_fad_spread() ran the reference's own code on these inputs under 1 / 2 / 8 torch threads, both argument orders
        # and with the rows handed over as float32 and as float64 (its covariance is computed in the rows' dtype,
        # data.py:44): the interval its own value moves in is stored, and the device value must lie INSIDE it.  (Threads move
        # the reference by 1e-8; f32 against f64 rows by 2.6e-4 / 3.6e-4 on the two strongly rank-deficient cases - the
        # square roots of the rounding dust its f32 torch.cov leaves in the null space, fad.py:30 - and the device value
        # coincides with the reference's float64-rows value.)
        lo, hi = float(g[f"{name}/ref_spread_min"]), float(g[f"{name}/ref_spread_max"])
        slack = fad_exact_tol(exact, scale)
        for got in (fad, swapped):
            assert lo - slack <= got <= hi + slack, (got, lo, hi)
        f64_values = g[f"{name}/ref_spread_f64"]
        assert np.abs(f64_values - fad).max() <= 1e-6 * abs(fad) + slack          # = the reference fed float64 rows


def test_fad_warns_when_rows_do_not_exceed_dimensions(am):
    """n <= D on float32 rows is where the reference's own value moves by up to 1.5e-4 with its add() batch
    size and by 2.6e-4 / 3.6e-4 between f32 and f64 rows (profiles/r6/fad_f32_probe.txt, reference fad.py:28-31 + data.py:44);
    the build returns the dust-free value and says so - once per call, for float32-derived statistics only."""
    import warnings
    for name, (kind, seed, nr, nc, d) in gi.FAD_CASES.items():
        ref, cand = gi.pair(kind, seed, nr, nc, d)
        a, b = amd_of(am, cand, False), amd_of(am, ref, False)
        if min(nr, nc) <= d:
            with pytest.warns(RuntimeWarning, match="no more rows than dimensions") as rec:
                am.frechet_distance(a, b)
            assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
            a64, b64 = amd_of(am, cand.astype(np.float64), False), amd_of(am, ref.astype(np.float64), False)
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                am.frechet_distance(a64, b64)                                # float64 rows: no dust, no warning
        else:
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                am.frechet_distance(a, b)


def test_fad_properties(am):
    x, y = gi.pair("randn", 71, 5000, 5000, 128)
    a, b = amd_of(am, x, False), amd_of(am, y, False)
    scale = float(a.cov.trace() + b.cov.trace())
    assert abs(am.frechet_distance(a, a)) <= 1e-10 * scale           # identical Gaussians
    f1 = am.frechet_distance(a, b)
    a3, b3 = amd_of(am, 3 * x, False), amd_of(am, 3 * y, False)
    assert abs(am.frechet_distance(a3, b3) - 9 * f1) <= 1e-5 * 9 * f1    # FD(sX, sY) = s^2 FD(X, Y)
    assert am.metrics.fad.last_info["iters"] <= 20


def test_apa_vs_golden(am, golden):
    g = golden("apa")
    for t, want in zip(g["table_in"], g["table_out"]):
        assert am.metrics.apa._apa(*t) == want
    d = 64
    ref, anti = gi.randn(51, 1500, d), gi.randn(52, 1500, d, 1.2, 0.3)
    b, c = amd_of(am, ref, False), amd_of(am, anti, False)
    for i in range(4):
        sc, sh = g[f"three_set_{i}/params"]
        a = amd_of(am, gi.randn(53 + i, 1200, d, sc, sh), False)
        want = float(g[f"three_set_{i}/apa"])
        assert abs(am.apa(a, b, c) - want) <= REL * max(abs(want), 1e-3)
        assert abs(am.apa(a, b, c, am.apa_compute_d_x_xp(b, c)) - want) <= REL * max(abs(want), 1e-3)


# ----------------------------------------------------------------- KD
@pytest.mark.parametrize("name", list(gi.KD_CASES))
def test_kd_vs_golden(am, golden, name):
    g = golden("kd")
    kind, seed, n1, n2, d = gi.KD_CASES[name]
    f2, f1 = gi.pair(kind, seed, n2, n1, d)
    a, b = amd_of(am, f1), amd_of(am, f2)
    res = am.kernel_distance(a, b)
    for key, gk in (("kernel_distance_mean", "mean"), ("kernel_distance_std", "std")):
        want = float(g[f"{name}/{gk}"])
        assert abs(res[key] - want) <= max(REL * abs(want), KD_ABS_FLOOR), (key, res[key], want)
    # per-subset values against the reference's own mmds[100]
    import oracle
    i1, i2 = oracle.draw_subsets(n1, n2)
    mm = am.hip_ops.kd_poly(a.embeddings, b.embeddings, dev(i1), dev(i2), 1.0 / d, 1.0, 3).cpu().numpy()
    assert np.all(np.abs(mm - g[f"{name}/mmds"]) <= np.maximum(REL * np.abs(g[f"{name}/mmds"]), KD_ABS_FLOOR))


@pytest.mark.parametrize("name", [n for n, c in gi.KD_CASES.items() if c[2] <= 3000])
def test_kd_rbf_vs_golden(am, golden, name):
    """RBF kernel option (reference kd.py:86-109), against the reference's own outputs."""
    g = golden("kd")
    kind, seed, n1, n2, d = gi.KD_CASES[name]
    f2, f1 = gi.pair(kind, seed, n2, n1, d)
    keys = [k for k in g.files if k.startswith(f"{name}/rbf_") and k.endswith("/mean")]
    assert keys
    for key in keys:
        sigma = float(key.split("rbf_")[1].split("/")[0])
        res = am.kid_features_to_metric(dev(f1), dev(f2), kernel_type="rbf", kid_sigma=sigma)
        for k2, gk in (("kernel_distance_mean", key), ("kernel_distance_std", key.replace("/mean", "/std"))):
            want = float(g[gk])
            assert abs(res[k2] - want) <= max(REL * abs(want), KD_ABS_FLOOR), (k2, sigma, res[k2], want)


def test_kd_argument_order_and_kwargs(am):
    f2, f1 = gi.pair("randn", 32, 3000, 3000, 64)
    import oracle
    ab = am.kid_features_to_metric(dev(f1), dev(f2))
    ba = am.kid_features_to_metric(dev(f2), dev(f1))
    assert ab != ba                                                  # the two rng draws swap
    o = oracle.kid_from_features(f1, f2, subsets=7, subset_size=500, degree=2, gamma=0.01, coef0=0.5, seed=99)
    r = am.kid_features_to_metric(dev(f1), dev(f2), kid_subsets=7, kid_subset_size=500, kid_degree=2,
                                  kid_gamma=0.01, kid_coef0=0.5, rng_seed=99)
    for key in o:
        assert abs(o[key] - r[key]) <= max(REL * abs(o[key]), KD_ABS_FLOOR)
    with pytest.raises(NotImplementedError):
        am.kid_features_to_metric(dev(f1), dev(f2), kernel_type="laplace")


# ----------------------------------------------------------------- symmetric k-NN path
def test_knn_symmetric_path_bit_exact(am):
    """N >= 8192, D >= 128 self-distance radii take the symmetric kernel (half the tile pairs +
    mirrored candidates); it must match the C model bit for bit, like the general kernel."""
    from oracle import exact
    x = gi.randn(81, 8500, 136)                      # D % 32 != 0 exercises the tail instantiation too
    for k in (3, 10):
        r = am.nearest_neighbour_distances(dev(x), k).cpu().numpy()
        assert np.array_equal(r.view(np.uint32), exact.knn_radii(x, k).view(np.uint32))
    dup = np.concatenate([x[:4300], x[:4300]])       # every row has an exact duplicate: zero radii, exact ties
    r = am.nearest_neighbour_distances(dev(dup), 1).cpu().numpy()
    assert np.array_equal(r.view(np.uint32), exact.knn_radii(dup, 1).view(np.uint32))


def test_knn_symmetric_fallbacks_agree():
    """General kernel, symmetric kernel, symmetric kernel with a 2-slot candidate buffer (every row overflows
    -> exact fix-up kernel) and with a 16-entry workgroup queue (direct per-row pushes), and the f16 filter path
    (plain, with overflowing candidate buffers, with overflowing queue regions -> spill queue, with an overflowing spill
    queue -> exact fix-up) give identical bits.
    The knobs are process-wide environment variables, hence subprocesses."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = dict(os.environ, AB_ROWS="9000", AB_DIM="160", AB_K="5", AB_REPS="1")
    outs = []
    exact = {"AM_KNN_FAST": "0"}                      # the exact kernels (9000 x 160 takes the f16 filter path since round 3)
    fast = {"AM_KNN_FAST_MIN_ROWS": "1000"}           # the f16 filter + exact verification path (pairwise_fast.h)
    for extra in (dict(exact, AM_KNN_SYM_MIN_ROWS="100000000"), exact, dict(exact, AM_KNN_SYM_CAP="2"), dict(exact, AM_KNN_SYM_QCAP="16"),
                  {}, fast, dict(fast, AM_KNN_SYM_CAP="2"), dict(fast, AM_KNN_SYM_QCAP="16"),
                  dict(fast, AM_KNN_SYM_QCAP="16", AM_KNN_FAST_OVCAP="64")):
        res = subprocess.run([sys.executable, os.path.join(root, "tools", "ab_knn.py")], env=knob_env(base, extra),
                             capture_output=True, text=True, timeout=600)
        m = re.search(r"radii sha1 ([0-9a-f]+)", res.stdout)
        assert m, res.stdout + res.stderr
        outs.append(m.group(1))
    assert len(set(outs)) == 1, outs


def test_cross_kernel_schedules_agree():
    """The exact membership-count kernel under its three schedules - plain pointer staging (variant 0), the
    register-staged early-commit pipeline (35) and the LDS-direct pipeline (99, buffer_load ... lds with
    XOR-swizzled rows) - and the filter-and-verify path produce identical counts, row flags and row minima."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = dict(os.environ, AB_ROWS="5000", AB_DIM="160", AB_WANT_MIN="1")
    outs = []
    # the fourth run is the production path at this size: the f16 filter + exact verification (pairwise_fast.h)
    for extra in ({"AM_ENGINE_VARIANT": "0", "AM_PRDC_FAST": "0"}, {"AM_ENGINE_VARIANT": "35", "AM_PRDC_FAST": "0"},
                  {"AM_ENGINE_VARIANT": "99", "AM_PRDC_FAST": "0"}, {}):
        res = subprocess.run([sys.executable, os.path.join(root, "tools", "ab_cross.py")],
                             env=knob_env(base, extra), capture_output=True, text=True, timeout=600)
        m = re.search(r"sha1 ([0-9a-f]+)", res.stdout)
        assert m, res.stdout + res.stderr
        outs.append(m.group(1))
    assert len(set(outs)) == 1, outs


@pytest.mark.parametrize("rows,dim,k", [(40000, 128, 5), (33000, 200, 10)])
def test_knn_filter_path_bit_identical_at_production_sizes(rows, dim, k):
    """At >= 32768 rows am_knn_radii_f32 runs the f16 filter sweep + exact verification; its radii equal the exact
    symmetric kernel's bit for bit."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = dict(os.environ, AB_ROWS=str(rows), AB_DIM=str(dim), AB_K=str(k), AB_REPS="1")
    outs = []
    for extra in ({"AM_KNN_FAST": "0"}, {}):
        res = subprocess.run([sys.executable, os.path.join(root, "tools", "ab_knn.py")], env=knob_env(base, extra),
                             capture_output=True, text=True, timeout=600)
        m = re.search(r"radii sha1 ([0-9a-f]+)", res.stdout)
        assert m, res.stdout + res.stderr
        outs.append(m.group(1))
    assert outs[0] == outs[1], outs


@pytest.mark.parametrize("data", ["clustered", "scales", "dups", "lowrank", "unit"])
def test_filter_paths_bit_identical_on_adversarial_data(data):
    """The f16 filter + exact verification forms of both PRDC kernels (production path at these sizes) against the exact
    f32 kernels on inputs chosen to stress the error bound and the queues: tight clusters (cancellation noise, clamps,
    ties), row norms spread over four orders of magnitude with zero rows (and a candidate set 1000x smaller than the
    reference), exact duplicates, a near-rank-4 set with a large offset, unit-norm rows.  Radii, counts and flags must
    agree bit for bit (sha1 of the outputs)."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = dict(os.environ, AB_ROWS="33000", AB_DIM="128", AB_K="5", AB_REPS="1", AB_DATA=data, AB_WANT_MIN="1")
    for tool, pattern, off in (("ab_knn.py", r"radii sha1 ([0-9a-f]+)", {"AM_KNN_FAST": "0"}),
                               ("ab_cross.py", r"sha1 ([0-9a-f]+)", {"AM_PRDC_FAST": "0", "AM_KNN_FAST": "0"})):
        outs = []
        for extra in (off, {}):
            res = subprocess.run([sys.executable, os.path.join(root, "tools", tool)], env=knob_env(base, extra),
                                 capture_output=True, text=True, timeout=900)
            m = re.search(pattern, res.stdout)
            assert m, res.stdout + res.stderr
            outs.append(m.group(1))
        assert outs[0] == outs[1], (tool, data, outs)


def test_membership_filter_survives_undecidable_inputs():
    """Found by tools/fuzz_filter.py: a candidate set three orders of magnitude smaller than the reference makes the
    error bound useless for most rows - more than 2^31 pairs reach the spill path, whose 32-bit counter wrapped and
    sent writes out of bounds.  The path must notice, hand the call to the exact kernel, and return its bits."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = dict(os.environ, AB_ROWS="52000", AB_DIM="200", AB_K="3", AB_REPS="1", AB_DATA="scales", AB_SEED="290",
                AB_WANT_MIN="1")
    outs = []
    for extra in ({"AM_PRDC_FAST": "0", "AM_KNN_FAST": "0"}, {}):
        res = subprocess.run([sys.executable, os.path.join(root, "tools", "ab_cross.py")], env=knob_env(base, extra),
                             capture_output=True, text=True, timeout=900)
        m = re.search(r"sha1 ([0-9a-f]+)", res.stdout)
        assert m, res.stdout[-500:] + res.stderr[-1500:]
        outs.append(m.group(1))
    assert outs[0] == outs[1], outs


@pytest.mark.parametrize("n_ref,n_cand", [(70000, 1500), (1500, 70000), (33000, 3100)])    # (>= 1e8 pairs: the filter's threshold at D = 64)
def test_membership_filter_unequal_sets_bit_exact(am, n_ref, n_cand):
    """Very unequal set sizes through the 256-row filter engine (one column chunk / two row blocks / ragged edges):
    counts, flags and row minima equal the C model bit for bit (radii chosen so that a few percent of the pairs count)."""
    from oracle import exact
    assert am.hip_ops.prdc_path(n_ref, n_cand, 64) == 3
    ref, cand = gi.pair("shifted", 700 + n_cand % 97, n_ref, n_cand, 64)
    rng = np.random.default_rng(5)
    r_ref = (9.0 + rng.random(n_ref) * 2.5).astype(np.float32)           # around the bulk of the distances (~11.5)
    r_cand = (9.0 + rng.random(n_cand) * 2.5).astype(np.float32)
    col, rany, rcov, rmin = am.hip_ops.prdc_counts(dev(ref), dev(cand), dev(r_ref), dev(r_cand), want_min=True)
    ecol, eany, emin = exact.prdc_counts(ref, cand, r_ref, r_cand)
    assert int(ecol.sum()) > 1000
    assert np.array_equal(col.cpu().numpy(), ecol)
    assert np.array_equal(rany.cpu().numpy(), eany)
    assert np.array_equal(rmin.cpu().numpy().view(np.uint32), emin.view(np.uint32))
    assert np.array_equal(rcov.cpu().numpy().astype(bool), emin < r_ref)


# ----------------------------------------------------------------- PCA projection (n_pca)
def test_incremental_pca_vs_reference(am, golden):
    """Device PCA against the reference's scikit-learn based IncrementalPCA: first fit, incremental update,
    projection.  Components are unit vectors with sklearn's sign convention (compared absolutely)."""
    g = golden("pca")
    x1 = gi.decaying(61, 500, 24, decades=1.5, shift=0.3)
    x2 = gi.decaying(62, 300, 24, decades=1.5, scale=1.2, shift=0.1)
    xt = gi.decaying(63, 40, 24, decades=1.5)
    pca = am.IncrementalPCA(n_components=6)
    for step, x in (("fit1", x1), ("fit2", x2)):
        pca.partial_fit(dev(x))
        assert pca.n_samples_seen_ == int(g[f"{step}/n_samples_seen_"])
        np.testing.assert_allclose(pca.singular_values_.cpu().numpy(), g[f"{step}/singular_values_"], rtol=2e-5)
        np.testing.assert_allclose(pca.components_.cpu().numpy(), g[f"{step}/components_"], atol=5e-5)
        np.testing.assert_allclose(pca.mean_.cpu().numpy(), g[f"{step}/mean_"], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(pca.var_.cpu().numpy(), g[f"{step}/var_"], rtol=1e-5)
        np.testing.assert_allclose(pca.explained_variance_.cpu().numpy(), g[f"{step}/explained_variance_"], rtol=5e-5)
        np.testing.assert_allclose(pca.explained_variance_ratio_.cpu().numpy(), g[f"{step}/explained_variance_ratio_"],
                                   rtol=5e-5)
        assert abs(pca.noise_variance_ - float(g[f"{step}/noise_variance_"])) <= 5e-5 * float(g[f"{step}/noise_variance_"])
        y = pca.transform(dev(xt))
        assert y.dtype == torch.float64 and y.shape == (40, 6)
        np.testing.assert_allclose(y.cpu().numpy(), g[f"{step}/transform"], atol=1e-4)
    clone = am.IncrementalPCA(n_components=6)
    clone.__setstate__(pca.__getstate__())
    assert torch.equal(clone.transform(dev(xt)).cpu(), pca.transform(dev(xt)).cpu())
    with pytest.raises(ValueError):
        am.IncrementalPCA(n_components=30).partial_fit(dev(x1))       # more components than features


def test_knn_and_prdc_on_clustered_data_bit_exact(am):
    """Adversarial input for the filters of the symmetric kernel: 20 tight clusters (intra-cluster squared
    distances ~1e-4 of the squared norms, so the matmul-form d2 is dominated by cancellation noise, clamps to 0
    and ties abound).  Radii, counts and flags must still equal the C model bit for bit."""
    from oracle import exact
    rng = np.random.default_rng(123)
    centers = rng.standard_normal((20, 128)).astype(np.float32)
    lab = rng.integers(0, 20, 8600)
    x = (centers[lab] + 1e-3 * rng.standard_normal((8600, 128))).astype(np.float32)
    y = (centers[rng.integers(0, 20, 8300)] + 1.5e-3 * rng.standard_normal((8300, 128))).astype(np.float32)
    k = 5
    rx = am.nearest_neighbour_distances(dev(x), k)
    ry = am.nearest_neighbour_distances(dev(y), k)
    ex, ey = exact.knn_radii(x, k), exact.knn_radii(y, k)
    assert np.array_equal(rx.cpu().numpy().view(np.uint32), ex.view(np.uint32))
    assert np.array_equal(ry.cpu().numpy().view(np.uint32), ey.view(np.uint32))
    col, rany, rcov, rmin = am.hip_ops.prdc_counts(dev(x), dev(y), rx, ry, want_min=True)
    ecol, eany, emin = exact.prdc_counts(x, y, ex, ey)
    assert np.array_equal(col.cpu().numpy(), ecol)
    assert np.array_equal(rany.cpu().numpy(), eany)
    assert np.array_equal(rmin.cpu().numpy().view(np.uint32), emin.view(np.uint32))
    assert np.array_equal(rcov.cpu().numpy().astype(bool), emin < ex)
    col3, rany3, rcov3 = am.hip_ops.prdc_counts(dev(x), dev(y), rx, ry)
    assert torch.equal(col, col3) and torch.equal(rany, rany3) and torch.equal(rcov, rcov3)


# ----------------------------------------------------------------- scale and odd shapes
def test_prdc_self_consistency_300k(am):
    """Beyond the BASELINE size (config 4 shards 1M rows over 8 GPUs): 300k x 256 on one GPU exercises the
    64-bit indexing, the larger window / queue plans and the candidate buffers of the symmetric kernel."""
    torch.manual_seed(1)
    x = torch.randn(300000, 256, device="cuda:0")
    a = am.AudioMetricsData(True)
    a.add(x)
    res = am.prdc(a, a, 3)
    assert (res["precision"], res["recall"], res["coverage"]) == (1.0, 1.0, 1.0)
    total = round(res["density"] * 3 * 300000)
    assert 900000 - 100 <= total <= 900000, total


@pytest.mark.parametrize("n_ref,n_cand,d,k", [(2, 3, 1, 1), (5, 4, 2, 2), (130, 127, 3, 4), (129, 257, 33, 7),
                                              (64, 1000, 7, 1), (1000, 64, 130, 9)])
def test_prdc_odd_shapes_bit_exact(am, n_ref, n_cand, d, k):
    """Tiny sets, D of 1..3, rows just past a tile edge, very unequal set sizes."""
    from oracle import exact
    ref, cand = gi.pair("shifted", 300 + d, n_ref, n_cand, d)
    a, b = amd_of(am, ref), amd_of(am, cand)
    res = am.prdc(a, b, k)
    want, aux = exact.prdc(ref, cand, k)
    assert np.array_equal(a.get_radii(k).cpu().numpy().view(np.uint32), aux["r_ref"].view(np.uint32))
    assert np.array_equal(b.get_radii(k).cpu().numpy().view(np.uint32), aux["r_cand"].view(np.uint32))
    assert res == want


def test_embedding_buffer_growth_and_views(am):
    """Many small adds (amortised-doubling HBM buffer) keep row order, stats and cached radii semantics."""
    x = gi.randn(400, 3000, 20)
    a = am.AudioMetricsData(True)
    s = 0
    for b in [1, 2, 3, 500, 31, 700, 1, 1762]:
        a.add(dev(x[s:s + b]))
        s += b
    assert s == 3000 and a.n == 3000
    np.testing.assert_array_equal(a.embeddings.cpu().numpy(), x)
    r1 = a.get_radii(3)
    a.add(dev(x[:10]))                              # reference quirk: the radii cache is NOT invalidated
    assert a.get_radii(3) is r1 and a.embeddings.shape[0] == 3010
    b = am.AudioMetricsData(False)
    b.add(dev(x))
    assert b.embeddings is None and b.get_radii(3) is None


def test_kernel_clock_counts_tile_kernel_launches(am):
    """am_kernel_clock_*: off by default (nothing recorded); when on, one record per tile-kernel launch with a positive
    duration no longer than the host-side bracket of the whole entry point; reading resets the record."""
    from audio_metrics_amd import hip_ops as ops
    x = torch.as_tensor(gi.randn(71, 4000, 64)).cuda()
    y = torch.as_tensor(gi.randn(72, 3000, 64)).cuda()
    ops.kernel_clock_enable(False)
    r_off = ops.knn_radii(x, 3)
    assert ops.kernel_clock_read(ops.KERNEL_KNN) == (0, 0.0)
    ops.kernel_clock_enable(True)
    try:
        with ops.KernelTimer() as timer:
            r_x = ops.knn_radii(x, 3)
            r_y = ops.knn_radii(y, 3)
            ops.prdc_counts(x, y, r_x, r_y)
        outer = timer.summary()
        n_knn, ms_knn = ops.kernel_clock_read(ops.KERNEL_KNN)
        n_cross, ms_cross = ops.kernel_clock_read(ops.KERNEL_PRDC_CROSS)
        assert n_knn == 2 and n_cross == 1
        # (both sides are hipEvent intervals: 5 % + 20 us for their resolution)
        assert 0.0 < ms_knn <= outer["am_knn_radii_f32"][1] * 1.05 + 0.02
        assert 0.0 < ms_cross <= outer["am_prdc_counts_f32"][1] * 1.05 + 0.02
        assert ops.kernel_clock_read(ops.KERNEL_KNN) == (0, 0.0)
        assert torch.equal(r_off, r_x)                       # the clock does not change results
        with pytest.raises(am._lib.HipLibraryError):
            ops.kernel_clock_read(7)
    finally:
        ops.kernel_clock_enable(False)


# ----------------------------------------------------------------- regression tests for reviewer findings
def test_single_row_recompute_then_merge(am):
    """add(1 row) -> recompute_stats() leaves the reference's (1, 1) zero covariance (data.py:56); the next merge must
    treat it as a D x D zero matrix, not hand an 8-byte buffer to a kernel that writes D*D doubles."""
    import oracle
    x = gi.randn(71, 40, 24, 1.2, 0.3)
    d = am.AudioMetricsData(True)
    o = oracle.OracleData(True)
    d.add(dev(x[:1])); o.add(torch.as_tensor(x[:1]))
    d.recompute_stats(); o.recompute_stats()
    assert tuple(d.cov.shape) == (1, 1)
    d.add(dev(x[1:33])); o.add(torch.as_tensor(x[1:33]))
    other = am.AudioMetricsData(True)
    other.add(dev(x[33:]))
    d += other
    o.merge(oracle.OracleData(True).add(torch.as_tensor(x[33:])))
    assert d.n == o.n == 40 and tuple(d.cov.shape) == (24, 24)
    np.testing.assert_allclose(d.mean.cpu().numpy(), o.mean.numpy(), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(d.cov.cpu().numpy(), o.cov.numpy(), rtol=1e-5, atol=1e-7)
    with pytest.raises(ValueError):
        am.hip_ops.stats_merge(3, d.mean, torch.zeros((1, 1), dtype=torch.float64, device="cuda:0"), 2, d.mean, d.cov)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_kernels_run_on_the_tensors_device_not_the_current_one(am):
    """Tensors on cuda:1 while cuda:0 is the thread's current device: every entry point must launch on cuda:1's stream."""
    from oracle import exact
    torch.cuda.set_device(0)
    x = gi.randn(72, 3000, 64)
    y = gi.randn(73, 2500, 64, 1.1, 0.1)
    a, b = am.AudioMetricsData(True, device="cuda:1"), am.AudioMetricsData(True, device="cuda:1")
    a.add(torch.as_tensor(x).to("cuda:1"))
    b.add(torch.as_tensor(y).to("cuda:1"))
    assert a.cov.device.index == 1
    res = am.prdc(a, b, 5)
    want, _ = exact.prdc(x, y, 5)
    assert res == want
    assert abs(am.frechet_distance(a, b) - am.frechet_distance(a.to("cuda:0"), b.to("cuda:0"))) < 1e-9


def test_frechet_enqueue_matches_blocking_call(am):
    """am_frechet_enqueue_f64 (side stream, device-side stopping rule, no host polling) against am_frechet_f64, including
    an ill-conditioned product that needs more than the first block of iterations."""
    ops = am.hip_ops
    for kind, d in (("randn", 128), ("decay", 128)):
        ref, cand = gi.pair(kind, 81, 3000, 3000, d)
        a, b = amd_of(am, cand, False), amd_of(am, ref, False)
        sync = ops.frechet(a.mean, a.cov, b.mean, b.cov)
        job = ops.frechet_async(a.mean, a.cov, b.mean, b.cov)
        got = job.result()
        assert got["fd"] == sync["fd"] and got["iters"] == sync["iters"], (kind, got, sync)


def test_own_eigensolver_and_projection(am):
    """am_eigh_sym_f64 (one-sided Jacobi) against numpy's eigh on Gram matrices of different shapes (odd size, rank
    deficient, D = 512), and am_project_f64 against the f64 matrix product."""
    ops = am.hip_ops
    rng = np.random.default_rng(9)
    for d, rows in ((7, 50), (24, 500), (129, 60), (512, 3000)):
        x = rng.standard_normal((rows, d)) * np.logspace(0, -2, d)
        g = x.T @ x
        evals, evecs = ops.eigh_descending(torch.as_tensor(g).to("cuda:0"))
        evals, evecs = evals.cpu().numpy(), evecs.cpu().numpy()
        want = np.linalg.eigvalsh(g)[::-1]
        np.testing.assert_allclose(evals, want, rtol=1e-9, atol=1e-10 * want[0])
        assert np.all(np.diff(evals) <= 0)
        np.testing.assert_allclose(evecs @ evecs.T, np.eye(d), atol=1e-10)                 # orthonormal rows
        np.testing.assert_allclose(evecs @ g @ evecs.T, np.diag(evals), atol=1e-9 * want[0])
    x = rng.standard_normal((1000, 70)).astype(np.float32)
    mean = rng.standard_normal(70)
    comp = rng.standard_normal((9, 70))
    got = ops.project(torch.as_tensor(x).to("cuda:0"), torch.as_tensor(mean).to("cuda:0"), torch.as_tensor(comp).to("cuda:0"))
    np.testing.assert_allclose(got.cpu().numpy(), (x.astype(np.float64) - mean) @ comp.T, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("rows,dim,k", [(2000, 64, 5), (9000, 128, 3), (33000, 128, 5)])
def test_prepared_sets_change_no_bit(am, rows, dim, k):
    """am_prepare_set_f32 + the *_prepared_* entry points (norms, maxima and scaled f16 copy computed once and shared)
    against the plain entry points: exact general kernel, exact symmetric kernel and the f16 filter forms; also a row
    shard of a prepared reference set, and the partitioned k-NN."""
    ops = am.hip_ops
    x, y = dev(gi.randn(201, rows, dim)), dev(gi.randn(202, rows - 37, dim, 1.05, 0.05))
    px, py = ops.prepare(x), ops.prepare(y)
    rx, ry = ops.knn_radii(x, k), ops.knn_radii(y, k)
    assert torch.equal(rx, ops.knn_radii(x, k, prepared=px)) and torch.equal(ry, ops.knn_radii(y, k, prepared=py))
    plain = ops.prdc_counts(x, y, rx, ry)
    shared = ops.prdc_counts(x, y, rx, ry, prepared_ref=px, prepared_cand=py)
    assert all(torch.equal(a, b) for a, b in zip(plain, shared))
    lo, hi = rows // 3, rows // 3 + rows // 2                      # a row shard of the prepared reference set
    part = ops.prdc_counts(x[lo:hi], y, rx[lo:hi], ry, prepared_ref=px.rows(lo, hi), prepared_cand=py)
    want = ops.prdc_counts(x[lo:hi], y, rx[lo:hi], ry)
    assert all(torch.equal(a, b) for a, b in zip(part, want))
    if ops.knn_sym_eligible(rows, dim, k):
        nparts = 3
        bounds = torch.cat([ops.knn_bounds(x, k, rows * p // nparts, rows * (p + 1) // nparts - rows * p // nparts, prepared=px)
                            for p in range(nparts)])
        lists = torch.stack([ops.knn_sym_part(x, k, p, nparts, bounds, prepared=px) for p in range(nparts)])
        assert torch.equal(ops.knn_lists_finish(lists, x, k), rx)


# ----------------------------------------------------------------- one call = one evaluate()
@pytest.mark.parametrize("n_ref,n_cand,d,k", [(2600, 2300, 96, 4), (9000, 8800, 128, 5), (300, 500, 24, 3)])
def test_fused_evaluate_equals_separate_entry_points(am, n_ref, n_cand, d, k):
    """am_evaluate_f32 (the whole FAD + KD + PRDC chain as one stream-ordered call with one read-back,
    audio_metrics.py:254-274) against the same entry points called one by one: identical values (same kernels, same
    order), cold and with the reference side handed in (cached statistics / radii, data.py:60-66)."""
    from audio_metrics_amd.distributed import evaluate_sharded, evaluate_single
    ops = am.hip_ops
    ref, cand = (dev(x) for x in gi.pair("randn", 91, n_ref, n_cand, d))
    kw = dict(nearest_k=k, kid_subsets=12, kid_subset_size=200)
    fused = evaluate_sharded(ref, cand, **kw)
    apart = evaluate_sharded(ref, cand, fused=False, **kw)
    assert list(fused) == ["fad", "kernel_distance_mean", "kernel_distance_std", "precision", "recall", "density", "coverage"]
    for key in fused:
        if key == "fad":        # (one-shot covariance here, column sums + centred scatter there: the same kernels, one more division)
            assert abs(fused[key] - apart[key]) <= 1e-9 * abs(apart[key]), key
        else:
            assert fused[key] == apart[key], key
    for metrics in (("fad", "kd"), ("prdc",), ("kd",), ("fad",)):
        part = evaluate_sharded(ref, cand, metrics=metrics, **kw)
        assert part == {key: fused[key] for key in part}, metrics
    # warm: the reference side's statistics and radii come from the object, the candidate's are written into tensors
    a, b = am.AudioMetricsData(True), am.AudioMetricsData(True)
    a.add(cand)
    b.add(ref)
    r_out = torch.empty(n_cand, dtype=torch.float32, device=cand.device)
    warm = evaluate_single(ref, cand, ("fad", "kd", "prdc"), k, ops, 12, 200,
                           given_ref={"mean": b.mean, "cov": b.cov, "radii": b.get_radii(k)},
                           given_cand={"mean": a.mean, "cov": a.cov, "radii_out": r_out})
    assert torch.equal(r_out, a.get_radii(k))
    want = {"fad": am.frechet_distance(a, b)}
    want.update(am.kid_features_to_metric(cand, ref, kid_subsets=12, kid_subset_size=200))
    want.update(am.prdc(b, a, k))
    assert warm == want


def test_fused_evaluate_finishes_an_ill_conditioned_frechet_solve(am):
    """A covariance product that needs more Newton-Schulz iterations than am_evaluate_f32 enqueues (stop code 0) is finished
    by the stand-alone solver on the statistics the chain wrote: same value as frechet_distance()."""
    from audio_metrics_amd.distributed import evaluate_sharded
    ref, cand = (dev(x) for x in gi.pair("decay", 24, 2000, 2000, 128))
    got = evaluate_sharded(ref, cand, metrics=("fad", "kd"), kid_subsets=4, kid_subset_size=100)
    a, b = amd_of(am, cand.cpu().numpy(), False), amd_of(am, ref.cpu().numpy(), False)
    assert abs(got["fad"] - am.frechet_distance(a, b)) <= 1e-9 * abs(got["fad"])
