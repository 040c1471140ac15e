"""FAD-infinity on the device: gathered statistics, the batched Newton-Schulz solve, and frechet_distance_inf end to end.

The float64 oracle is this module's own and is the definition, not the code under test: numpy mean / np.cov of the
gathered rows, tr sqrt(Cx Cy) as the sum of the square roots of the clipped real eigenvalues of Cx Cy, np.linalg.lstsq for
the fit in 1/n.  Indices always come from the implementation (fad_inf_subset_indices), never from a generator of the
test's, so the draw can change without touching a test."""
import warnings

import numpy as np
import pytest
import torch

import inputs as gi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FAD_EXACT_REL = 1e-6      # the bar the single solve meets (test_gpu_parity.py): device value against the f64 definition ...
FAD_TERMS_REL = 1e-7      # ... plus the f32 rounding of the centred inputs, relative to tr Sx + tr Sy


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    audio_metrics_amd._lib.load()
    return audio_metrics_amd


# ------------------------------------------------------------------ the oracle
def oracle_stats(rows):
    rows = np.asarray(rows, dtype=np.float64)
    d = rows.shape[1]
    return rows.mean(0), (np.cov(rows, rowvar=False).reshape(d, d) if len(rows) > 1 else np.zeros((d, d)))


def oracle_fd(mx, cx, my, cy):
    lam = np.linalg.eigvals(cx @ cy)
    tr_sqrt = np.sqrt(np.clip(lam.real, 0.0, None)).sum()
    return float(((mx - my) ** 2).sum() + np.trace(cx) + np.trace(cy) - 2.0 * tr_sqrt)


def oracle_fit(sizes, values):
    sizes = np.asarray(sizes, dtype=np.float64)
    design = np.stack([1.0 / sizes, np.ones_like(sizes)], axis=1)
    (slope, intercept), *_ = np.linalg.lstsq(design, np.asarray(values, dtype=np.float64), rcond=None)
    fitted = design @ np.array([slope, intercept])
    r2 = 1.0 - ((values - fitted) ** 2).sum() / ((values - np.mean(values)) ** 2).sum()
    return float(intercept), float(slope), float(r2), np.linalg.pinv(design)


def spectrum_rows(seed, n, d, s=0.0, dtype=np.float32):
    """decaying spectrum 1 / sqrt(1 + j); the candidate is scaled by 1 + s and shifted by s"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)) / np.sqrt(1.0 + np.arange(d))
    return (x * (1.0 + s) + s).astype(dtype)


def data_of(am, rows, store=True):
    a = am.AudioMetricsData(store_embeddings=store)
    a.add(torch.as_tensor(rows).to(DEV))
    return a


# ------------------------------------------------------------------ 1. gathered statistics against float64
GATHER_CASES = [
    (20_000, 512, 512, [600, 5_000, 20_000], np.float32),
    (8_000, 128, 128, [1, 2, 129, 8_000], np.float32),
    (3_001, 100, 100, [37, 3_001], np.float32),
    (8_000, 64, 64, [65, 4_000, 8_000], np.float64),
]


def check_gathered(am, x, xd, idx, offsets, f64):
    means, covs = am.hip_ops.stats_gather(xd, idx, offsets)
    host_idx = idx.cpu().numpy()
    for b in range(len(offsets) - 1):
        rows = x[host_idx[offsets[b]:offsets[b + 1]]]
        want_mean, want_cov = oracle_stats(rows)
        got_mean, got_cov = means[b].cpu().numpy(), covs[b].cpu().numpy()
        n_b = offsets[b + 1] - offsets[b]
        scale = float(np.abs(want_cov).max()) if n_b > 1 else 1.0
        print(f"gather N={x.shape} n_b={n_b} f64={f64}: mean err {np.abs(got_mean - want_mean).max():.3e} "
              f"cov err {np.abs(got_cov - want_cov).max():.3e} (scale {scale:.3e}) "
              f"trace rel {abs(np.trace(got_cov) - np.trace(want_cov)) / max(np.trace(want_cov), 1e-300):.3e}")
        if n_b == 1:
            assert not got_cov.any()                                       # one row -> zero covariance, as am_stats_f32
        if f64:
            assert np.abs(got_mean - want_mean).max() <= 1e-13 * max(1.0, np.abs(want_mean).max())
            assert np.abs(got_cov - want_cov).max() <= 1e-12 * max(scale, 1e-30)
        else:
            np.testing.assert_allclose(got_mean, want_mean, rtol=0, atol=1e-12)
            if n_b > 1:
                assert abs(np.trace(got_cov) - np.trace(want_cov)) <= 1e-7 * np.trace(want_cov)
            np.testing.assert_allclose(got_cov, want_cov, rtol=1e-5, atol=1e-6)
        assert np.array_equal(got_cov, got_cov.T)


@pytest.mark.parametrize("n, d, ld, sizes, dtype", GATHER_CASES)
def test_gathered_statistics_vs_float64(am, n, d, ld, sizes, dtype):
    from audio_metrics_amd.metrics.fad import fad_inf_subset_indices
    rng = np.random.default_rng(n + d)
    x = (rng.standard_normal((n, d)) * (0.5 + rng.random(d)) + rng.standard_normal(d)).astype(dtype)
    xd = torch.as_tensor(x).to(DEV)
    assert xd.stride(0) == ld
    idx, offsets = fad_inf_subset_indices(n, sizes, 5, torch.device(DEV))
    check_gathered(am, x, xd, idx, offsets, dtype == np.float64)
    # a hand-made table: repeated and descending indices - the kernel gathers what it is told
    hand = [np.arange(n - 1, -1, -3), np.array([7, 7, 7, 3, 3, n - 1, 0, 7]), np.repeat(np.arange(min(n, 300))[::-1], 2)]
    offsets = [0] + list(np.cumsum([len(h) for h in hand]))
    idx = torch.as_tensor(np.concatenate(hand).astype(np.int64)).to(DEV)
    check_gathered(am, x, xd, idx, [int(o) for o in offsets], dtype == np.float64)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_out_of_range_index_is_a_value_error_not_a_fault(am, dtype):
    n, d = 5_000, 64
    xd = torch.randn((n, d), device=DEV, dtype=dtype)
    good = torch.arange(0, 4_000, device=DEV)
    for bad_value, where in ((n, 1234), (-1, 0), (2 ** 40, 3_999)):
        idx = good.clone()
        idx[where] = bad_value
        with pytest.raises(ValueError, match=r"idx\[%d\]" % where):
            am.hip_ops.stats_gather(xd, idx, [0, 1_500, 4_000])
    means, covs = am.hip_ops.stats_gather(xd, good, [0, 1_500, 4_000])         # the process is still usable
    want = xd[:1_500].to(torch.float64).mean(0)
    assert float((means[0] - want).abs().max()) <= 1e-12


# ------------------------------------------------------------------ 2. the batched solve
def single_record(am, mu_x, cov_x, mu_y, cov_y, max_iter=64, tol=1e-13):
    """the five doubles of am_frechet_enqueue_f64, driven block by block as am_frechet_f64 does"""
    ops, lib = am.hip_ops, am._lib.load()
    d = mu_x.numel()
    nb = lib.am_frechet_workspace_bytes(d)
    ws = torch.empty(nb, dtype=torch.uint8, device=mu_x.device)
    out = torch.zeros(8, dtype=torch.float64, device=mu_x.device)
    first, block = 0, lib.am_frechet_first_block()
    while first < max_iter:
        n_iter = min(block, max_iter - first)
        ops._call(lib, "am_frechet_enqueue_f64", mu_x.device, ops._ptr(mu_x), ops._ptr(cov_x), ops._ptr(mu_y), ops._ptr(cov_y), d,
                  first, n_iter, max_iter, tol, ops._ptr(out), ops._ptr(ws), nb)
        rec = out.cpu().tolist()
        first += n_iter
        if int(rec[4]) != 0:
            break
    return rec[:5]


def solver_pairs(d, count, seed):
    """(mu_x, cov_x, mu_y, cov_y) f64 device tensors: well-conditioned pairs, one rank-deficient (40 rows), one zero"""
    rng = np.random.default_rng(seed)
    pairs = []
    for i in range(count):
        rows_x = 40 if i == 1 else 4 * d + 50 * i
        x = rng.standard_normal((rows_x, d)) * (1.0 + 0.1 * i) / np.sqrt(1.0 + np.arange(d)) + 0.05 * i
        y = rng.standard_normal((4 * d, d)) / np.sqrt(1.0 + np.arange(d))
        (mx, cx), (my, cy) = oracle_stats(x), oracle_stats(y)
        if i == 2:
            cx = np.zeros((d, d))
        pairs.append(tuple(torch.as_tensor(np.ascontiguousarray(t)).to(DEV) for t in (mx, cx, my, cy)))
    return pairs


def test_batch_of_one_equals_the_single_solve_bit_for_bit(am):
    for d, seed in ((512, 1), (100, 2), (64, 3)):
        for mx, cx, my, cy in solver_pairs(d, 2, seed):                   # a well-conditioned and a rank-deficient pair
            single = am.hip_ops.frechet(mx, cx, my, cy)
            rec = single_record(am, mx, cx, my, cy)
            out = torch.zeros((1, 5), dtype=torch.float64, device=DEV)
            batch = am.hip_ops.frechet_batch(mx[None], cx[None], my, cy, out=out)[0]
            assert [batch[k] for k in ("fd", "tr_sqrt", "iters", "resid")] == [single[k] for k in ("fd", "tr_sqrt", "iters", "resid")]
            assert out[0].cpu().tolist() == rec                           # all five doubles of am_frechet_enqueue_f64
            per_set = am.hip_ops.frechet_batch(mx[None], cx[None], my[None], cy[None])[0]
            assert per_set == batch


@pytest.mark.parametrize("b, d", [(7, 512), (25, 100)])
def test_batched_solve_equals_the_single_solves(am, b, d):
    pairs = solver_pairs(d, b, 10 + b)
    mu_x, cov_x, mu_y, cov_y = (torch.stack([p[k] for p in pairs]) for k in range(4))
    got = am.hip_ops.frechet_batch(mu_x, cov_x, mu_y, cov_y)
    stops = set()
    for i, p in enumerate(pairs):
        single, rec = am.hip_ops.frechet(*p), single_record(am, *p)
        print(f"B={b} D={d} set {i}: batch {got[i]['fd']!r} single {single['fd']!r} iters {got[i]['iters']} stop {got[i]['stop']}")
        assert abs(got[i]["fd"] - single["fd"]) <= 1e-12 * abs(single["fd"])
        assert got[i]["stop"] == int(rec[4]) and got[i]["iters"] == single["iters"]
        stops.add(got[i]["stop"])
    assert 3 in stops and 1 in stops                                      # the zero covariance and converged sets are in the mix
    # one reference shared by all sets: the same values as B copies of it
    shared = am.hip_ops.frechet_batch(mu_x, cov_x, mu_y[0], cov_y[0])
    copies = am.hip_ops.frechet_batch(mu_x, cov_x, mu_y[:1].expand(b, d).contiguous(), cov_y[:1].expand(b, d, d).contiguous())
    assert shared == copies


def test_non_finite_set_raises_naming_the_set_and_the_others_are_written(am):
    d, b = 64, 5
    pairs = solver_pairs(d, b, 77)
    mu_x, cov_x, mu_y, cov_y = (torch.stack([p[k] for p in pairs]) for k in range(4))
    good = am.hip_ops.frechet_batch(mu_x, cov_x, mu_y, cov_y)
    cov_x[3, 5, 5] = float("nan")
    with pytest.raises(am._lib.HipLibraryError):
        am.hip_ops.frechet(mu_x[3], cov_x[3], mu_y[3], cov_y[3])
    out = torch.full((b, 5), -7.0, dtype=torch.float64, device=DEV)
    with pytest.raises(am._lib.HipLibraryError, match="set 3"):
        am.hip_ops.frechet_batch(mu_x, cov_x, mu_y, cov_y, out=out)
    rec = out.cpu().tolist()
    assert int(rec[3][4]) == 4
    for i in (0, 1, 2, 4):
        assert rec[i][0] == good[i]["fd"] and int(rec[i][4]) == good[i]["stop"]


# ------------------------------------------------------------------ 3. end to end against the float64 oracle
E2E_CASES = [
    ("d64_s0", 64, 8_000, 15, 1_000, 0.0, np.float32),
    ("d64_s01", 64, 8_000, 15, 1_000, 0.1, np.float32),
    ("d128", 128, 20_000, 15, 2_000, 0.05, np.float32),
    ("d512", 512, 20_000, 8, 2_000, 0.05, np.float32),
    ("d64_f64", 64, 8_000, 15, 1_000, 0.1, np.float64),
]


@pytest.mark.parametrize("tag, d, n, steps, min_n, s, dtype", E2E_CASES)
def test_fad_inf_vs_float64_oracle(am, tag, d, n, steps, min_n, s, dtype):
    from audio_metrics_amd.metrics import fad
    cand, ref = spectrum_rows(0, n, d, s, dtype), spectrum_rows(100, n, d, 0.0, dtype)
    x, y = data_of(am, cand), data_of(am, ref, store=False)
    got = am.frechet_distance_inf(x, y, steps=steps, min_n=min_n, seed=0)
    info = dict(fad.last_info)
    sizes = np.linspace(min_n, n, steps).round().astype(int)
    assert info["sizes"] == [int(m) for m in sizes]
    idx, offsets = fad.fad_inf_subset_indices(n, sizes, 0, torch.device(DEV))       # the subsets the call drew
    host_idx = idx.cpu().numpy()
    my, cy = oracle_stats(ref)
    exact, tol = [], []
    for b in range(steps):
        mx, cx = oracle_stats(cand[host_idx[offsets[b]:offsets[b + 1]]])
        exact.append(oracle_fd(mx, cx, my, cy))
        tol.append(FAD_EXACT_REL * abs(exact[-1]) + FAD_TERMS_REL * (np.trace(cx) + np.trace(cy)))
        print(f"{tag} n_b={sizes[b]}: device {info['fads'][b]!r} exact {exact[-1]!r} |diff| {abs(info['fads'][b] - exact[-1]):.3e} "
              f"tol {tol[-1]:.3e} iters {info['iters'][b]} stop {info['stops'][b]}")
    for b in range(steps):
        assert abs(info["fads"][b] - exact[b]) <= tol[b], (b, info["fads"][b], exact[b], tol[b])
    icpt, slope, _, w = oracle_fit(sizes, np.array(exact))
    tol = np.array(tol)
    # intercept and slope are linear in the per-subset values: W = pinv([1/n_i, 1]), row 0 the slope, row 1 the intercept
    icpt_tol, slope_tol = float(np.abs(w[1]) @ tol), float(np.abs(w[0]) @ tol)
    print(f"{tag}: fad_inf {got['fad_inf']!r} oracle {icpt!r} tol {icpt_tol:.3e} (sum|W1| {np.abs(w[1]).sum():.3f}); "
          f"slope {got['fad_inf_slope']!r} oracle {slope!r} tol {slope_tol:.3e}; r2 {got['fad_inf_r2']!r}")
    assert abs(got["fad_inf"] - icpt) <= icpt_tol
    assert abs(got["fad_inf_slope"] - slope) <= slope_tol
    _, _, r2_here, _ = oracle_fit(sizes, np.array(info["fads"]))         # r2 has no linear bound: recomputed from the returned values
    assert abs(got["fad_inf_r2"] - r2_here) <= 1e-12
    if dtype == np.float32 and d < 512:                                   # ordering sanity (holds for the oracle on these generators)
        full = am.frechet_distance(x, y)
        print(f"{tag}: fad_inf {got['fad_inf']:.6f} < fad {full:.6f} < fad at min_n {info['fads'][0]:.6f}")
        assert got["fad_inf"] < full < info["fads"][0]


# ------------------------------------------------------------------ 4. behaviour
def test_seeds_subsets_and_cached_statistics(am):
    from audio_metrics_amd.metrics import fad
    n, d = 6_000, 32
    x, y = data_of(am, spectrum_rows(1, n, d, 0.1)), data_of(am, spectrum_rows(2, n, d), store=False)
    before = am.frechet_distance(x, y)
    mean0, cov0 = x.mean.clone(), x.cov.clone()
    a = am.frechet_distance_inf(x, y, steps=6, min_n=500, seed=4)
    fads_a = list(fad.last_info["fads"])
    assert set(a) == {"fad_inf", "fad_inf_slope", "fad_inf_r2"} and all(isinstance(v, float) for v in a.values())
    assert am.frechet_distance_inf(x, y, steps=6, min_n=500, seed=4) == a and fad.last_info["fads"] == fads_a
    am.frechet_distance_inf(x, y, steps=6, min_n=500, seed=5)
    assert fad.last_info["fads"] != fads_a
    assert fad.last_info["sizes"] == [int(m) for m in np.linspace(500, n, 6).round().astype(int)]
    assert am.frechet_distance(x, y) == before                            # no state leaks into the cached statistics
    assert torch.equal(x.mean, mean0) and torch.equal(x.cov, cov0)
    sizes = [500, 1_600, 6_000]
    idx, offsets = fad.fad_inf_subset_indices(n, sizes, 4, torch.device(DEV))
    assert idx.dtype == torch.int64 and idx.is_cuda and offsets == [0, 500, 2_100, 8_100]
    for b, m in enumerate(sizes):
        part = idx[offsets[b]:offsets[b + 1]].cpu().numpy()
        assert len(np.unique(part)) == m and part.min() >= 0 and part.max() < n
    again, _ = fad.fad_inf_subset_indices(n, sizes, 4, torch.device(DEV))
    assert torch.equal(idx, again)


def test_small_subsets_warn_once(am):
    from audio_metrics_amd.metrics.fad import RANK_DEFICIENT_NOTE
    n, d = 1_000, 64
    x, y = data_of(am, spectrum_rows(3, n, d, 0.1)), data_of(am, spectrum_rows(4, n, d), store=False)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        am.frechet_distance_inf(x, y, steps=5, min_n=40, seed=0)
    notes = [w for w in caught if issubclass(w.category, RuntimeWarning)]
    assert len(notes) == 1 and str(notes[0].message) == RANK_DEFICIENT_NOTE.format(n=40, d=d)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        am.frechet_distance_inf(x, y, steps=5, min_n=65, seed=0)
    assert not [w for w in caught if issubclass(w.category, RuntimeWarning)]
    x64 = data_of(am, spectrum_rows(3, n, d, 0.1, np.float64))
    y64 = data_of(am, spectrum_rows(4, n, d, 0.0, np.float64), store=False)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        am.frechet_distance_inf(x64, y64, steps=5, min_n=40, seed=0)     # float64 rows carry no such dust
    assert not [w for w in caught if issubclass(w.category, RuntimeWarning)]


# ------------------------------------------------------------------ 5. through AudioMetrics
def test_through_audio_metrics(am):
    c = gi.E2E

    def make(metrics):
        return am.AudioMetrics(metrics=metrics, embedder=gi.NumpyEmbedder(c["dim"], c["sr"]), mix_function=gi.e2e_mix,
                               win_dur=c["win_dur"], device_indices=[0], fad_inf_steps=5, fad_inf_min_n=30, fad_inf_seed=2)
    ref = [x[:, 1] for x in gi.e2e_pairs(c["seed"], c["n_ref"], c["seconds"], c["sr"])]
    cand = [x[:, 1] for x in gi.e2e_pairs(c["seed"] + 1, c["n_cand"], c["seconds"], c["sr"], stem_gain=1.3)]
    results = []
    for metrics in (["fad", "fad_inf"], ["fad", "precision"], ["fad"]):
        m = make(metrics)
        m.add_reference(ref)
        results.append(m.evaluate(cand))
    both, stored, alone = results
    assert list(both) == ["fad", "fad_inf", "fad_inf_slope", "fad_inf_r2"]
    assert list(alone) == ["fad"] and list(stored) == ["fad"]
    # A configuration that keeps the stem rows recomputes the reference's statistics in one shot after add_reference (the
    # reference's own rule, audio_metrics.py:139), one that keeps none merges them batch by batch: "fad" is bit-equal to
    # that of any other row-keeping configuration, and equal to the statistics-only one up to the f32-centred rounding of the
    # two routes - both meet FAD_EXACT_REL against the definition (measured here: 3.5e-8 relative)
    assert both["fad"] == stored["fad"]
    print(f"fad with fad_inf {both['fad']!r}, statistics-only {alone['fad']!r}")
    assert abs(both["fad"] - alone["fad"]) <= FAD_EXACT_REL * abs(alone["fad"])
    assert all(np.isfinite(v) for v in both.values())
