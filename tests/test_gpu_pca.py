"""The n_pca path on the device against the float64 oracles of tests/pca_reference.py: the eigensolver
(hip_ops.eigh_descending / am_eigh_sym_f64), the projection (am_project_f64 / am_project_rows_f64) and the
projection.IncrementalPCA glue around them.

  1  shape sweep: single / ragged / odd block counts, both load paths, the second pass of the row update (D > 512) and of
     the Gram loop (D > 1024);  2  spectra: graded over 12 decades, clusters, a near-degenerate pair, rank 0 / 1 / D/3,
     diagonal input (exact);  3  determinism;  4  scale 2^-600 .. 2^600;  5  non-finite input and the sweep limit;
  6  projection: covering set of (N, D, p), contiguous and padded, exact on integers;  7  IncrementalPCA after every update
     in statistics mode and in rows mode (float32 / float64 rows), and its transform.

Limits (all relative to lam0 = the largest eigenvalue; the ones test_own_eigensolver_and_projection asserts):
  E1  max |evals - lambda| <= 1e-10 lam0, evals non-increasing     E2  max |V V^T - I| <= 1e-10
  E3  max |V A V^T - diag(evals)| <= 1e-9 lam0                       E4  cluster projectors to component_bound(1e-9 lam0)
Every test prints the figures it measured before it asserts."""
import time

import numpy as np
import pytest
import torch

import pca_reference as pr

pytestmark = pytest.mark.gpu

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


def solve(ops, a, **kw):
    evals, evecs = ops.eigh_descending(dev(a), **kw)
    assert evals.dtype == evecs.dtype == torch.float64 and tuple(evals.shape) == (a.shape[0],) and tuple(evecs.shape) == a.shape
    return evals.cpu().numpy(), evecs.cpu().numpy()


def assert_e123(name, a, evals, evecs):
    chk = pr.eigh_check(a, evals, evecs)
    print(f"{name}: D={a.shape[0]} lam0={chk['lam0']:.3e} E1={chk['e1']:.2e} E2={chk['e2']:.2e} E3={chk['e3']:.2e}")
    assert np.all(np.isfinite(evals)) and np.all(np.isfinite(evecs))
    assert chk["sorted"], "eigenvalues are not in descending order"
    assert chk["e1"] <= pr.E1_LIMIT, ("E1", chk["e1"])
    assert chk["e2"] <= pr.E2_LIMIT, ("E2", chk["e2"])
    assert chk["e3"] <= pr.E3_LIMIT, ("E3", chk["e3"])
    return chk


# ----------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("d", pr.SHAPE_SWEEP)
def test_shape_sweep(ops, d):
    a = pr.gram(d, 3 * d)
    evals, evecs = solve(ops, a)
    if d >= 513:                                         # the solve again, timed (the first call paid for the allocations)
        ad = dev(a)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.eigh_descending(ad)
        torch.cuda.synchronize()
        print(f"solve time D={d}: {(time.perf_counter() - t0) * 1e3:.1f} ms")
    assert_e123(f"gram({d}, {3 * d})", a, evals, evecs)


# ----------------------------------------------------------------- 2. spectra
@pytest.mark.parametrize("name,build", pr.spectra_cases(), ids=[n for n, _ in pr.spectra_cases()])
def test_spectra(ops, name, build):
    a = build()
    d = a.shape[0]
    evals, evecs = solve(ops, a)
    chk = assert_e123(name, a, evals, evecs)
    if name.startswith("clustered"):                     # E4: the vectors of a cluster are determined as a space only
        lam, vec = np.linalg.eigh(a)
        want = pr.cluster_projectors(lam[::-1], vec[:, ::-1].T, pr.CLUSTER_VALUES, chk["lam0"])
        got = pr.cluster_projectors(evals, evecs, pr.CLUSTER_VALUES, chk["lam0"])
        for k, (g, w) in enumerate(zip(got, want)):
            err = np.linalg.norm(g - w, 2)
            bound = pr.component_bound(np.array(pr.CLUSTER_VALUES) * chk["lam0"], k, pr.E3_LIMIT * chk["lam0"])
            print(f"{name}: cluster {pr.CLUSTER_VALUES[k]} rank {int(round(np.trace(g)))} projector error {err:.2e} (bound {bound:.2e})")
            assert int(round(np.trace(g))) == int(round(np.trace(w))) and err <= bound <= 1e-8 * (1 + 1e-12)
    if name.startswith("rank"):
        r = int(name[4:].split("-")[0])
        assert np.all(np.abs(evals[r:]) <= pr.E1_LIMIT * max(chk["lam0"], 1.0))
        if r == 0:
            assert not evals.any()
    if name.startswith("diagonal"):                      # no rotation: the result is the rank permutation and the sort, exactly
        diag = np.diagonal(a)
        assert np.array_equal(evals, np.sort(diag)[::-1])
        assert np.array_equal(np.sort(evecs, axis=1)[:, :-1], np.zeros((d, d - 1))) and np.array_equal(evecs.max(axis=1), np.ones(d))
        where = evecs.argmax(axis=1)
        assert sorted(where.tolist()) == list(range(d))                      # a permutation ...
        assert np.array_equal(diag[where], evals)                            # ... that takes a tied value's vectors in either order


# ----------------------------------------------------------------- 3. determinism
@pytest.mark.parametrize("d", [130, 528])
def test_two_calls_give_the_same_bits(ops, d):
    a = dev(pr.gram(d, 3 * d))
    e1, v1 = ops.eigh_descending(a)
    e2, v2 = ops.eigh_descending(a)
    assert torch.equal(e1, e2) and torch.equal(v1, v2)


# ----------------------------------------------------------------- 4. scale
_UNSCALED = {}


def unscaled(ops, name, build):
    if name not in _UNSCALED:
        a = build()
        _UNSCALED[name] = (a,) + solve(ops, a)
    return _UNSCALED[name]


@pytest.mark.parametrize("e", pr.SCALE_EXPONENTS)
@pytest.mark.parametrize("name,build", pr.scale_bases(), ids=[n for n, _ in pr.scale_bases()])
def test_scale(ops, name, build, e):
    """A matrix times 2^e: E1-E3 relative to the scaled lam0, and evals / 2^e against the e = 0 solve.  Before the solver scaled
    its input by the trace, |e| >= 300 returned the sorted diagonal and a permutation matrix with status AM_OK (the rotation
    test compares quantities of order lambda^4, which overflow or underflow), and e = -260 stopped nine digits early."""
    a0, evals0, evecs0 = unscaled(ops, name, build)
    assert_e123(f"{name} e=0", a0, evals0, evecs0)
    a = pr.scaled(a0, e)
    assert np.all(np.isfinite(a)) and np.array_equal(np.ldexp(a, -e), a0)      # the scaling is exact
    evals, evecs = solve(ops, a)
    chk = assert_e123(f"{name} e={e}", a, evals, evecs)
    back = np.ldexp(evals, -e)
    lam0 = np.ldexp(chk["lam0"], -e)
    drift = float(np.max(np.abs(back - evals0))) / lam0
    print(f"{name} e={e}: |evals / 2^e - evals(e=0)| = {drift:.2e} lam0, same bits: {np.array_equal(back, evals0) and np.array_equal(evecs, evecs0)}")
    assert drift <= pr.E1_LIMIT


# ----------------------------------------------------------------- 5. non-finite input, sweep limit
@pytest.mark.parametrize("kind", ["nan-off-diagonal", "inf-diagonal"])
def test_non_finite_matrix_raises_and_the_next_solve_is_good(am, ops, kind):
    good = pr.gram(40, 120)
    a = good.copy()
    if kind == "nan-off-diagonal":
        a[3, 17] = a[17, 3] = np.nan
    else:
        a[5, 5] = np.inf
    with pytest.raises(am._lib.HipLibraryError, match="status -5.*non-finite"):
        ops.eigh_descending(dev(a))
    evals, evecs = solve(ops, good)
    assert_e123("gram(40, 120) after " + kind, good, evals, evecs)


def test_sweep_limit_raises(am, ops):
    with pytest.raises(am._lib.HipLibraryError, match="status -5.*still not orthogonal"):
        ops.eigh_descending(dev(pr.gram(64, 192)), max_sweeps=1)


def test_partial_fit_on_a_nan_batch_raises_and_keeps_the_fit(am):
    batches, held = pr.case_batches(pr.PCA_CASES[1], 1)
    pca = am.IncrementalPCA(n_components=6)
    pca.partial_fit(dev(batches[0]))
    before = pca.__getstate__()
    bad = batches[2].copy()
    bad[4, :] = np.nan
    with pytest.raises(am._lib.HipLibraryError):
        pca.partial_fit(dev(bad))
    after = pca.__getstate__()
    assert before.keys() == after.keys()
    for k, v in before.items():
        assert torch.equal(v, after[k]) if torch.is_tensor(v) else v == after[k], k
    fresh = am.IncrementalPCA(n_components=6)
    with pytest.raises(am._lib.HipLibraryError):
        fresh.partial_fit(dev(bad))
    assert not any(hasattr(fresh, k) for k in ("components_", "n_components_", "n_samples_seen_", "mean_"))
    pca.partial_fit(dev(batches[2]))                       # and the fit goes on
    assert pca.n_samples_seen_ == len(batches[0]) + len(batches[2])


# ----------------------------------------------------------------- 6. projection
def padded(x, dtype):
    """The same rows as a column slice of a wider tensor whose padding is NaN (a row stride the float32 entry point accepts
    as it is: a multiple of four elements)."""
    n, d = x.shape
    ld = (d + 3) // 4 * 4 + 4 if dtype == torch.float32 else d + 3
    buf = torch.full((n, ld), float("nan"), dtype=dtype, device=DEV)
    buf[:, :d] = dev(x).to(dtype)
    view = buf[:, :d]
    assert view.stride(0) == ld and view.data_ptr() == buf.data_ptr()
    return view


@pytest.mark.parametrize("n,d,p", pr.PROJECT_SHAPES)
def test_projection(ops, n, d, p):
    for exact in (True, False):
        x, mean, comp = pr.project_inputs(n, d, p, exact)
        want, scale = pr.project_reference(x, mean, comp)
        for dtype in (torch.float32, torch.float64):
            for layout in ("contiguous", "padded"):
                xd = dev(x).to(dtype) if layout == "contiguous" else padded(x, dtype)
                got = ops.project(xd, dev(mean), dev(comp))
                assert got.dtype == torch.float64 and tuple(got.shape) == (n, p)
                got = got.cpu().numpy()
                if exact:
                    assert np.array_equal(got, want), (dtype, layout, "integers: every sum is exact")
                else:
                    ratio = float(np.max(np.abs(got - want) / scale))
                    print(f"project N={n} D={d} p={p} {dtype} {layout}: max |err| / sum|x - mean||c| = {ratio:.2e}")
                    assert ratio <= 1e-12, (dtype, layout, ratio)


# ----------------------------------------------------------------- 7. IncrementalPCA
def _np(t):
    return t.detach().cpu().numpy()


def assert_fit(tag, pca, st, delta, stats_err, mean_abs):
    """The fitted attributes against the oracle's state `st`.  delta: norm of the Gram matrix's error allowed (eigensolver limit
    E3, plus the statistics' own limit in rows mode); stats_err = delta minus the eigensolver's share (0 in statistics
    mode): what Weyl's inequality lets the device statistics move an eigenvalue, on top of 1e-10 lam0."""
    lam0 = st["lams"][0]
    n, d = st["n_samples_seen_"], st["mean_"].shape[0]
    p = st["n_components_"]
    assert pca.n_samples_seen_ == n and pca.n_components_ == p
    comps = _np(pca.components_)
    assert comps.shape == (p, d)
    val_tol = 1e-10 * lam0 + stats_err
    bounds, null = pr.component_bounds(st, delta)
    s2_err = float(np.max(np.abs(_np(pca.singular_values_) ** 2 - st["singular_values_"] ** 2)))
    norm_err = float(np.max(np.abs(np.linalg.norm(comps, axis=1) - 1.0)))
    worst = 0.0
    for i in range(p):
        if null[i]:            # a vector of the numerical null space: the space is determined, the direction in it is not
            err = float(np.linalg.norm(pr.outside_null_space(st, delta, comps[i])))
        else:                  # unit vectors with the oracle's sign: the distance is taken without aligning them
            err = float(np.linalg.norm(comps[i] - st["components_"][i]))
        worst = max(worst, err / bounds[i])
        assert err <= bounds[i], (tag, "component", i, err, bounds[i])
    print(f"{tag}: n={n} p={p} lam0={lam0:.3e} s^2 err {s2_err / lam0:.2e} lam0 (limit {val_tol / lam0:.1e}), component err / bound "
          f"{worst:.2e} (largest bound {bounds.max():.1e}), | |c| - 1 | {norm_err:.1e}")
    assert s2_err <= val_tol and norm_err <= 1e-10
    top = np.abs(comps).argmax(axis=1)
    assert np.all(comps[np.arange(p), top] > 0)                                    # svd_flip's rule holds on the device's own rows
    mean_tol = 1e-10 * np.max(np.abs(st["mean_"])) + mean_abs
    var_tol = 1e-10 * np.max(st["var_"]) + stats_err / n
    assert np.max(np.abs(_np(pca.mean_) - st["mean_"])) <= mean_tol
    assert np.max(np.abs(_np(pca.var_) - st["var_"])) <= var_tol
    assert np.max(np.abs(_np(pca.explained_variance_) - st["explained_variance_"])) <= val_tol / (n - 1)
    total = float(np.sum(st["var_"] * n))
    ratio_tol = (val_tol + (1e-10 * total + d * stats_err)) / total                # numerator, and the trace below it (ratios <= 1)
    assert np.max(np.abs(_np(pca.explained_variance_ratio_) - st["explained_variance_ratio_"])) <= ratio_tol
    assert abs(pca.noise_variance_ - st["noise_variance_"]) <= val_tol / (n - 1)


def assert_transform(tag, pca, held, dtype):
    """transform of a held-out batch against numpy on the DEVICE's fitted attributes: the projection judged on its own."""
    x = dev(held).to(dtype)
    got = _np(pca.transform(x))
    want, scale = pr.project_reference(_np(x).astype(np.float64), _np(pca.mean_), _np(pca.components_))
    ratio = float(np.max(np.abs(got - want) / scale))
    print(f"{tag}: transform max |err| / sum|x - mean||c| = {ratio:.2e}")
    assert got.shape == (pr.HELD_OUT_ROWS, pca.n_components_) and ratio <= 1e-12


CASE_IDS = [pr.case_id(c) for c in pr.PCA_CASES]


@pytest.mark.parametrize("index", range(len(pr.PCA_CASES)), ids=CASE_IDS)
def test_incremental_pca_statistics_mode(am, index):
    """partial_fit(batch_stats=...) with numpy float64 statistics: the eigensolver plus the torch glue."""
    case = pr.PCA_CASES[index]
    batches, held = pr.case_batches(case, index)
    pca = am.IncrementalPCA(n_components=case[1])
    for step, (x, st) in enumerate(zip(batches, pr.trajectory(index))):
        pca.partial_fit(dev(x), batch_stats=pr.batch_stats(x))
        tag = f"{pr.case_id(case)} statistics update {step}"
        assert_fit(tag, pca, st, pr.delta_statistics(st), 0.0, 0.0)
        assert_transform(tag, pca, held, torch.float32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("index", range(len(pr.PCA_CASES)), ids=CASE_IDS)
def test_incremental_pca_rows_mode(am, index, dtype):
    """partial_fit(rows): the statistics come from ops.stats in the dtype of the rows.  The (40, 40) fit is compared only
    where its bound meets the cap (pca_reference.rows_mode_cases; test_pca_cpu asserts that nothing else is left out) - it
    is still FITTED and its values, which need no gap, are still checked."""
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    case = pr.PCA_CASES[index]
    batches, held = pr.case_batches(case, index)
    pca = am.IncrementalPCA(n_components=case[1])
    compare_vectors = index in pr.rows_mode_cases(np_dtype)
    for step, (x, st) in enumerate(zip(batches, pr.trajectory(index))):
        pca.partial_fit(dev(x).to(dtype))
        tag = f"{pr.case_id(case)} rows {np.dtype(np_dtype).name} update {step}"
        delta = pr.delta_rows(st, np_dtype)
        stats_err = delta - pr.delta_statistics(st)
        mean_abs = 1e-12 if dtype == torch.float32 else 1e-13 * max(1.0, float(np.max(np.abs(st["mean_"]))))
        if compare_vectors:
            assert_fit(tag, pca, st, delta, stats_err, mean_abs)
        else:
            s2_err = float(np.max(np.abs(_np(pca.singular_values_) ** 2 - st["singular_values_"] ** 2)))
            print(f"{tag}: vectors not compared (bound above the cap); s^2 err {s2_err / st['lams'][0]:.2e} lam0")
            assert pca.n_samples_seen_ == st["n_samples_seen_"] and s2_err <= 1e-10 * st["lams"][0] + stats_err
        assert_transform(tag, pca, held, dtype)
