"""The PCA oracle (tests/pca_reference.py) checked on the CPU: against scikit-learn's IncrementalPCA, against the limits
the device test asserts (np.linalg.eigh meets them with a factor of 1000 to spare on every input: the inputs are well
posed at those limits), and the conditions on the case table that make every component comparable."""
import numpy as np
import pytest

import pca_reference as pr


def _all_eigh_inputs():
    for d in pr.SHAPE_SWEEP:
        yield f"gram-{d}", lambda d=d: pr.gram(d, 3 * d)
    yield from pr.spectra_cases()
    for name, build in pr.scale_bases():
        yield name, build
        for e in pr.SCALE_EXPONENTS:
            yield f"{name}-2^{e}", lambda build=build, e=e: pr.scaled(build(), e)


@pytest.mark.parametrize("name,build", list(_all_eigh_inputs()), ids=[n for n, _ in _all_eigh_inputs()])
def test_numpy_eigh_meets_the_device_limits_with_a_factor_1000(name, build):
    a = build()
    assert np.array_equal(a, a.T) and np.all(np.isfinite(a))
    lam, vec = np.linalg.eigh(a)
    chk = pr.eigh_check(a, lam[::-1], vec[:, ::-1].T)
    print(name, {k: chk[k] for k in ("lam0", "e1", "e2", "e3")})
    assert chk["sorted"]
    assert chk["e1"] <= pr.E1_LIMIT / 1000 and chk["e2"] <= pr.E2_LIMIT / 1000 and chk["e3"] <= pr.E3_LIMIT / 1000


def test_eigh_check_sees_a_wrong_answer():
    """A permutation matrix with the diagonal as eigenvalues - what the solver returned for a matrix outside its scale
    range - fails E1 and E3; swapped rows fail the order; a scaled vector fails E2."""
    a = pr.gram(17, 51)
    d = a.shape[0]
    order = np.argsort(-np.diagonal(a))
    chk = pr.eigh_check(a, np.diagonal(a)[order], np.eye(d)[order])
    assert chk["e2"] == 0 and chk["e1"] > 1e-3 and chk["e3"] > 1e-3
    lam, vec = np.linalg.eigh(a)
    lam, vt = lam[::-1].copy(), vec[:, ::-1].T.copy()
    assert not pr.eigh_check(a, lam[::-1], vt[::-1])["sorted"]
    vt[3] *= 1.0 + 1e-6
    assert pr.eigh_check(a, lam, vt)["e2"] > 1e-7


def test_matrix_families_are_seed_stable_and_as_described():
    for name, build in _all_eigh_inputs():
        assert build().tobytes() == build().tobytes(), name
    lam = np.linalg.eigvalsh(pr.clustered(48))
    assert sorted(np.round(lam, 12).tolist()) == sorted(pr.clustered_spectrum(48).tolist())
    assert np.linalg.matrix_rank(pr.rank_r(130, 43)) == 43 and not pr.rank_r(17, 0).any()
    lam = np.linalg.eigvalsh(pr.near_pair(33))[::-1]
    assert 0 <= (lam[0] - lam[1]) / lam[0] < 1e-12
    assert np.ptp(np.log10(np.linalg.eigvalsh(pr.graded(33, 12)))) > 11.9
    ties = np.diagonal(pr.diagonal(40, "ties"))
    assert len(set(ties)) < 40 and len(set(np.diagonal(pr.diagonal(40, "distinct")))) == 40
    assert np.any(np.diff(np.diagonal(pr.diagonal(40, "distinct"))) > 0)              # shuffled, not sorted


def test_projection_shapes_cover_every_axis_value():
    ns, ds, ps = (set(s[i] for s in pr.PROJECT_SHAPES) for i in range(3))
    assert ns == {1, 63, 64, 65, 1000} and ds == {1, 3, 4, 5, 70, 513} and ps == {1, 15, 16, 17, 33}
    assert (1, 1, 1) in pr.PROJECT_SHAPES and (1000, 513, 33) in pr.PROJECT_SHAPES and len(set(pr.PROJECT_SHAPES)) == len(pr.PROJECT_SHAPES)
    x, mean, comp = pr.project_inputs(65, 513, 15, exact=True)
    want, scale = pr.project_reference(x, mean, comp)
    assert np.array_equal(want, np.rint(want)) and np.max(scale) < 2 ** 30                # integers: every sum is exact


@pytest.mark.parametrize("index", range(len(pr.PCA_CASES)), ids=[pr.case_id(c) for c in pr.PCA_CASES])
def test_case_table_conditions(index):
    """A bound is a condition, not an escape: over the whole table the largest component bound stays below the caps and the
    sign of every kept component is decided with a margin.  Only a component of the numerical null space (the twelfth of
    the fit whose only batch has 12 rows: the centred batch has rank 11) has no direction of its own; it is bounded as a
    member of that space instead (pca_reference.component_bounds) and takes no part in the sign comparison."""
    case = pr.PCA_CASES[index]
    null_seen = 0
    for step, st in enumerate(pr.trajectory(index)):
        bounds, null = pr.component_bounds(st, pr.delta_statistics(st))
        margin = pr.sign_margins(st, null)
        print(pr.case_id(case), "update", step, "statistics bound", bounds.max(), "sign margin", margin.min(),
              "null components", int(null.sum()))
        assert bounds.max() <= pr.STAT_CAP
        assert margin.min() > pr.SIGN_MARGIN
        null_seen += int(null.sum())
        for dtype in (np.float32, np.float64):
            if index in pr.rows_mode_cases(dtype):
                rb, rnull = pr.component_bounds(st, pr.delta_rows(st, dtype))
                print("   rows", np.dtype(dtype).name, "bound", rb.max())
                assert rb.max() <= pr.ROWS_CAP
                assert pr.sign_margins(st, rnull).min() > pr.SIGN_MARGIN
    assert null_seen == (1 if "fewer rows" in case[3] else 0)
    for dtype in (np.float32, np.float64):
        left_out = set(range(len(pr.PCA_CASES))) - set(pr.rows_mode_cases(dtype))
        assert all(pr.PCA_CASES[i][:2] == (40, 40) for i in left_out)


@pytest.mark.parametrize("index", range(len(pr.PCA_CASES)), ids=[pr.case_id(c) for c in pr.PCA_CASES])
def test_gram_route_against_scikit_learn(index):
    skd = pytest.importorskip("sklearn.decomposition")
    case = pr.PCA_CASES[index]
    batches, held = pr.case_batches(case, index)
    ref = skd.IncrementalPCA(n_components=case[1])
    for step, (x, st) in enumerate(zip(batches, pr.trajectory(index))):
        ref.partial_fit(x.astype(np.float64))
        lam0 = st["lams"][0]
        delta = 1e-12 * lam0
        bounds, null = pr.component_bounds(st, delta)
        assert ref.n_samples_seen_ == st["n_samples_seen_"] and ref.n_components_ == st["n_components_"]
        np.testing.assert_allclose(ref.singular_values_ ** 2, st["singular_values_"] ** 2, rtol=0, atol=1e-12 * lam0)
        for i in range(st["n_components_"]):
            got, want = ref.components_[i], st["components_"][i]
            if null[i]:                          # determined as a space only: scikit-learn's vector lies in the oracle's null space
                assert np.linalg.norm(pr.outside_null_space(st, delta, got)) <= bounds[i]
            else:
                assert np.linalg.norm(got - want) <= bounds[i], (step, i, np.linalg.norm(got - want), bounds[i])
        np.testing.assert_allclose(ref.mean_, st["mean_"], rtol=0, atol=1e-13 * np.max(np.abs(st["mean_"])))
        np.testing.assert_allclose(ref.var_, st["var_"], rtol=0, atol=1e-12 * np.max(st["var_"]))
        np.testing.assert_allclose(ref.explained_variance_, st["explained_variance_"], rtol=0, atol=1e-12 * lam0)
        np.testing.assert_allclose(ref.explained_variance_ratio_, st["explained_variance_ratio_"], rtol=0, atol=1e-12)
        if np.isfinite(ref.noise_variance_):
            assert abs(ref.noise_variance_ - st["noise_variance_"]) <= 1e-12 * lam0
    fit = pr.GramPCA(case[1])
    for x in batches:
        fit.partial_fit(x)
    assert fit.transform(held).shape == (pr.HELD_OUT_ROWS, st["n_components_"])


def test_component_bound_is_davis_kahan():
    lams = np.array([4.0, 3.0, 1.0])
    assert pr.component_bound(lams, 1, 1e-3) == 4e-3 / 1.0 and pr.component_bound(lams, 2, 1e-3) == 4e-3 / 2.0
    assert pr.component_bound(np.array([1.0, 1.0]), 0, 1e-9) == np.inf
    rng = np.random.default_rng(3)                                       # and it holds on a perturbed matrix
    a = pr.graded(12, 1)
    e = rng.standard_normal((12, 12)) * 1e-7
    e = 0.5 * (e + e.T)
    delta = np.linalg.norm(e, 2)
    l0, v0 = np.linalg.eigh(a)
    _, v1 = np.linalg.eigh(a + e)
    for i in range(12):
        u, w = v0[:, i], v1[:, i] * np.sign(v1[:, i] @ v0[:, i])
        assert np.linalg.norm(u - w) <= pr.component_bound(l0, i, delta)
