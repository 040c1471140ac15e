"""The Frechet and f32-statistics references (tests/frechet_reference.py) validated on the CPU, and the two bounds the device
tests use tied to what the documented arithmetic delivers: a transcription of the Newton-Schulz solve against the closed
form, and a transcription of the f32 covariance against float64.  The device files import SOLVER_REL and STATS_F32_ELEM
from here; each is asserted below to leave a stated factor over the model's own error on the very inputs the device gets."""
import numpy as np

import frechet_reference as fr

# |tr_sqrt - closed form| / (tr Cx + tr Cy) of ns_model over D_EDGES x COND: measured maximum 3.44e-13 (D = 5, cond 1e8).
# The factor 8 below covers another summation order of the same error order (four wave partials per tile, matrix-core
# order against BLAS).  A value above 1e-10 would mean the inputs are ill posed, not that the cap should move.
SOLVER_REL = 5e-12
SOLVER_FACTOR = 8

# max |model - f64|_ij / sqrt(C_ii C_jj) of stats_f32_model over STATS_N x STATS_D and the foreign-mean scatters:
# measured maximum 8.94e-07 = 15.0 units of 2^-24 (N = 256, D = 131).  The factor 4 covers the matrix core's summation
# order inside a chain and chain boundaries that fall at row-slab edges instead of every 256 rows.
STATS_F32_ELEM = 4e-6
STATS_FACTOR = 4

FAD_EXACT_REL, FAD_TERMS_REL = 1e-6, 1e-7       # the project's end-to-end bar (test_gpu_parity.py), used for rank-deficient pairs


def test_closed_form_psd_oracle_and_model_agree_at_every_edge():
    worst, worst_psd, where = 0.0, 0.0, None
    for d in fr.D_EDGES:
        for cond in fr.COND:
            mu_x, cx, mu_y, cy, tr = fr.commuting_pair(d, cond, 0)
            assert np.array_equal(cx, cx.T) and np.array_equal(cy, cy.T)
            scale = fr.solver_scale(cx, cy)
            fd_p, tr_p = fr.fd_psd(mu_x, cx, mu_y, cy)
            tr_m, iters, stop, resid = fr.ns_model(cx, cy)
            assert stop in (1, 2), (d, cond, stop)
            e_m, e_p = abs(tr_m - tr) / scale, abs(tr_p - tr) / scale
            assert abs(fd_p - fr.fd_closed(mu_x, cx, mu_y, cy, tr)) <= 2 * SOLVER_REL * scale
            if e_m > worst:
                worst, where = e_m, (d, cond)
            worst_psd = max(worst_psd, e_p)
    print(f"ns_model against the closed form: max |tr_sqrt - closed| / (tr Cx + tr Cy) = {worst:.3e} at D, cond = {where}; "
          f"fd_psd: {worst_psd:.3e}; SOLVER_REL = {SOLVER_REL:.1e}")
    assert SOLVER_REL <= 1e-10
    assert SOLVER_FACTOR * worst <= SOLVER_REL
    assert SOLVER_FACTOR * worst_psd <= SOLVER_REL


def test_model_meets_the_bounds_of_the_general_and_rank_deficient_pairs():
    for d in fr.GENERAL_D:
        p = fr.sample_pair(d, 4 * d, 4 * d, 1)
        assert np.linalg.matrix_rank(p[1]) == d and np.linalg.matrix_rank(p[3]) == d
        _, tr_p = fr.fd_psd(*p)
        tr_m, _, stop, _ = fr.ns_model(p[1], p[3])
        assert stop == 1 and SOLVER_FACTOR * abs(tr_m - tr_p) <= SOLVER_REL * fr.solver_scale(p[1], p[3])
    for d, rows_x, rows_y in fr.RANK_DEFICIENT:
        p = fr.sample_pair(d, rows_x, rows_y, 0)
        assert np.linalg.matrix_rank(p[1]) == min(rows_x - 1, d) < d
        _, tr_p = fr.fd_psd(*p)
        tr_m, _, stop, _ = fr.ns_model(p[1], p[3])
        rel = abs(tr_m - tr_p) / fr.solver_scale(p[1], p[3])
        print(f"rank-deficient D={d} rows {rows_x}/{rows_y}: model - oracle = {rel:.3e} of the terms, stop {stop}")
        assert stop == 2 and rel <= 1e-8               # a tenth of FAD_TERMS_REL: the device bound is not the model's slack


def test_model_codes_of_degenerate_products():
    d = 5
    mu_x, cx, mu_y, cy, _ = fr.commuting_pair(d, 1e4, 0)
    assert fr.ns_model(np.zeros((d, d)), cy) == (0.0, 0, 3, 0.0)
    for bad in (np.nan, np.inf):
        c = cx.copy()
        c[1, 2] = bad
        assert fr.ns_model(c, cy)[2] == 4
    mu_x, mu_y, cy = fr.dyadic_pair(33, 0)
    assert np.array_equal(cy, cy.T)
    fd = fr.fd_of(mu_x, np.zeros_like(cy), mu_y, cy, 0.0)
    assert fd == float(((mu_x - mu_y)[::-1] ** 2).sum() + np.diagonal(cy)[::-1].sum())       # exact in any order


def test_model_meets_the_bound_of_its_kind_on_the_batch_sets_and_equal_pairs():
    for d in fr.BATCH_D:
        for shared in (False, True):
            for kind, mu_x, cx, mu_y, cy, fd, tr in fr.batch_sets(d, shared):
                tr_m, _, stop, _ = fr.ns_model(cx, cy)
                rel = abs(tr_m - tr) / fr.solver_scale(cx, cy)
                print(f"batch D={d} shared={shared} {kind}: model - oracle = {rel:.3e} of the terms, stop {stop}")
                if kind == "rank":
                    assert stop == 2 and rel <= 1e-8
                elif kind == "zero":
                    assert stop == 3 and tr_m == 0.0
                else:
                    assert stop in (1, 2) and SOLVER_FACTOR * rel <= SOLVER_REL
    for d in fr.DEGENERATE_D:
        _, cx, _, _, _ = fr.commuting_pair(d, fr.EQUAL_PAIR_COND, 0)
        tr_m, _, stop, _ = fr.ns_model(cx, cx)
        assert stop in (1, 2) and SOLVER_FACTOR * abs(tr_m - np.trace(cx)) <= SOLVER_REL * 2 * np.trace(cx)


def test_budget_pair_leaves_a_margin_of_three_iterations():
    """Budgets that end with stop 0 must do so by at least three iterations, so a one-step difference in the device's
    decision cannot change the expected outcome; the converged budgets all return the same record."""
    d, cond, seed = fr.BUDGET_PAIR
    _, cx, _, cy, tr = fr.commuting_pair(d, cond, seed)
    full = fr.ns_model(cx, cy)
    print(f"budget pair D={d} cond={cond:g}: the model converges at {full[1]} evaluations (stop {full[2]})")
    assert full[2] == 1 and full[1] > 16 + 3           # converges, and only in the second block of 16
    traces = []
    for budget in fr.BUDGETS:
        tr_m, iters, stop, _ = fr.ns_model(cx, cy, max_iter=budget)
        traces.append(tr_m)
        if budget + 1 < full[1]:
            assert (stop, iters) == (0, budget + 1) and full[1] >= budget + 3
        else:
            assert (tr_m, iters, stop) == full[:3]
    assert [b for b in fr.BUDGETS if b + 1 < full[1]] == [1, 2, 15, 16, 17]
    assert all(b >= a for a, b in zip(traces, traces[1:]))
    assert traces[0] < 0.9 * tr                         # a spent budget is visibly short of the answer


def test_f32_statistics_model_against_float64():
    worst, where = 0.0, None
    for n in fr.STATS_N:
        for d in fr.STATS_D:
            x = fr.stats_input(n, d)
            e = fr.elem_rel(fr.stats_f32_model(x), fr.cov_f64(x))
            if e > worst:
                worst, where = e, ("cov", n, d)
    for n in fr.SCATTER_N:
        for d in fr.SCATTER_D:
            big = fr.stats_input(2 * n, d, seed=1)
            x = big[:n]
            for kind, mean in (("own", x.astype(np.float64).mean(0)), ("foreign", big.astype(np.float64).mean(0))):
                e = fr.elem_rel(fr.stats_f32_model(x, mean), fr.scatter_f64(x, mean))
                if e > worst:
                    worst, where = e, (kind, n, d)
    print(f"stats_f32_model against f64: max |model - f64|_ij / sqrt(C_ii C_jj) = {worst:.3e} = {worst * 2 ** 24:.1f} x 2^-24 "
          f"at {where}; STATS_F32_ELEM = {STATS_F32_ELEM:.1e}")
    assert STATS_FACTOR * worst <= STATS_F32_ELEM


def test_statistics_oracles_agree_with_numpy():
    x = fr.stats_input(257, 5)
    np.testing.assert_allclose(fr.cov_f64(x), np.cov(x.astype(np.float64), rowvar=False), rtol=1e-13, atol=0)
    assert not fr.cov_f64(x[:1]).any() and not fr.stats_f32_model(x[:1]).any()
    # the merge formula reproduces the covariance of the concatenated rows
    a, b = x[:100].astype(np.float64), x[100:].astype(np.float64)
    mean, cov, bound = fr.merge_f64(100, a.mean(0), fr.cov_f64(a), 157, b.mean(0), fr.cov_f64(b))
    np.testing.assert_allclose(mean, x.astype(np.float64).mean(0), rtol=0, atol=1e-14)
    assert np.abs(cov - fr.cov_f64(x)).max() <= 1e-13 * np.abs(cov).max()
    assert np.all(bound >= np.abs(cov) * (1 - 1e-15))
    # elem_rel sees one wrong element that a Frobenius norm at 1e-5 would not
    want = fr.cov_f64(fr.stats_input(513, 129))
    got = want.copy()
    got[128, 3] += 1e-4 * np.sqrt(want[128, 128] * want[3, 3])
    assert fr.elem_rel(got, want) > STATS_F32_ELEM
    assert np.linalg.norm(got - want) <= 1e-5 * np.linalg.norm(want)
