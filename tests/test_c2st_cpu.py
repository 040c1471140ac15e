"""The host side of the classifier two-sample test, without a GPU: the fold dealing, the lockstep L-BFGS against a Newton
solve, the summary formulas against hand-worked cases, the checks that fire before any device call, and the calibration of
the test under H0 - hip_ops.logit_pass replaced by the float64 oracle of tests/c2st_reference.py.

Calibration, 300 seeded draws from ONE law, d = 8, 5 folds, l2 = 1e-3 (the figures printed by the tests, also in the README):
  independent rows, 400 against 500           one-fold test rejects 6.0 % at the one-sided 5 % level, mean accuracy 0.4984
  48 against 40 songs of 16 windows, by song  rejects 6.3 %, mean accuracy 0.4990
  the same rows, folds dealt by row           rejects 91.3 %, mean accuracy 0.6063"""
import types
import warnings

import numpy as np
import pytest
import torch

import c2st_reference as cr

D = 8
DRAWS = 300
L2 = 1e-3


@pytest.fixture(scope="module")
def c2():
    from audio_metrics_amd.metrics import c2st
    return c2st


def stub(rows, store=True, n=None):
    """what the entry point reads of an AudioMetricsData"""
    rows = np.asarray(rows)
    r64 = rows.astype(np.float64)
    return types.SimpleNamespace(embeddings=torch.as_tensor(rows) if store else None, n=len(rows) if n is None else n,
                                 mean=torch.as_tensor(r64.mean(axis=0)), cov=torch.as_tensor(np.cov(r64.T).reshape(rows.shape[1], -1)),
                                 store_embeddings=store)


def host_merge(n1, mean1, cov1, n2, mean2, cov2, inplace=False):
    n = n1 + n2
    delta = mean2 - mean1
    mean = mean1 + delta * (n2 / n)
    cov = ((n1 - 1) * cov1 + (n2 - 1) * cov2 + torch.outer(delta, delta) * (n1 * n2 / n)) / (n - 1)
    return mean, cov


@pytest.fixture
def host_ops(c2, monkeypatch):
    """hip_ops.logit_pass / stats_merge computed on the host; the calls are recorded"""
    import audio_metrics_amd.data as data
    calls = []
    knobs = {"pass": cr.host_pass}

    def logit_pass(rows, fold, label, coef, want_z=True):
        calls.append("logit_pass")
        return knobs["pass"](rows, fold, label, coef, want_z)

    def stats_merge(*args, **kwargs):
        calls.append("stats_merge")
        return host_merge(*args, **kwargs)

    monkeypatch.setattr(c2.ops, "logit_pass", logit_pass)
    monkeypatch.setattr(c2.ops, "stats_merge", stats_merge)
    monkeypatch.setattr(c2.ops, "as_rows", lambda e, name="embeddings": e)
    monkeypatch.setattr(data, "default_device", lambda: torch.device("cpu"))
    return types.SimpleNamespace(calls=calls, knobs=knobs)


# ------------------------------------------------------------------ folds
def test_folds_are_stratified_keep_units_whole_and_follow_the_seed(c2):
    import audio_metrics_amd as am
    assert am.c2st_folds is c2.c2st_folds
    got = c2.c2st_folds(23, 5, np.random.default_rng(4))
    assert got.dtype == np.int32 and got.shape == (23,)
    assert sorted(np.bincount(got, minlength=5).tolist()) == [4, 4, 5, 5, 5]                # 23 rows in 5 folds
    assert np.array_equal(got, cr.folds(23, 5, np.random.default_rng(4)))                   # the definition, by a loop
    assert np.array_equal(got, c2.c2st_folds(23, 5, np.random.default_rng(4)))              # the seed reproduces
    assert not np.array_equal(got, c2.c2st_folds(23, 5, np.random.default_rng(5)))
    labels = np.random.default_rng(0).permutation(np.repeat(np.array([7, -3, 40, 41, 1000, 2, 9]), [3, 1, 5, 2, 4, 4, 2]))
    got = c2.c2st_folds(labels, 3, np.random.default_rng(11))
    assert np.array_equal(got, cr.folds(labels, 3, np.random.default_rng(11)))
    assert np.array_equal(got, c2.c2st_folds(torch.as_tensor(labels), 3, np.random.default_rng(11)))
    for value in np.unique(labels):
        assert len(set(got[labels == value].tolist())) == 1                                 # a unit is never split
    units_per_fold = [len(set(labels[got == k].tolist())) for k in range(3)]
    assert sorted(units_per_fold) == [2, 2, 3]                                              # 7 units in 3 folds
    # one generator, the candidate set first: the reference's folds depend on the candidate's unit count
    rng = np.random.default_rng(2)
    first, second = c2.c2st_folds(10, 2, rng), c2.c2st_folds(10, 2, rng)
    assert not np.array_equal(first, second)
    rng = np.random.default_rng(2)
    assert np.array_equal(first, cr.folds(10, 2, rng)) and np.array_equal(second, cr.folds(10, 2, rng))
    with pytest.raises(ValueError, match="4 unit"):
        c2.c2st_folds(4, 5, np.random.default_rng(0))
    with pytest.raises(ValueError, match="2 unit"):
        c2.c2st_folds(np.array([1, 1, 2, 2, 2]), 3, np.random.default_rng(0))
    for bad in (1, 17):
        with pytest.raises(ValueError, match="folds"):
            c2.c2st_folds(100, bad, np.random.default_rng(0))
    with pytest.raises(ValueError, match="integers"):
        c2.c2st_folds(np.array([0.5, 1.5]), 2, np.random.default_rng(0))


# ------------------------------------------------------------------ the summary, by hand
def test_summary_hand_worked_cases(c2):
    # candidate logits: right, right, tie, wrong; reference: right (negative), wrong, right.  All rows in fold 0.
    zc, zr = np.array([2.0, 0.5, 0.0, -1.0]), np.array([-1.0, 0.25, -3.0])
    fc, fr = np.zeros(4, dtype=np.int32), np.zeros(3, dtype=np.int32)
    got = c2.c2st_summary(zc, zr, fc, fr)
    acc = 0.5 * (2.5 / 4 + 2.0 / 3)
    assert got["c2st_accuracy"] == acc == got["c2st_accuracy_holdout"] and got["c2st_holdout_rows"] == (4, 3)
    v = (3 * 0.25 + 0.0) / 16 + 3 * 0.25 / 9                                                # the tie adds (1/2 - 1/2)^2 = 0
    assert got["c2st_z"] == pytest.approx((acc - 0.5) / np.sqrt(0.25 * v), rel=1e-15)
    assert got["c2st_p_value"] == pytest.approx(cr.phi(-got["c2st_z"]), rel=1e-15)
    # pairs (candidate > reference): 2.0 beats 3, 0.5 beats 3, 0.0 beats 2, -1.0 beats 1 and ties 1
    assert got["c2st_auc"] == (3 + 3 + 2 + 1 + 0.5) / 12
    hc, hr = np.array([1, 1, 0.5, 0]), np.array([1.0, 0, 1])
    se = np.sqrt(0.25 * (hc.var(ddof=1) / 4 + hr.var(ddof=1) / 3))
    assert got["c2st_std_error"] == pytest.approx(se, rel=1e-14)
    assert got["c2st_log_loss"] == pytest.approx(0.5 * (np.mean([cr.softplus(-t) for t in zc]) + np.mean([cr.softplus(t) for t in zr])), rel=1e-14)
    want = cr.summary(zc, zr, fc, fr)
    for key in ("c2st_accuracy", "c2st_accuracy_holdout", "c2st_z", "c2st_p_value", "c2st_auc", "c2st_holdout_rows"):
        assert got[key] == want[key], key

    # rows as units: v_side = 1 / (4 n0) exactly, so z = (acc0 - 1/2) / sqrt((1 / n0c + 1 / n0r) / 16)
    rng = np.random.default_rng(1)
    zc, zr = rng.standard_normal(37) + 0.3, rng.standard_normal(29) - 0.3
    fc, fr = (np.arange(37) % 3).astype(np.int32), (np.arange(29) % 3).astype(np.int32)
    got = c2.c2st_summary(zc, zr, fc, fr)
    n0c, n0r = 13, 10
    assert got["c2st_holdout_rows"] == (n0c, n0r)
    acc0 = 0.5 * ((zc[fc == 0] > 0).mean() + (zr[fr == 0] < 0).mean())
    assert got["c2st_accuracy_holdout"] == acc0
    assert got["c2st_z"] == (acc0 - 0.5) / np.sqrt(0.25 * (1.0 / (4 * n0c) + 1.0 / (4 * n0r)))

    # perfect separation: a finite z, the largest the fold allows
    got = c2.c2st_summary(np.full(8, 5.0), np.full(6, -5.0), np.arange(8) % 2, np.arange(6) % 2)
    assert got["c2st_accuracy"] == 1.0 and got["c2st_auc"] == 1.0 and got["c2st_std_error"] == 0.0
    assert got["c2st_z"] == 0.5 / np.sqrt(0.25 * (1.0 / 16 + 1.0 / 12)) and 0.0 < got["c2st_p_value"] < 0.01

    # songs as units: two windows of a song that are both right count as one unit of weight 1, not two of 1/2
    zc, zr = np.array([1.0, 1.0, -1.0, 1.0]), np.array([-1.0, -1.0, 1.0, 1.0])
    fold = np.zeros(4, dtype=np.int32)
    groups = np.array([5, 5, 9, 9])
    got = c2.c2st_summary(zc, zr, fold, fold, groups, groups)
    assert got["c2st_accuracy_holdout"] == 0.5 * (0.75 + 0.5)
    assert got["c2st_z"] == (0.625 - 0.5) / np.sqrt(0.25 * ((1.0 + 0.0) / 16 + (1.0 + 1.0) / 16))
    assert got == pytest.approx(cr.summary(zc, zr, fold, fold, groups, groups), rel=1e-14)
    # every unit's hits and misses cancel: z = 0, p = 1/2
    got = c2.c2st_summary(np.array([1.0, -1.0]), np.array([1.0, -1.0]), fold[:2], fold[:2], np.array([1, 1]), np.array([2, 2]))
    assert got["c2st_z"] == 0.0 and got["c2st_p_value"] == 0.5
    # rows without a finite logit or without a fold take part in nothing
    a = c2.c2st_summary(np.array([1.0, np.nan, -2.0, 3.0]), np.array([-1.0, 2.0, 9.0]), np.array([0, 0, 1, 1]), np.array([0, 1, -1]))
    b = c2.c2st_summary(np.array([1.0, -2.0, 3.0]), np.array([-1.0, 2.0]), np.array([0, 1, 1]), np.array([0, 1]))
    assert a == b
    with pytest.raises(ValueError, match="one logit and one fold per row"):
        c2.c2st_summary(np.zeros(3), np.zeros(3), np.zeros(2), np.zeros(3))


# ------------------------------------------------------------------ the optimiser
def test_lbfgs_minimises_quadratics_in_lockstep(c2):
    rng = np.random.default_rng(3)
    q = np.linalg.qr(rng.standard_normal((12, 12)))[0]
    base = q @ np.diag(np.logspace(0, 3, 12)) @ q.T                    # the shared initial Hessian, condition 1000
    mats, rhs = [], []
    for k in range(3):
        low = rng.standard_normal((12, 3))
        mats.append(base + (k + 1.0) * low @ low.T + 0.5 * k * np.eye(12))
        rhs.append(rng.standard_normal(12))
    calls = []

    def precondition(v):
        return np.linalg.solve(base, v)

    def evaluate(theta):
        calls.append(theta.copy())
        return ([0.5 * t @ m @ t - b @ t for t, m, b in zip(theta, mats, rhs)], [m @ t - b for t, m, b in zip(theta, mats, rhs)])

    fit = c2.logistic_lbfgs(evaluate, 3, 12, precondition, 1e-9, 500)
    assert fit["converged"].all() and (fit["gradient_norm"] <= 1e-9).all() and fit["passes"] == len(calls)
    for k in range(3):
        assert np.linalg.norm(fit["theta"][k] - np.linalg.solve(mats[k], rhs[k])) <= 1e-9      # |x - x*| <= |grad| / lambda_min
    first_done = min(i for i, t in enumerate(calls) if np.array_equal(t[0], fit["theta"][0]))
    assert all(np.array_equal(t[0], fit["theta"][0]) for t in calls[first_done:])               # a converged model keeps its point
    capped = c2.logistic_lbfgs(evaluate, 3, 12, precondition, 1e-9, 3)
    assert capped["passes"] == 3 and not capped["converged"].all()


def sample(seed=10, shift=0.5):
    rng = np.random.default_rng(seed)
    law = cr.law(rng, 6)
    x, gx = cr.draw_songs(rng, 14, 6, law, 0.5, shift)
    y, gy = cr.draw_songs(rng, 12, 7, law, 0.5)
    return x, gx * 3 + 1, y, gy[::-1].copy()


def test_the_fit_reaches_tol_and_lands_within_the_strong_convexity_bound(c2, host_ops):
    x, gx, y, gy = sample()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        got = c2.classifier_two_sample_test(stub(x), stub(y), groups=gx, ref_groups=torch.as_tensor(gy), folds=4, l2=L2, seed=3, return_rows=True)
    assert got["c2st_converged"].all() and (got["c2st_gradient_norm"] <= 1e-8).all() and got["c2st_rows_nonfinite"] == 0
    assert host_ops.calls.count("logit_pass") == 2 * (got["c2st_passes"] + 1) and host_ops.calls.count("stats_merge") == 1
    rng = np.random.default_rng(3)
    fx, fy = cr.folds(gx, 4, rng), cr.folds(gy, 4, rng)
    assert np.array_equal(got["c2st_candidate_fold"], fx) and np.array_equal(got["c2st_reference_fold"], fy)
    mu, sigma = cr.pooled(x, y)
    thetas, norms, zx, zy = cr.fit(x, y, fx, fy, 4, L2, mu, sigma)
    assert (norms <= 1e-13).all()
    w = got["c2st_weights"] * sigma
    b = got["c2st_intercepts"] + got["c2st_weights"] @ mu
    dist = np.linalg.norm(np.concatenate([w, b[:, None]], axis=1) - thetas, axis=1)
    bound = (got["c2st_gradient_norm"] + norms) / L2
    print("distance to the Newton optimum", dist, "bound", bound, "passes", got["c2st_passes"])
    assert (dist <= bound + 1e-12).all()
    for z_got, z_want, rows in ((got["c2st_candidate_logit"], zx, x), (got["c2st_reference_logit"], zy, y)):
        reach = np.sqrt((((rows - mu) / sigma) ** 2).sum(axis=1) + 1.0)
        assert (np.abs(z_got - z_want) <= bound.max() * reach + 1e-12).all()
    want = cr.summary(zx, zy, fx, fy, gx, gy)
    margin = min(np.abs(zx).min(), np.abs(zy).min())
    assert margin > 1e-3                                         # no logit near 0: the hits agree and the figures are equal
    for key in ("c2st_accuracy", "c2st_accuracy_holdout", "c2st_z", "c2st_p_value", "c2st_holdout_rows"):
        assert got[key] == want[key], key
    assert got["c2st_auc"] == pytest.approx(want["c2st_auc"], abs=1e-3)        # the order of two logits 1e-5 apart may differ
    assert got["c2st_std_error"] == pytest.approx(want["c2st_std_error"], rel=1e-9)
    assert got["c2st_log_loss"] == pytest.approx(want["c2st_log_loss"], rel=1e-6)
    assert list(got)[:8] == ["c2st_accuracy", "c2st_std_error", "c2st_log_loss", "c2st_auc", "c2st_accuracy_holdout", "c2st_holdout_rows",
                             "c2st_z", "c2st_p_value"]
    # the same rows and labels in another order: the same units, the same folds per unit, the same figures
    perm = np.random.default_rng(8).permutation(len(x))
    again = c2.classifier_two_sample_test(stub(x[perm]), stub(y), groups=gx[perm], ref_groups=gy, folds=4, l2=L2, seed=3, return_rows=True)
    assert np.array_equal(again["c2st_candidate_fold"], fx[perm]) and again["c2st_accuracy"] == got["c2st_accuracy"]
    assert np.allclose(again["c2st_candidate_logit"], got["c2st_candidate_logit"][perm], rtol=0, atol=1e-4)


def test_warnings_for_non_finite_rows_and_for_the_pass_limit(c2, host_ops):
    x, gx, y, gy = sample()
    bad = x.copy()
    bad[5, 2], bad[40, 0] = np.nan, np.inf
    with np.errstate(invalid="ignore"):
        cand = stub(bad)                                          # its stored statistics are NaN, as a real set's would be
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = c2.classifier_two_sample_test(cand, stub(y), groups=gx, ref_groups=gy, folds=4, l2=L2, seed=3, return_rows=True)
    assert len(caught) == 1 and caught[0].category is RuntimeWarning and "2 row(s)" in str(caught[0].message)
    assert got["c2st_rows_nonfinite"] == 2 and got["c2st_converged"].all()
    assert np.flatnonzero(np.isnan(got["c2st_candidate_logit"])).tolist() == [5, 40] and not np.isnan(got["c2st_reference_logit"]).any()
    assert got["c2st_candidate_fold"][5] == -1 and got["c2st_candidate_fold"][40] == -1
    clean = np.delete(np.arange(len(x)), [5, 40])
    rng = np.random.default_rng(3)
    fx, fy = cr.folds(gx, 4, rng), cr.folds(gy, 4, rng)
    both = np.concatenate([x[clean], y])
    _, _, zx, zy = cr.fit(bad, y, fx, fy, 4, L2, both.mean(axis=0), both.std(axis=0, ddof=1))
    assert np.allclose(got["c2st_candidate_logit"][clean], zx[clean], rtol=0, atol=1e-4)        # the statistics leave the two rows out
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = c2.classifier_two_sample_test(stub(x), stub(y), folds=4, l2=L2, max_passes=3)
    assert len(caught) == 1 and caught[0].category is RuntimeWarning and "have not reached" in str(caught[0].message)
    assert got["c2st_passes"] == 3 and not got["c2st_converged"].any() and np.isfinite(got["c2st_accuracy"])


def test_every_raise_fires_before_a_device_call(c2, host_ops):
    x, gx, y, gy = sample()
    run = c2.classifier_two_sample_test
    with pytest.raises(NotImplementedError, match="mixed pair"):
        run(stub(x.astype(np.float32)), stub(y))
    with pytest.raises(NotImplementedError, match="mixed pair"):
        run(stub(x), stub(y.astype(np.float32)))
    cases = [
        (lambda: run(stub(x, store=False), stub(y)), "keeps none"),
        (lambda: run(stub(x), stub(y, n=len(y) + 1)), "statistics describe"),
        (lambda: run(stub(x[:, :5]), stub(y)), "widths differ"),
        (lambda: run(stub(x), stub(y), folds=1), "folds"),
        (lambda: run(stub(x), stub(y), folds=17), "folds"),
        (lambda: run(stub(x), stub(y), folds=2.5), "folds"),
        (lambda: run(stub(x), stub(y), l2=0.0), "l2"),
        (lambda: run(stub(x), stub(y), tol=0.0), "tol"),
        (lambda: run(stub(x), stub(y), max_passes=0), "max_passes"),
        (lambda: run(stub(x), stub(y), groups=gx[:-1]), "labels for"),
        (lambda: run(stub(x), stub(y), groups=gx, ref_groups=gy, folds=13), "12 unit"),
        (lambda: run(stub(x), stub(y), groups=np.zeros(len(x), dtype=np.int64)), "1 unit"),
    ]
    for call, words in cases:
        with pytest.raises(ValueError, match=words):
            call()
    assert host_ops.calls == []


def test_names_are_exported_and_the_probe_is_no_metric_name():
    import audio_metrics_amd as am
    for name in ("classifier_two_sample_test", "c2st_folds", "c2st_summary", "logistic_lbfgs"):
        assert callable(getattr(am, name)), name
    assert callable(am.hip_ops.logit_pass) and am.metrics.c2st.classifier_two_sample_test is am.classifier_two_sample_test
    for name in ("am_logit_pass_workspace_bytes", "am_logit_pass_f32", "am_logit_pass_f64"):
        assert name in am._lib.SIGNATURES, name
    assert len(am._lib.SIGNATURES["am_logit_pass_f32"][1]) == 14 == len(am._lib.SIGNATURES["am_logit_pass_f64"][1])
    import inspect
    assert "c2st" not in inspect.getsource(am.audio_metrics)


# ------------------------------------------------------------------ calibration under H0
def calibrate(c2, make, by_song):
    rejections, accs = 0, []
    for draw in range(DRAWS):
        rng = np.random.default_rng(5000 + draw)
        x, gx, y, gy = make(rng)
        got = c2.classifier_two_sample_test(stub(x), stub(y), groups=gx if by_song else None, ref_groups=gy if by_song else None,
                                            folds=5, l2=L2, seed=draw)
        rejections += got["c2st_p_value"] < 0.05
        accs.append(got["c2st_accuracy"])
    return rejections / DRAWS, float(np.mean(accs))


def iid_case(rng):
    law = cr.law(rng, D)
    return cr.draw(rng, 400, law), None, cr.draw(rng, 500, law), None


def song_case(rng):
    law = cr.law(rng, D)
    x, gx = cr.draw_songs(rng, 48, 16, law, 0.3)
    y, gy = cr.draw_songs(rng, 40, 16, law, 0.3)
    return x, gx, y, gy


def test_calibration_independent_rows(c2, host_ops):
    host_ops.knobs["pass"] = cr.fast_pass
    rate, acc = calibrate(c2, iid_case, False)
    print(f"CALIBRATION iid 400 x 500, d = {D}: rejection rate {rate:.4f}, mean cross-fitted accuracy {acc:.4f}")
    assert 0.012 <= rate <= 0.088                                  # 5 % +- 3 binomial standard deviations for 300 draws
    assert abs(acc - 0.5) <= 0.02


def test_calibration_songs_as_units(c2, host_ops):
    host_ops.knobs["pass"] = cr.fast_pass
    rate, acc = calibrate(c2, song_case, True)
    print(f"CALIBRATION songs 48 x 16 against 40 x 16, folds by song: rejection rate {rate:.4f}, mean cross-fitted accuracy {acc:.4f}")
    assert 0.012 <= rate <= 0.088
    assert abs(acc - 0.5) <= 0.02


def test_folds_dealt_by_row_reject_equal_song_data(c2, host_ops):
    host_ops.knobs["pass"] = cr.fast_pass
    rate, acc = calibrate(c2, song_case, False)
    print(f"CALIBRATION songs 48 x 16 against 40 x 16, folds by ROW: rejection rate {rate:.4f}, mean cross-fitted accuracy {acc:.4f}")
    assert rate > 0.5
