"""The feature likelihood divergence, the part that needs no GPU: the float64 oracle's gradient against finite differences,
the host Adam step against the oracle's, fld_from_logliks, validation before any device call in both layers, the new names
in header / signature table / package, the entry points' error paths and workspace queries, and the behaviour of the
construction on seeded clusters with copied training rows (the oracle's 100-step fit at the shipped defaults)."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import fld_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -4
FAKE = ctypes.c_void_p(0x10000)                       # 16-byte aligned, never dereferenced: the calls stop at validation
NAMES = ("am_fld_loglik_workspace_bytes", "am_fld_loglik_f32", "am_fld_grad_workspace_bytes", "am_fld_grad_f32")


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    return audio_metrics_amd


@pytest.fixture(scope="module")
def lib(am):
    return am._lib.load()


def host_set(am, rows):
    s = am.AudioMetricsData(True)
    s._embeddings = rows
    return s


# ---------------------------------------------------------------------------------------------------- the oracle itself
def test_the_oracle_gradient_matches_central_differences():
    rng = np.random.default_rng(1)
    x, g = rng.standard_normal((30, 5)).astype(np.float32) * 0.4, rng.standard_normal((12, 5)).astype(np.float32) * 0.4
    theta = rng.uniform(-2.0, 1.0, 12)
    a, b, grad = fr.grad_sums(x, g, theta)
    assert np.isclose(a.sum(), 30.0, rtol=1e-12)                            # the responsibilities of a row sum to 1
    assert np.allclose(grad, fr.gradient(theta, a, b, 5, 30), rtol=1e-13, atol=0)
    eps = 1e-5
    for j in range(12):
        e = np.zeros(12)
        e[j] = eps
        fd = (fr.loss(x, g, theta + e) - fr.loss(x, g, theta - e)) / (2 * eps)
        assert abs(fd - grad[j]) <= 1e-8, (j, fd, grad[j])
    # a row and a centre with non-finite elements drop out: the gradient of the rest, and 0 for the centre
    x2, g2 = np.vstack([x, np.full((1, 5), np.nan, np.float32)]), np.vstack([g, np.full((1, 5), np.inf, np.float32)])
    a2, b2, grad2 = fr.grad_sums(x2, g2, np.append(theta, 0.0))
    ll = fr.loglik(x2, g2, np.append(theta, 0.0))
    assert ll[-1] == -np.inf and np.isfinite(ll[:-1]).all()
    assert a2[-1] == b2[-1] == grad2[-1] == 0.0 and np.allclose(a2[:-1], a, rtol=1e-12) and np.allclose(b2[:-1], b, rtol=1e-12)
    assert np.allclose(ll[:-1], fr.loglik(x, g, theta) - math.log(13 / 12), rtol=1e-12)       # M counts the dead centre


def test_loglik_of_one_centre_is_the_gaussian_density():
    x, g = np.array([[0.5, -1.0, 2.0]], np.float32), np.array([[0.0, 0.0, 1.0]], np.float32)
    for theta in (-1.5, 0.0, 2.0):
        var = math.exp(theta)
        want = -0.5 * 2.25 / var - 1.5 * math.log(2 * math.pi * var)
        assert math.isclose(fr.loglik(x, g, np.array([theta]))[0], want, rel_tol=1e-13)


def test_host_adam_step_is_the_oracles(am):
    rng = np.random.default_rng(2)
    theta, grad, m, v = rng.uniform(-9, 2, 50), rng.standard_normal(50), rng.standard_normal(50) * 0.1, rng.uniform(0, 0.2, 50)
    for step in (1, 2, 57, 1000):
        got = am.fld_adam_step(theta, grad, m, v, step, 0.5, -10.0)
        want = fr.adam_step(theta, grad, m, v, step, 0.5, -10.0)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
    # the first step from zero moments moves every entry by lr, whatever the gradient's size; the clamp is hit exactly
    t1, m1, v1 = am.fld_adam_step(np.zeros(3), np.array([1e-3, -5.0, 0.0]), np.zeros(3), np.zeros(3), 1, 0.5, -10.0)
    assert np.allclose(t1, [-0.5, 0.5, 0.0], atol=1e-4) and t1[2] == 0.0
    lo, _, _ = am.fld_adam_step(np.array([-9.9, 29.9]), np.array([1.0, -1.0]), np.zeros(2), np.zeros(2), 1, 0.5, -10.0)
    assert lo[0] == -10.0 and lo[1] == 30.0
    with pytest.raises(ValueError, match="step"):
        am.fld_adam_step(theta, grad, m, v, 0, 0.5, -10.0)
    from audio_metrics_amd.metrics import fld
    a, b = rng.uniform(0, 3, 50), rng.uniform(0, 3, 50)
    assert np.array_equal(fld.fld_gradient(theta, a, b, 40, 77.0), fr.gradient(theta, a, b, 40, 77.0))
    assert not fld.fld_gradient(theta, a, b, 40, 0.0).any()


def test_from_logliks_arithmetic(am):
    tr, te = np.array([-10.0, -30.0, -np.inf, -20.0]), np.array([-50.0, np.nan, -70.0])
    out = am.fld_from_logliks(tr, te, 10, baseline_nll=1.5)
    assert out["fld_nll_train"] == 2.0 and out["fld_nll_test"] == 6.0 and out["fld_generalization_gap"] == 4.0
    assert out["fld"] == 450.0 and out["fld_baseline_nll"] == 1.5
    assert am.fld_from_logliks(tr, te, 10)["fld"] == 600.0
    assert math.isnan(am.fld_from_logliks([-np.inf], te, 10)["fld_nll_train"])
    for bad in (0, -2):
        with pytest.raises(ValueError, match="D="):
            am.fld_from_logliks(tr, te, bad)
    with pytest.raises(ValueError, match="baseline_nll"):
        am.fld_from_logliks(tr, te, 10, baseline_nll=math.nan)


# ---------------------------------------------------------------------------------------------------- behaviour
@pytest.mark.parametrize("d,n,m,t", [(16, 384, 320, 256), (40, 300, 257, 200)], ids=["D16", "D40"])
def test_copied_training_rows_stand_out(d, n, m, t):
    copies = 40
    train, test, gen = fr.clustered(5, d, n, m, t, copies)
    theta, history = fr.fit(train, gen, steps=100, lr=0.5, theta_min=-10.0)
    others = theta[copies:]
    print(f"D={d}: copies at {theta[:copies].min():.3f} .. {theta[:copies].max():.3f}, others median {np.median(others):.3f}")
    assert (theta[:copies] == -10.0).all()                                  # the copies end at the clamp
    assert np.median(others) > -8.0 and (others > -10.0).mean() > 0.9
    nll_train, nll_test = fr.loss(train, gen, theta) / d, fr.loss(test, gen, theta) / d
    print(f"D={d}: nll_train {nll_train:.4f} nll_test {nll_test:.4f}, loss {history[0] / d:.4f} -> {history[-1] / d:.4f}")
    assert nll_train < nll_test
    assert history[-1] < history[0] and history.shape == (101,) and history[-1] == fr.loss(train, gen, theta)
    score = fr.overfit_scores(gen, train, test, theta)
    print(f"D={d}: overfit score of the copies >= {score[:copies].min():.4g}, of the others <= {score[copies:].max():.4g}")
    assert score[:copies].min() > score[copies:].max()


def test_the_oracle_leaves_few_authenticity_ties():
    rng = np.random.default_rng(9)
    train, gen = rng.standard_normal((130, 40)).astype(np.float32), rng.standard_normal((150, 40)).astype(np.float32)
    gen[:10] = train[:10] + (1e-3 * rng.standard_normal((10, 40))).astype(np.float32)
    authentic, nearest, margin = fr.authenticity(gen, train)
    assert (margin <= 1e-5).mean() <= 0.02
    assert not authentic[:10].any() and (nearest[:10] == np.arange(10)).all()      # a copy is nearer than any other training row
    assert 0.0 < authentic.mean() < 1.0


# ---------------------------------------------------------------------------------------------------- validation
def test_validation_happens_before_any_device_call(am, monkeypatch):
    from audio_metrics_amd import hip_ops

    def forbidden(*a, **k):
        raise AssertionError("device call before validation")
    for name in ("as_matrix", "_call", "_workspace"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    x, g = torch.zeros((10, 8)), torch.zeros((12, 8))
    theta, lse = torch.zeros(12, dtype=torch.float64), torch.zeros(10, dtype=torch.float64)
    nf = torch.ones(1, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match=r"fld_loglik takes float32 rows \(the float64 matrix-core form is not implemented\)"):
        hip_ops.fld_loglik(x.double(), g, theta)
    with pytest.raises(NotImplementedError, match="fld_grad_step takes float32 rows"):
        hip_ops.fld_grad_step(g, x.double(), theta, lse, nf, theta, theta, 1, 0.5, -10.0)
    with pytest.raises(ValueError, match="feature widths"):
        hip_ops.fld_loglik(x, torch.zeros((12, 12)), theta)
    with pytest.raises(ValueError, match="2-D"):
        hip_ops.fld_loglik(torch.zeros(8), g, theta)
    with pytest.raises(ValueError, match="rows on both sides"):
        hip_ops.fld_loglik(x, torch.zeros((0, 8)), torch.zeros(0, dtype=torch.float64))
    for bad in (theta[:11], theta.float(), torch.zeros((12, 1), dtype=torch.float64), [0.0] * 12):
        with pytest.raises(ValueError, match="one log-variance per row of g"):
            hip_ops.fld_loglik(x, g, bad)
        with pytest.raises(ValueError, match="theta must be a float64 tensor of 12 elements"):
            hip_ops.fld_grad_step(g, x, bad, lse, nf, theta, theta, 1, 0.5, -10.0)
    for bad in (torch.zeros(2, dtype=torch.float64), torch.zeros(3)):
        with pytest.raises(ValueError, match="stats"):
            hip_ops.fld_loglik(x, g, theta, stats=bad)
    with pytest.raises(ValueError, match="lse must be a float64 tensor of 10 elements"):
        hip_ops.fld_grad_step(g, x, theta, lse[:9], nf, theta, theta, 1, 0.5, -10.0)
    with pytest.raises(ValueError, match="m must be"):
        hip_ops.fld_grad_step(g, x, theta, lse, nf, theta[:3], theta, 1, 0.5, -10.0)
    with pytest.raises(ValueError, match="n_finite"):
        hip_ops.fld_grad_step(g, x, theta, lse, 10.0, theta, theta, 1, 0.5, -10.0)
    with pytest.raises(ValueError, match="step"):
        hip_ops.fld_grad_step(g, x, theta, lse, nf, theta, theta, 0, 0.5, -10.0)
    for bad in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="lr"):
            hip_ops.fld_grad_step(g, x, theta, lse, nf, theta, theta, 1, bad, -10.0)
    for bad in (-90.0, 30.5, math.inf, math.nan):
        with pytest.raises(ValueError, match="theta_min"):
            hip_ops.fld_grad_step(g, x, theta, lse, nf, theta, theta, 1, 0.5, bad)
    with pytest.raises(AssertionError, match="device call before validation"):
        hip_ops.fld_loglik(x, g, theta)
    with pytest.raises(AssertionError, match="device call before validation"):
        hip_ops.fld_grad_step(g, x, theta, lse, nf, theta, theta, 1, 0.5, -10.0)

    # the front end: with the operations it uses forbidden too
    for name in ("fld_loglik", "fld_grad_step", "knn_search"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    gen, train, test = (host_set(am, torch.randn((k, 8))) for k in (12, 10, 9))
    both = (lambda **kw: am.feature_likelihood_fit(gen, train, **kw), lambda **kw: am.feature_likelihood_divergence(gen, train, test, **kw))
    for call in both:
        for bad in (0, -5):
            with pytest.raises(ValueError, match="steps"):
                call(steps=bad)
        for bad in (math.nan, math.inf, -0.1):
            with pytest.raises(ValueError, match="lr"):
                call(lr=bad)
        for bad in (math.nan, -math.inf, -90.0, 31.0):
            with pytest.raises(ValueError, match="min_log_variance"):
                call(min_log_variance=bad)
        with pytest.raises(ValueError, match="normalize"):
            call(normalize="test")
        with pytest.raises(AssertionError, match="device call before validation"):
            call(normalize=None)
    with pytest.raises(ValueError, match="baseline_nll"):
        am.feature_likelihood_divergence(gen, train, test, baseline_nll=math.nan)
    wide, none64 = host_set(am, torch.randn((9, 12))), host_set(am, torch.randn((9, 8)).double())
    for args in ((wide, train, test), (gen, wide, test), (gen, train, wide)):
        with pytest.raises(ValueError, match="feature widths"):
            am.feature_likelihood_divergence(*args, normalize=None)
    for args in ((none64, train, test), (gen, none64, test), (gen, train, none64)):
        with pytest.raises(NotImplementedError, match="float64 rows"):
            am.feature_likelihood_divergence(*args, normalize=None)
    empty = am.AudioMetricsData(False)
    for args in ((empty, train, test), (gen, empty, test), (gen, train, empty)):
        with pytest.raises(ValueError, match="keeps none"):
            am.feature_likelihood_divergence(*args)
    with pytest.raises(ValueError, match="keeps none"):
        am.feature_likelihood_fit(gen, empty)
    with pytest.raises(ValueError, match="keeps none"):
        am.authenticity_score(empty, train)
    with pytest.raises(ValueError, match="feature widths"):
        am.authenticity_score(wide, train)
    with pytest.raises(NotImplementedError, match="float64 rows"):
        am.authenticity_score(gen, none64)
    with pytest.raises(AssertionError, match="device call before validation"):
        am.authenticity_score(gen, train)


# ---------------------------------------------------------------------------------------------------- names
def test_header_signature_table_and_package_agree(am, lib):
    with open(os.path.join(ROOT, "include", "audio_metrics_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in am._lib.SIGNATURES and hasattr(lib, name), name
    assert len(am._lib.SIGNATURES["am_fld_loglik_f32"][1]) == 13 and len(am._lib.SIGNATURES["am_fld_grad_f32"][1]) == 21
    from audio_metrics_amd.metrics import fld
    assert am.feature_likelihood_divergence is fld.feature_likelihood_divergence and am.feature_likelihood_fit is fld.feature_likelihood_fit
    assert am.fld_adam_step is fld.fld_adam_step and am.fld_from_logliks is fld.fld_from_logliks
    assert am.authenticity_score is fld.authenticity_score and am.metrics.fld is fld
    assert callable(am.hip_ops.fld_loglik) and callable(am.hip_ops.fld_grad_step)
    # function calls on three sets, not a metric name of AudioMetrics
    assert "fld" not in inspect.getsource(am.audio_metrics).lower()


# ---------------------------------------------------------------------------------------------------- entry points
def test_entry_point_error_paths_and_workspace(lib):
    n, m, d, ld = 130, 300, 40, 40
    nb = lib.am_fld_loglik_workspace_bytes(n, m, d)
    nbg = lib.am_fld_grad_workspace_bytes(m, n, d)
    assert nb > 0 and nbg > 0

    def loglik(x=FAKE, n=n, ldx=ld, g=FAKE, m=m, ldg=ld, d=d, theta=FAKE, out=FAKE, stats=FAKE, ws=FAKE, nb=nb):
        return lib.am_fld_loglik_f32(x, n, ldx, g, m, ldg, d, theta, out, stats, ws, nb, None)

    def grad(g=FAKE, m=m, ldg=ld, x=FAKE, n=n, ldx=ld, d=d, theta=FAKE, lse=FAKE, nf=FAKE, am_=FAKE, av=FAKE, step=1, lr=0.5, tmin=-10.0,
             tout=FAKE, a=None, b=None, ws=FAKE, nb=nbg):
        return lib.am_fld_grad_f32(g, m, ldg, x, n, ldx, d, theta, lse, nf, am_, av, step, lr, tmin, tout, a, b, ws, nb, None)
    for null in ("x", "g", "theta", "out", "stats"):
        assert loglik(**{null: None}) == BAD_ARG, null
    for null in ("x", "g", "theta", "lse", "nf", "am_", "av", "tout"):
        assert grad(**{null: None}) == BAD_ARG, null
    for call in (loglik, grad):
        assert call(x=ctypes.c_void_p(0x10004)) == BAD_ARG and call(g=ctypes.c_void_p(0x10008)) == BAD_ARG      # alignment
        assert call(ldx=42) == BAD_ARG and call(ldg=36) == BAD_ARG                                              # ld % 4, ld >= D
        assert call(n=0) == BAD_SHAPE and call(m=0) == BAD_SHAPE and call(d=0, ldx=0, ldg=0) == BAD_SHAPE
        assert call(ws=None) == WORKSPACE
    assert loglik(nb=nb - 1) == WORKSPACE and "am_fld_loglik_workspace_bytes" in lib.am_last_error().decode()
    assert grad(nb=nbg - 1) == WORKSPACE and "am_fld_grad_workspace_bytes" in lib.am_last_error().decode()
    assert grad(step=0) == BAD_ARG and "step" in lib.am_last_error().decode()
    for bad in (-1.0, math.inf, math.nan):
        assert grad(lr=bad) == BAD_ARG, bad
    for bad in (-90.0, 30.5, math.inf, -math.inf, math.nan):               # 0.5 exp(-theta_min) has to be a normal float32 number
        assert grad(tmin=bad) == BAD_ARG, bad
        assert "theta_min" in lib.am_last_error().decode()
    for bad in ((0, 5, 8), (5, 0, 8), (5, 5, 0)):
        assert lib.am_fld_loglik_workspace_bytes(*bad) == 0 and lib.am_fld_grad_workspace_bytes(*bad) == 0, bad
    # loglik: norms of both sets, two floats per centre, (4 + 8) bytes per row and chunk, 16 bytes per block of 256 rows;
    # grad: norms of both sets, two floats per centre and per row, 16 bytes per centre and chunk - plus alignment
    for n_, m_ in ((130, 300), (1000, 100_000), (100_000, 1000)):
        need = 4 * n_ + 12 * m_ + 12 * n_ * lib.am_knn_search_chunks(n_, m_, 64, 1) + 16 * ((n_ + 255) // 256)
        got = lib.am_fld_loglik_workspace_bytes(n_, m_, 64)
        assert need <= got <= need + 8 * 256, (n_, m_, need, got)
        need = 12 * m_ + 12 * n_ + 16 * m_ * lib.am_knn_search_chunks(m_, n_, 64, 1)
        got = lib.am_fld_grad_workspace_bytes(m_, n_, 64)
        assert need <= got <= need + 9 * 256, (n_, m_, need, got)
