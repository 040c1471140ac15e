"""The feature likelihood sweeps on the device (hip_ops.fld_loglik, hip_ops.fld_grad_step, csrc/fld.hip) and the front end
(metrics/fld.py) against the float64 oracle of tests/fld_reference.py.

  1  loglik, every shape: per row within delta_i = 2^-24 ((D + 16) (max |x|^2 + max |g|^2) h_max + 4 (|lse_i| + max |c|));
     the largest observed error / delta per shape goes to profiles/fld/accuracy.txt
  2  gradient sums, every shape, with Delta = max_i delta_i:  |A - A*| <= 2 Delta A*,
     |h (B - B*)| <= 2 Delta h B* + 2^-24 (D + 16) (max |x|^2 + max |g|^2) h A*, each plus 1e-300; sum_j A_j = finite rows
  3  one device Adam step from a seeded (theta, m, v, step) against fld_adam_step on the device's own A and B, every element
     of theta, m and v to 1e-14 relative; the clamp exactly
  4  padded views;  5  non-finite rows and centres;  6  determinism;  7  every term but the largest underflows;
  8  end to end: the front end's numbers against the oracle at the device's theta, the optimiser against the oracle's own
     fit, the copies on top of the overfit scores and at the clamp, the authenticity score.

The shapes (rows, centres, D) are the soft-min's edge set: one row, 128 +- 1 rows, a partial third column tile, D with and
without the inner-dimension tail, a set against itself, and 32 column chunks.  Inputs are clustered rows after the default
normalisation; theta is uniform in [-10, 1] with 20 centres at -10 on near-copies of evaluated rows."""
import math
import warnings

import numpy as np
import pytest
import torch

import fld_reference as fr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 1, 1), (127, 129, 33), (130, 300, 40), (130, 300, 64), (257, 130, 96), (130, 130, 64), (130, 4000, 40)]
SELF = (130, 130, 64)                                # the centres are the evaluated rows
IDS = ["x".join(map(str, s)) for s in SHAPES]
THETA_MIN = -10.0
WORST = {}                                           # case -> largest error / bound
CASES = {}                                           # shape -> inputs and oracle results, computed once


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    audio_metrics_amd._lib.load()
    return audio_metrics_amd


@pytest.fixture(scope="module")
def ops(am):
    return am.hip_ops


@pytest.fixture(scope="module", autouse=True)
def accuracy_record():
    yield
    if WORST:
        fr.record_accuracy("loglik and gradient sums: largest |device - oracle| / bound per shape (bound: 1)",
                           [f"{case}: {ratio:.4f}" for case, ratio in WORST.items()])


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def padded(a, extra, fill):
    """The same rows as a view of a wider buffer whose padding must never be read as data."""
    buf = torch.full((a.shape[0], a.shape[1] + extra), fill, dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = dev(a)
    view = buf[:, :a.shape[1]]
    assert view.stride(0) == a.shape[1] + extra
    return view


def case(shape):
    """x [rows, D], g [centres, D], theta and the oracle's loglik, sums and bound for one shape."""
    if shape in CASES:
        return CASES[shape]
    n, m, d = shape
    x, _, g = fr.clustered(21 + d, d, max(n, 2), m, 2, 0)
    x = x[:n]
    rng = np.random.default_rng(31)
    copies = min(20, m, n)
    if shape == SELF:
        g = x
    else:
        g = g.copy()
        g[:copies] = x[:copies] + (1e-3 * rng.standard_normal((copies, d)) / math.sqrt(d)).astype(np.float32)
    theta = rng.uniform(THETA_MIN, 1.0, m)
    theta[:copies] = THETA_MIN
    c = {"x": x, "g": g, "theta": theta, "loglik": fr.loglik(x, g, theta)}
    c["a"], c["b"], _ = fr.grad_sums(x, g, theta)
    x64, g64 = x.astype(np.float64), g.astype(np.float64)
    c["norms"] = float((x64 * x64).sum(1).max()) + float((g64 * g64).sum(1).max())
    c["hmax"] = float(0.5 * np.exp(-theta).max())
    c["delta"] = fr.delta(d, c["norms"], 0.0, c["hmax"], c["loglik"] + fr.mixture_constant(m, d), float(np.abs(0.5 * d * theta).max()))
    CASES[shape] = c
    return c


def loglik_on_device(ops, x, g, theta):
    ll, stats = ops.fld_loglik(x, g, dev(theta))
    assert ll.dtype == stats.dtype == torch.float64 and ll.is_cuda and stats.is_cuda
    assert tuple(ll.shape) == (x.shape[0],) and tuple(stats.shape) == (3,)
    return ll, stats


def grad_on_device(ops, g, x, theta, ll, stats, m=None, v=None, step=1, lr=0.5):
    rows = g.shape[0]
    m = torch.zeros(rows, dtype=torch.float64, device=DEV) if m is None else m
    v = torch.zeros(rows, dtype=torch.float64, device=DEV) if v is None else v
    out = ops.fld_grad_step(g, x, dev(theta), ll, stats[1:2], m, v, step, lr, THETA_MIN)
    assert all(t.dtype == torch.float64 and t.is_cuda and tuple(t.shape) == (rows,) for t in out)
    return [t.cpu().numpy() for t in out]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ------------------------------------------------------------------------------------------------ 1, 2: against the oracle
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_loglik_and_gradient_sums_within_the_derived_bounds(ops, shape):
    n, m, d = shape
    c = case(shape)
    if shape == (130, 4000, 40):
        assert ops.knn_search_chunks(130, 4000, 40, 1) == 32               # the cross-chunk merge
    dx = dev(c["x"])
    dg = dx if shape == SELF else dev(c["g"])
    ll, stats = loglik_on_device(ops, dx, dg, c["theta"])
    got, st = ll.cpu().numpy(), stats.cpu().numpy()
    err = np.abs(got - c["loglik"])
    ratio = float((err / c["delta"]).max())
    print(f"{shape}: loglik error {err.max():.3e}, delta {c['delta'].min():.3e} .. {c['delta'].max():.3e}, ratio {ratio:.4f}")
    assert np.isfinite(got).all() and st[1] == n and st[2] == 0
    assert abs(st[0] - got.sum()) <= 1e-12 * np.abs(got).sum()
    assert (err <= c["delta"]).all(), (shape, ratio)

    theta1, m1, v1, a, b = grad_on_device(ops, dg, dx, c["theta"], ll, stats)
    big = float(c["delta"].max())
    h = 0.5 * np.exp(-c["theta"])
    lim_a = 2.0 * big * c["a"] + 1e-300
    lim_b = 2.0 * big * h * c["b"] + 2.0 ** -24 * (d + 16) * c["norms"] * h * c["a"] + 1e-300
    ratio_a = float((np.abs(a - c["a"]) / lim_a).max())
    ratio_b = float((np.abs(h * (b - c["b"])) / lim_b).max())
    print(f"{shape}: Delta {big:.3e}, A ratio {ratio_a:.4f}, B ratio {ratio_b:.4f}, sum A - n {a.sum() - n:.3e}")
    assert np.isfinite(a).all() and np.isfinite(b).all() and (a >= 0).all() and (b >= 0).all()
    assert ratio_a <= 1.0 and ratio_b <= 1.0, (shape, ratio_a, ratio_b)
    assert abs(a.sum() - n) <= 1e-9 * n
    WORST[IDS[SHAPES.index(shape)]] = max(ratio, ratio_a, ratio_b)


# ------------------------------------------------------------------------------------------------ 3: the Adam step
@pytest.mark.parametrize("shape", [(130, 300, 40), (257, 130, 96)], ids=lambda s: "x".join(map(str, s)))
def test_one_adam_step_is_the_host_formula_on_the_device_sums(am, ops, shape):
    from audio_metrics_amd.metrics import fld
    n, m, d = shape
    c = case(shape)
    rng = np.random.default_rng(41)
    # The seeded momentum has the sign of the (oracle's) gradient, as it has along a run on a smooth loss.  The one operation
    # of the update that the device and the host do not round alike is exp (each within an ulp, 2.2e-16 of h); 1e-14 relative
    # leaves room for that error amplified 45 times by the subtraction inside the gradient, and none for a second
    # cancellation between 0.9 m and 0.1 grad: a momentum opposed to the gradient asks for digits the terms do not have
    # (seeded without regard to the sign, one element in 300 cancelled 60-fold and came out at 1.36e-14).
    sign = np.where(fr.gradient(c["theta"], c["a"], c["b"], d, n) < 0.0, -1.0, 1.0)
    m0, v0 = sign * np.abs(rng.standard_normal(m)) * 0.1, rng.uniform(0.0, 0.05, m)
    step, lr = 7, 0.5
    dx, dg = dev(c["x"]), dev(c["g"])
    ll, stats = loglik_on_device(ops, dx, dg, c["theta"])
    theta1, m1, v1, a, b = grad_on_device(ops, dg, dx, c["theta"], ll, stats, dev(m0), dev(v0), step, lr)
    nf = float(stats[1])
    grad = fld.fld_gradient(c["theta"], a, b, d, nf)
    want_t, want_m, want_v = am.fld_adam_step(c["theta"], grad, m0, v0, step, lr, THETA_MIN)
    for name, got, want in (("m", m1, want_m), ("v", v1, want_v), ("theta", theta1, want_t)):
        rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
        print(f"{shape} {name}: largest relative difference {rel.max():.3e}, exact in {(got == want).mean():.3f} of the elements")
        assert (rel <= 1e-14).all(), (name, rel.max())
    clamped = want_t == THETA_MIN
    assert clamped.any() and (theta1[clamped] == THETA_MIN).all() and (theta1 >= THETA_MIN).all() and (theta1 <= 30.0).all()


# ------------------------------------------------------------------------------------------------ 4: padded views
@pytest.mark.parametrize("shape", [(130, 300, 40), (127, 129, 33)], ids=lambda s: "x".join(map(str, s)))
def test_padded_views_read_no_padding(ops, shape):
    c = case(shape)
    dx, dg = dev(c["x"]), dev(c["g"])
    ll, stats = loglik_on_device(ops, dx, dg, c["theta"])
    plain = [ll.cpu().numpy(), stats.cpu().numpy()] + grad_on_device(ops, dg, dx, c["theta"], ll, stats)
    for fill in (math.nan, 1e30):
        px, pg = padded(c["x"], 4 + (-c["x"].shape[1]) % 4, fill), padded(c["g"], 8 + (-c["g"].shape[1]) % 4, fill)
        ll2, stats2 = loglik_on_device(ops, px, pg, c["theta"])
        wide = [ll2.cpu().numpy(), stats2.cpu().numpy()] + grad_on_device(ops, pg, px, c["theta"], ll2, stats2)
        for a, b in zip(plain, wide):
            assert np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ 5: non-finite inputs
def test_non_finite_rows_and_centres_contribute_nothing(am, ops):
    shape = (130, 300, 40)
    n, m, d = shape
    c = case(shape)
    dx, dg = dev(c["x"]), dev(c["g"])
    ll, stats = loglik_on_device(ops, dx, dg, c["theta"])
    clean = ll.cpu().numpy()
    x2 = c["x"].copy()
    x2[17, 3], x2[128, 39] = np.nan, np.inf
    dx2 = dev(x2)
    ll2, stats2 = loglik_on_device(ops, dx2, dg, c["theta"])
    got, st = ll2.cpu().numpy(), stats2.cpu().numpy()
    keep = np.ones(n, bool)
    keep[[17, 128]] = False
    assert got[17] == -np.inf and got[128] == -np.inf and st[1] == n - 2 and st[2] == 2
    assert np.array_equal(bits(got[keep]), bits(clean[keep]))
    theta1, m1, v1, a, b = grad_on_device(ops, dg, dx2, c["theta"], ll2, stats2)
    assert np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(theta1).all() and np.isfinite(m1).all() and np.isfinite(v1).all()
    want_a, want_b, _ = fr.grad_sums(x2, c["g"], c["theta"])
    big = float(c["delta"].max())
    h = 0.5 * np.exp(-c["theta"])
    assert (np.abs(a - want_a) <= 2.0 * big * want_a + 1e-300).all() and abs(a.sum() - (n - 2)) <= 1e-9 * n
    assert (np.abs(h * (b - want_b)) <= 2.0 * big * h * want_b + 2.0 ** -24 * (d + 16) * c["norms"] * h * want_a + 1e-300).all()

    # a NaN centre (the last one): exactly 0 in both sums; the others have the bits they have beside a finite centre so
    # far away that every term of it underflows, and - up to the rounding of log M - the values they have without it
    g_nan, g_far = c["g"].copy(), c["g"].copy()
    g_nan[-1, 5] = np.nan
    g_far[-1] = 1e15
    out = {}
    for name, gg in (("nan", g_nan), ("far", g_far), ("without", c["g"][:-1])):
        dgg = dev(gg)
        th = c["theta"][:gg.shape[0]]
        l3, s3 = loglik_on_device(ops, dx, dgg, th)
        out[name] = [l3.cpu().numpy()] + grad_on_device(ops, dgg, dx, th, l3, s3)
    assert out["nan"][4][-1] == 0.0 and out["nan"][5][-1] == 0.0
    for got_nan, got_far in zip(out["nan"], out["far"]):
        keep_c = slice(None) if got_nan.shape[0] == n else slice(0, m - 1)
        assert np.array_equal(bits(got_nan[keep_c]), bits(got_far[keep_c]))
    assert np.allclose(out["nan"][4][:-1], out["without"][4], rtol=1e-11, atol=1e-300)
    assert np.allclose(out["nan"][5][:-1], out["without"][5], rtol=1e-11, atol=1e-300)
    # in a fit it keeps theta = 0 and is counted, with one warning
    gen, train = am.AudioMetricsData(True), am.AudioMetricsData(True)
    gen.add(dev(g_nan))
    train.add(dx2)
    with pytest.warns(RuntimeWarning, match="2 training rows, 1 generated rows"):
        fit = am.feature_likelihood_fit(gen, train, steps=5, normalize=None)
    theta = fit["fld_log_variances"].cpu().numpy()
    assert theta[-1] == 0.0 and (theta[:-1] != 0.0).all() and fit["fld_rows_nonfinite"] == 2 and fit["fld_centres_nonfinite"] == 1
    assert np.isfinite(fit["fld_nll_train_history"]).all() and fit["fld_nll_train_history"].shape == (6,)


# ------------------------------------------------------------------------------------------------ 6: determinism
@pytest.mark.parametrize("shape", [(130, 4000, 40), SELF], ids=lambda s: "x".join(map(str, s)))
def test_two_calls_give_the_same_bits(am, ops, shape):
    c = case(shape)
    dx = dev(c["x"])
    dg = dx if shape == SELF else dev(c["g"])
    runs = []
    for _ in range(2):
        ll, stats = loglik_on_device(ops, dx, dg, c["theta"])
        runs.append([ll.cpu().numpy(), stats.cpu().numpy()] + grad_on_device(ops, dg, dx, c["theta"], ll, stats))
    for a, b in zip(*runs):
        assert np.array_equal(bits(a), bits(b))
    gen, train = am.AudioMetricsData(True), am.AudioMetricsData(True)
    gen.add(dev(c["g"]))
    train.add(dx)
    fits = [am.feature_likelihood_fit(gen, train, steps=5) for _ in range(2)]
    assert np.array_equal(bits(fits[0]["fld_log_variances"].cpu().numpy()), bits(fits[1]["fld_log_variances"].cpu().numpy()))
    assert np.array_equal(bits(fits[0]["fld_nll_train_history"]), bits(fits[1]["fld_nll_train_history"]))


# ------------------------------------------------------------------------------------------------ 7: underflow
def test_every_term_but_the_largest_underflows(ops):
    n, m, d = 130, 300, 40
    rng = np.random.default_rng(51)
    g = (0.02 * rng.standard_normal((m, d))).astype(np.float32)
    g[:, 0] += 0.5 * np.arange(m, dtype=np.float32) - 75.0                  # centres half a unit apart along one axis
    x = g[rng.choice(m, n, replace=False)].copy()
    x[:, 0] += np.float32(0.1)                                              # each row a tenth from its centre: gap 0.15 in d2
    theta = np.full(m, THETA_MIN)
    h, cc = 0.5 * math.exp(-THETA_MIN), 0.5 * d * THETA_MIN
    d2 = fr.sq_dists(x, g)
    part = np.partition(d2, 1, axis=1)
    assert math.exp(-h * (part[:, 1] - part[:, 0]).min()) == 0.0 and len(np.unique(x, axis=0)) == n
    dx, dg = dev(x), dev(g)
    ll, stats = loglik_on_device(ops, dx, dg, theta)
    got = ll.cpu().numpy()
    nearest = ops.knn_search(dx, dg, 1, squared=True)[0][:, 0].cpu().numpy().astype(np.float64)
    want = -h * nearest - cc - fr.mixture_constant(m, d)
    x64, g64 = x.astype(np.float64), g.astype(np.float64)
    lim = fr.delta(d, float((x64 * x64).sum(1).max()), float((g64 * g64).sum(1).max()), h, want + fr.mixture_constant(m, d), abs(cc))
    print("underflow: largest |device - (-h min d2 - c - const)| / delta", float((np.abs(got - want) / lim).max()))
    assert np.isfinite(got).all() and (np.abs(got - want) <= lim).all()
    assert (np.abs(got - fr.loglik(x, g, theta)) <= lim).all()
    theta1, m1, v1, a, b = grad_on_device(ops, dg, dx, theta, ll, stats)
    assert abs(a.sum() - n) <= 1e-9 * n and np.abs(a - np.round(a)).max() <= 1e-9 and a.max() <= 1.0 + 1e-9      # a row belongs to one centre alone


# ------------------------------------------------------------------------------------------------ 8: end to end
def test_end_to_end_against_the_oracle(am):
    d, n, t, m, copies = 40, 130, 140, 150, 10
    rng = np.random.default_rng(61)
    centres = rng.standard_normal((8, d)) * 3.0

    def draw(k):
        return (centres[rng.integers(0, 8, k)] + rng.standard_normal((k, d))).astype(np.float32)
    train, test, gen = draw(n), draw(t), draw(m)
    gen[:copies] = train[:copies] + (1e-3 * rng.standard_normal((copies, d))).astype(np.float32)
    sets = []
    for rows in (gen, train, test):
        s = am.AudioMetricsData(True)
        s.add(dev(rows))
        sets.append(s)
    dgen, dtrain, dtest = sets
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = am.feature_likelihood_divergence(dgen, dtrain, dtest, baseline_nll=0.25, return_rows=True)
    assert out["fld_steps"] == 100 and out["fld_rows_nonfinite"] == (0, 0, 0) and out["fld_baseline_nll"] == 0.25
    theta = out["fld_log_variances"]
    # the oracle on the rows the device read: the stored statistics of the training set, the same f64 operations
    mean, var = dtrain.mean.cpu().numpy().reshape(-1), np.diagonal(dtrain.cov.cpu().numpy())
    assert np.allclose(var, train.astype(np.float64).var(0, ddof=1), rtol=1e-6)       # unbiased; accumulated from float32 rows
    gn, xn, tn = (fr.normalize(a, mean, var) for a in (gen, train, test))
    consts = fr.mixture_constant(m, d)
    norm2 = lambda a: float((a.astype(np.float64) ** 2).sum(1).max())                        # noqa: E731
    hmax, cmax = float(0.5 * np.exp(-theta).max()), float(np.abs(0.5 * d * theta).max())
    for name, rows, key in (("train", xn, "fld_train_loglik"), ("test", tn, "fld_test_loglik")):
        want = fr.loglik(rows, gn, theta)
        lim = fr.delta(d, norm2(rows), norm2(gn), hmax, want + consts, cmax)
        err = np.abs(out[key] - want)
        print(f"e2e {name}: per-row error / delta {float((err / lim).max()):.4f}; nll {out['fld_nll_' + name]:.6f} "
              f"oracle {-want.mean() / d:.6f} bound {lim.mean() / d:.3e}")
        assert (err <= lim).all()
        assert abs(out["fld_nll_" + name] - (-want.mean() / d)) <= lim.mean() / d
    assert out["fld_generalization_gap"] == out["fld_nll_test"] - out["fld_nll_train"] and out["fld_nll_train"] < out["fld_nll_test"]
    assert out["fld"] == 100.0 * (out["fld_nll_test"] - 0.25)
    host = am.fld_from_logliks(out["fld_train_loglik"], out["fld_test_loglik"], d, baseline_nll=0.25)
    assert all(math.isclose(host[k], out[k], rel_tol=1e-12) for k in host)
    # the optimiser: the oracle's loss at the device's theta against the oracle's own 100-step fit
    theta_ref, history = fr.fit(xn, gn, steps=100, lr=0.5, theta_min=-10.0)
    gap = abs(fr.loss(xn, gn, theta) - history[-1]) / d
    print(f"e2e: oracle loss at the device's theta - oracle's own fit = {gap:.3e} per dimension (bound 0.005); "
          f"largest |theta - theta_ref| {np.abs(theta - theta_ref).max():.3e}")
    assert gap <= 0.005
    # the copies
    score = out["fld_overfit_score"]
    assert set(np.argsort(score)[-copies:]) == set(range(copies)) and (theta[:copies] == -10.0).all()
    assert (out["fld_nearest_train"][:copies] == np.arange(copies)).all()
    want_score = fr.overfit_scores(gn, xn, tn, theta)
    assert np.allclose(score, want_score, rtol=1e-3, atol=2.0 ** -24 * (d + 16) * (norm2(gn) + max(norm2(xn), norm2(tn))) * hmax * 2)
    assert math.isclose(out["fld_overfit_fraction"], float((score > 0).mean()), rel_tol=1e-12)
    fit = am.feature_likelihood_fit(dgen, dtrain)
    assert np.array_equal(bits(fit["fld_log_variances"].cpu().numpy()), bits(theta)) and fit["fld_nll_train"] == out["fld_nll_train"]
    assert fit["fld_nll_train_history"].shape == (101,) and fit["fld_nll_train_history"][-1] == out["fld_nll_train"]
    assert fit["fld_nll_train_history"][-1] < fit["fld_nll_train_history"][0]
    # authenticity, on the rows as they are
    auth = am.authenticity_score(dgen, dtrain, return_rows=True)
    want_auth, want_nearest, margin = fr.authenticity(gen, train)
    two = np.partition(np.sqrt(fr.sq_dists(gen, train)), 1, axis=1)
    clear = (margin > 1e-5) & (two[:, 1] - two[:, 0] > 1e-5 * two[:, 1])          # neither the comparison nor the nearest row is a tie
    assert (~clear).mean() <= 0.02
    assert np.array_equal(auth["authentic"][clear], want_auth[clear]) and not auth["authentic"][:copies].any()
    assert np.array_equal(auth["authenticity_nearest_train"][clear], want_nearest[clear])
    assert math.isclose(auth["authenticity"], float(auth["authentic"].mean()), rel_tol=1e-12)
    assert math.isclose(auth["authenticity"], am.authenticity_score(dgen, dtrain)["authenticity"], rel_tol=1e-12)
