"""sinkhorn_divergence on the device against the float64 oracle of tests/sinkhorn_reference.py run on the same float32 rows.

  1  a fixed number of steps (rtol = 0, max_iter = len(schedule) + 8): all four potentials within the solve bound
     sum_t delta(eps_t) of the oracle's after the same steps, S within four times that
  2  the default stop rule: the device stops at the oracle's step in all three solves, on sets whose oracle run passes its
     stopping step clearly - change >= 2 tol on the step before, <= tol / 2 on the step itself.  The averaged solve of the
     1 000-row reference contracts by 0.46 per step, so no seed puts a factor 2 on both sides of ITS stopping step
     (2 x 2 > 1 / 0.46); that one solve is held to the factor 1.4 its contraction allows, every other one to 2.
  3  S(x, x), the marginal error, the potentials' means, the reference-side cache, max_iter reached, the default blur.

Measured on the MI355X (the figures the tests print): see profiles/sinkhorn/accuracy.txt."""
import math
import warnings

import numpy as np
import pytest
import torch

import sinkhorn_reference as sr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (n, m, D, shift of the reference, seed of x, seed of y, clearance of the (XY, XX, YY) stopping steps asserted on the oracle)
CASES = [(300, 257, 64, 0.3, 4, 1065, (2.0, 2.0, 2.0)),
         (127, 129, 33, 0.0, 16, 1067, (2.0, 2.0, 2.0)),
         (130, 1000, 40, 0.2, 9, 1006, (2.0, 2.0, 1.4))]
IDS = ["300x257x64", "127x129x33", "130x1000x40"]
RTOL = 1e-5
MEASURED = {}


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
    if MEASURED:
        sr.record_accuracy("solves: largest |device - oracle| / bound (bound: 1)", [f"{k}: {v}" for k, v in MEASURED.items()])


def rows(seed, n, d, shift):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32) + np.float32(shift)


def data_set(am, a):
    s = am.AudioMetricsData(True)
    s.add(torch.as_tensor(a).to(DEV))
    return s


_SHARED = {}


def case_data(am, ops, index):
    """Rows, sets, the default blur (0.25 x the device's own median distance) and the oracle's default run: computed once."""
    if index not in _SHARED:
        n, m, d, shift, xs, ys, clearance = CASES[index]
        x, y = rows(xs, n, d, 0.0), rows(ys, m, d, shift)
        sx, sy = data_set(am, x), data_set(am, y)
        blur = 0.25 * math.sqrt(float(ops.pairwise_select_sq(sy.embeddings)))
        x2 = float((x.astype(np.float64) ** 2).sum(1).max())
        y2 = float((y.astype(np.float64) ** 2).sum(1).max())
        _SHARED[index] = dict(x=x, y=y, sx=sx, sy=sy, blur=blur, x2=x2, y2=y2, d=d, clearance=clearance,
                              oracle=sr.divergence(x, y, blur, rtol=RTOL, max_iter=200))
    return _SHARED[index]


def bounds(c, o):
    """The solve bounds of the three solves of oracle run o on the sets of case c."""
    return (sr.solve_bound(o["xy"]["history"], c["d"], c["x2"], c["y2"]),
            sr.solve_bound(o["xx"]["history"], c["d"], c["x2"], c["x2"]),
            sr.solve_bound(o["yy"]["history"], c["d"], c["y2"], c["y2"]))


@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_a_fixed_number_of_steps_within_the_solve_bound(am, ops, index):
    from audio_metrics_amd.metrics import sinkhorn
    c = case_data(am, ops, index)
    x, y, blur = c["x"], c["y"], c["blur"]
    sched_xy = sr.schedule(sr.diam2(x, y), blur, 0.5)
    max_iter = len(sched_xy) + 8
    o = sr.divergence(x, y, blur, rtol=0.0, max_iter=max_iter)
    assert o["iterations"] == (max_iter,) * 3 and o["converged"] == (False,) * 3
    b_xy, b_xx, b_yy = bounds(c, o)
    # the four potentials, from the solves themselves
    ex, ey = ops.as_matrix(c["sx"].embeddings), ops.as_matrix(c["sy"].embeddings)
    f_star, g_star, _, it_xy, ok_xy = sinkhorn._solve_cross(ex, ey, am.sinkhorn_schedule(sr.diam2(x, y), blur, 0.5), 0.0, max_iter)
    p_star, it_xx, ok_xx = sinkhorn._solve_self(ex, am.sinkhorn_schedule(sr.diam2(x), blur, 0.5), 0.0, max_iter)
    q_star, it_yy, ok_yy = sinkhorn._solve_self(ey, am.sinkhorn_schedule(sr.diam2(y), blur, 0.5), 0.0, max_iter)
    assert (it_xy, it_xx, it_yy) == (max_iter,) * 3 and not (ok_xy or ok_xx or ok_yy)
    errs = {"f*": (np.abs(f_star.cpu().numpy() - o["xy"]["f_star"]).max(), b_xy), "g*": (np.abs(g_star.cpu().numpy() - o["xy"]["g_star"]).max(), b_xy),
            "p*": (np.abs(p_star.cpu().numpy() - o["xx"]["star"]).max(), b_xx), "q*": (np.abs(q_star.cpu().numpy() - o["yy"]["star"]).max(), b_yy)}
    # the divergence, through the front end
    with pytest.warns(RuntimeWarning, match="did not reach"):
        got = am.sinkhorn_divergence(c["sx"], data_set(am, y), blur=blur, rtol=0.0, max_iter=max_iter, return_potentials=True)
    assert got["sinkhorn_iterations"] == (max_iter,) * 3 and got["sinkhorn_converged"] == (False,) * 3
    errs["S"] = (abs(got["sinkhorn_divergence"] - o["divergence"]), 4.0 * max(b_xy, b_xx, b_yy))
    errs["f* - p*"] = (np.abs(got["candidate_potential"] - o["candidate_potential"]).max(), b_xy + b_xx)
    errs["g* - q*"] = (np.abs(got["reference_potential"] - o["reference_potential"]).max(), b_xy + b_yy)
    for name, (err, lim) in errs.items():
        print(f"{IDS[index]} {max_iter} steps {name}: error {err:.3e}, bound {lim:.3e}, ratio {err / lim:.4f}")
    MEASURED[f"{IDS[index]}, {max_iter} steps"] = ", ".join(f"{k} {e / b:.4f}" for k, (e, b) in errs.items())
    for name, (err, lim) in errs.items():
        assert err <= lim, (name, err, lim)
    assert got["sinkhorn_divergence"] == got["sinkhorn_ot_xy"] - 0.5 * got["sinkhorn_ot_xx"] - 0.5 * got["sinkhorn_ot_yy"]
    assert got["sinkhorn_w2"] == math.sqrt(2.0 * max(got["sinkhorn_divergence"], 0.0)) and got["sinkhorn_blur"] == blur


@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_the_default_stop_rule_stops_at_the_oracles_step(am, ops, index):
    c = case_data(am, ops, index)
    o = c["oracle"]
    assert o["converged"] == (True, True, True)
    for key, x_rows, clearance in zip(("xy", "xx", "yy"), ((c["x"], c["y"]), (c["x"],), (c["y"],)), c["clearance"]):
        h = o[key]["history"]
        assert len(h) - 1 >= len(sr.schedule(sr.diam2(*x_rows), c["blur"], 0.5))       # the step before the stop was a checked one
        before, after = h[-2][2] / (RTOL * h[-2][3]), h[-1][2] / (RTOL * h[-1][3])
        print(f"{IDS[index]} {key}: {len(h)} steps, change / tol {before:.3f} on the step before, {after:.3f} on the last")
        assert before >= clearance and after <= 1.0 / clearance, (key, before, after)
    got = am.sinkhorn_divergence(c["sx"], c["sy"], return_potentials=True)
    print(IDS[index], "device", got["sinkhorn_iterations"], "oracle", o["iterations"], "S", got["sinkhorn_divergence"], o["divergence"])
    assert got["sinkhorn_blur"] == c["blur"]                                           # blur=None is 0.25 x the median
    assert got["sinkhorn_iterations"] == o["iterations"] and got["sinkhorn_converged"] == (True, True, True)
    b = bounds(c, o)
    err, lim = abs(got["sinkhorn_divergence"] - o["divergence"]), 4.0 * max(b)
    assert err <= lim, (err, lim)
    # the row-marginal error of the XY plan: exp is 1-Lipschitz up to its own value, f and f* each within the solve bound
    eps = c["blur"] ** 2
    slack = (1.0 + o["marginal_error"]) * math.expm1(2.0 * b[0] / eps)
    print(IDS[index], "marginal error", got["sinkhorn_marginal_error"], "oracle", o["marginal_error"], "slack", slack)
    assert abs(got["sinkhorn_marginal_error"] - o["marginal_error"]) <= slack
    # the potentials say which rows carry the divergence: their means add up to it
    total = got["candidate_potential"].mean() + got["reference_potential"].mean()
    assert got["candidate_potential"].shape == (c["x"].shape[0],) and got["reference_potential"].shape == (c["y"].shape[0],)
    assert got["candidate_potential"].dtype == got["reference_potential"].dtype == np.float64
    assert abs(total - got["sinkhorn_divergence"]) <= 1e-12 * max(abs(got["sinkhorn_ot_xy"]), 1.0)
    MEASURED[f"{IDS[index]}, default stop"] = (f"S {err / lim:.4f}, steps {got['sinkhorn_iterations']}, marginal error "
                                               f"{got['sinkhorn_marginal_error']:.3e} (oracle {o['marginal_error']:.3e})")
    # an explicit blur of the same value: the same bits
    again = am.sinkhorn_divergence(c["sx"], c["sy"], blur=c["blur"])
    assert again["sinkhorn_divergence"] == got["sinkhorn_divergence"] and again["sinkhorn_iterations"] == got["sinkhorn_iterations"]


def test_a_set_against_itself(am, ops):
    c = case_data(am, ops, 1)
    x, blur = c["x"], c["blur"]
    o = sr.divergence(x, x, blur, rtol=RTOL, max_iter=200)
    # (Between identical sets exp(-C / eps) is close to the identity, so the pair (f + c, g - c) is almost free in c: the
    # alternating solve drifts along it and reaches max_iter in the oracle as on the device; OT_xy = mean f* + mean g* does
    # not depend on c.)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = am.sinkhorn_divergence(c["sx"], c["sx"], blur=blur)
    assert got["sinkhorn_iterations"] == o["iterations"] and got["sinkhorn_converged"] == o["converged"]
    b_xy = sr.solve_bound(o["xy"]["history"], c["d"], c["x2"], c["x2"])
    b_xx = sr.solve_bound(o["xx"]["history"], c["d"], c["x2"], c["x2"])
    lim = 4.0 * max(b_xy, b_xx)
    print("S(x, x)", got["sinkhorn_divergence"], "oracle", o["divergence"], "bound", lim, got["sinkhorn_iterations"], o["iterations"])
    assert abs(got["sinkhorn_divergence"]) <= lim and abs(got["sinkhorn_divergence"] - o["divergence"]) <= lim
    assert got["sinkhorn_ot_xx"] == got["sinkhorn_ot_yy"] and got["sinkhorn_w2"] == math.sqrt(2.0 * max(got["sinkhorn_divergence"], 0.0))
    MEASURED["127x33 against itself"] = f"|S| / bound {abs(got['sinkhorn_divergence']) / lim:.4f}"


def test_the_reference_side_cache(am, ops, monkeypatch):
    from audio_metrics_amd.metrics.kad import reference_cache
    c = case_data(am, ops, 1)
    blur = c["blur"]
    calls = []
    real = ops.softmin
    monkeypatch.setattr(ops, "softmin", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    ref = data_set(am, c["y"])
    first = am.sinkhorn_divergence(c["sx"], ref, blur=blur, return_potentials=True)
    uncached_calls = len(calls)
    assert len(reference_cache(ref).sinkhorn) == 1
    second = am.sinkhorn_divergence(c["sx"], ref, blur=blur, return_potentials=True)
    cached_calls = len(calls) - uncached_calls
    assert cached_calls == uncached_calls - (first["sinkhorn_iterations"][2] + 1)       # the YY solve and its final pass were not run
    fresh = am.sinkhorn_divergence(c["sx"], data_set(am, c["y"]), blur=blur, return_potentials=True)
    for other in (second, fresh):                                                      # a cached call returns the bits of an uncached one
        for key, v in first.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v.view(np.uint64), other[key].view(np.uint64)), key
            else:
                assert v == other[key], key
    # another blur is another entry; appended rows drop them all
    am.sinkhorn_divergence(c["sx"], ref, blur=1.5 * blur)
    assert len(reference_cache(ref).sinkhorn) == 2
    ref.add(torch.as_tensor(c["y"][:5]).to(DEV))
    assert reference_cache(ref).sinkhorn == {}
    grown = am.sinkhorn_divergence(c["sx"], ref, blur=blur)
    assert grown["sinkhorn_ot_yy"] != first["sinkhorn_ot_yy"] and len(reference_cache(ref).sinkhorn) == 1


def test_max_iter_reached_warns_once_and_says_so(am, ops):
    c = case_data(am, ops, 1)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = am.sinkhorn_divergence(c["sx"], data_set(am, c["y"]), blur=c["blur"], max_iter=7)
    assert [w.category for w in caught] == [RuntimeWarning] and "XY, XX, YY solves did not reach" in str(caught[0].message)
    assert got["sinkhorn_converged"] == (False, False, False) and got["sinkhorn_iterations"] == (7, 7, 7)
    assert math.isfinite(got["sinkhorn_divergence"])
    # the plateau of change / magnitude far past convergence: the rounding jitter of the f32 z that rtol has to stay above
    ratios = []
    ex = ops.as_matrix(c["sx"].embeddings)
    eps = c["blur"] ** 2
    p = torch.zeros(ex.shape[0], dtype=torch.float64, device=DEV)
    for step in range(60):
        p, change, magnitude = ops.softmin(ex, ex, p, eps, prev=p, damping=0.5)
        if step >= 40:
            ratios.append(float(change) / float(magnitude))
    print("plateau of change / magnitude, steps 41 - 60 at blur^2:", max(ratios))
    MEASURED["plateau of change / magnitude (127x33 against itself, steps 41 - 60 at blur^2)"] = f"{max(ratios):.3e}; rtol = {RTOL:g} is {RTOL / max(ratios):.0f} x that"
    assert RTOL >= 20.0 * max(ratios)
