"""Error bars for the Frechet distance: a closed-form large-sample standard error, a two-model comparison against one
reference set and a per-row attribution, all from the first-order INFLUENCE of every row on the distance - one quadratic
form per row (ops.frechet_influence: one N x D x D pass on the f64 matrix cores), no resampling.

With M = cov_x cov_y and fd = |mu_x - mu_y|^2 + tr cov_x + tr cov_y - 2 tr M^(1/2), let A be the symmetric positive
definite matrix with A cov_x A = cov_y (the Gaussian optimal-transport map; ops.frechet_maps forms it and its inverse from
the Newton-Schulz solve's final iterate, no explicit inverse).  Then d tr M^(1/2) / d cov_x = A / 2, d / d cov_y = A^-1 / 2 and

  psi_x(x) =  2 (mu_x - mu_y)^T (x - mu_x) + (x - mu_x)^T (I - A) (x - mu_x) - tr((I - A) cov_x)          per candidate row
  psi_y(y) = -2 (mu_x - mu_y)^T (y - mu_y) + (y - mu_y)^T (I - A^-1) (y - mu_y) - tr((I - A^-1) cov_y)    per reference row
  var(fd) ~ s^2(psi_x) / n + s^2(psi_y) / m                                                               (s^2: ddof = 1)

Rows that are windows of the same track are not independent: with one label per row (the song), the cluster-robust form
  var_x = G / (G - 1) * sum_g (sum_{i in g} psi_i)^2 / n^2
takes the songs as the sampling units.  Two candidates A and B against the same reference rows share them, so
  var(fd_A - fd_B) = s^2(psi_A) / n_a + s^2(psi_B) / n_b + s^2(psi_y^A - psi_y^B) / m,     z = (fd_A - fd_B) / sqrt(var),
one-sided p = Phi(z) (small: A is significantly closer to the reference than B), two-sided p = 2 Phi(-|z|) - the conventions
of kernel_audio_distance_compare.

Two caveats.  The interval describes the sampling variability at this sample size; it does NOT remove the 1 / N bias of the
Frechet distance (pair it with frechet_distance_inf), and differences between sets of unequal size carry different biases.
Under equal distributions A = I and mu_x = mu_y, so psi vanishes and the estimate tends to 0: it is NOT a test of fad = 0."""
import math
import statistics
import warnings

import numpy as np
import torch

from .. import hip_ops as ops
from ..data import AudioMetricsData, ensure_tensor
from ._groups import labelled_rows
from .fad import NS_MAX_ITER, NS_TOL

NAN = float("nan")


def _phi(z):
    return 0.5 * math.erfc(-z / math.sqrt(2.0))


def _vec(a, name):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 1:
        raise ValueError(f"{name} must be a vector of influence values, got shape {a.shape}")
    return a


def _units(groups, n, name):
    """(unit index per row, number of units) of one side: every row its own unit without labels."""
    if groups is None:
        if n < 2:
            raise ValueError(f"{name} holds {n} rows: a variance needs at least 2 units on every side")
        return None, n
    labels = np.asarray(groups.cpu() if isinstance(groups, torch.Tensor) else groups)
    if labels.ndim != 1 or len(labels) != n:
        raise ValueError(f"{name}: {labels.shape} labels for {n} influence values (one label per row)")
    if labels.dtype.kind not in "iu":
        raise ValueError(f"{name} must hold integer labels, got dtype {labels.dtype}")
    uniq, inverse = np.unique(labels, return_inverse=True)
    if len(uniq) < 2:
        raise ValueError(f"{name} names {len(uniq)} unit(s): a variance needs at least 2 units on every side")
    return inverse.reshape(-1), len(uniq)


def _side_variance(psi, inverse, units):
    """The variance contribution of one side: s^2(psi) / n over rows, or the cluster-robust form over labelled units."""
    n = len(psi)
    if inverse is None:
        return psi.var(ddof=1) / n
    per_unit = np.bincount(inverse, weights=psi, minlength=units)
    return units / (units - 1.0) * float(np.sum(per_unit * per_unit)) / (float(n) * n)


def _variance_problem(var, *psis):
    if not all(np.isfinite(p).all() for p in psis):
        return "an influence value is not finite (a row with a NaN or inf element)"
    if not var > 0.0:
        return "the variance estimate is 0"
    return None


def frechet_standard_error(psi_x, psi_y, groups_x=None, groups_y=None):
    """The standard error of the Frechet distance from the influence values of its candidate rows (psi_x) and reference rows
    (psi_y) - host arithmetic, float64 numpy.  groups_x / groups_y: one integer label per row (any order, any values) make
    the labelled units (songs) the sampling units of that side (cluster-robust variance) instead of the rows.  Fewer than 2
    units on a side raise; a non-finite influence value or a variance of 0 give NaN with ONE RuntimeWarning.  The error is
    the first-order term for two distributions that differ: under equality it tends to 0, it is NOT a test of fad = 0."""
    psi_x, psi_y = _vec(psi_x, "psi_x"), _vec(psi_y, "psi_y")
    inv_x, gx = _units(groups_x, len(psi_x), "groups_x" if groups_x is not None else "psi_x")
    inv_y, gy = _units(groups_y, len(psi_y), "groups_y" if groups_y is not None else "psi_y")
    with np.errstate(invalid="ignore", over="ignore"):
        var = _side_variance(psi_x, inv_x, gx) + _side_variance(psi_y, inv_y, gy)
    problem = _variance_problem(var, psi_x, psi_y)
    if problem:
        warnings.warn(f"frechet_standard_error: {problem}: the standard error is NaN", RuntimeWarning, stacklevel=2)
        return NAN
    return float(math.sqrt(var))


def frechet_difference_test(fad_a, fad_b, psi_a, psi_b, psi_ya, psi_yb, groups_a=None, groups_b=None, groups_y=None):
    """The comparison of two candidate sets against ONE reference from their influence values (psi_a, psi_b: per row of A, of
    B; psi_ya, psi_yb: per REFERENCE row, from the solve against A and against B) - host arithmetic, float64 numpy.  Returns
    {"difference": fad_a - fad_b, "std_error", "z", "p_value": Phi(z) (small: A is closer), "p_value_two_sided"}.  The
    reference enters through psi_ya - psi_yb (both distances share its rows); A and B count as independent samples.  Labels
    as in frechet_standard_error.  A non-finite influence value or a variance of 0 (the same rows handed in twice have
    psi_ya == psi_yb and difference 0) give NaN for the error, z and the p-values, with ONE RuntimeWarning."""
    psi_a, psi_b = _vec(psi_a, "psi_a"), _vec(psi_b, "psi_b")
    psi_ya, psi_yb = _vec(psi_ya, "psi_ya"), _vec(psi_yb, "psi_yb")
    if len(psi_ya) != len(psi_yb):
        raise ValueError(f"psi_ya and psi_yb hold one entry per reference row ({len(psi_ya)}, {len(psi_yb)})")
    inv_a, ga = _units(groups_a, len(psi_a), "groups_a" if groups_a is not None else "psi_a")
    inv_b, gb = _units(groups_b, len(psi_b), "groups_b" if groups_b is not None else "psi_b")
    inv_y, gy = _units(groups_y, len(psi_ya), "groups_y" if groups_y is not None else "psi_ya")
    diff = float(fad_a) - float(fad_b)
    with np.errstate(invalid="ignore", over="ignore"):
        var = _side_variance(psi_a, inv_a, ga) + _side_variance(psi_b, inv_b, gb) + _side_variance(psi_ya - psi_yb, inv_y, gy)
    same = len(psi_a) == len(psi_b) and np.array_equal(psi_a, psi_b) and np.array_equal(psi_ya, psi_yb)
    problem = _variance_problem(var, psi_a, psi_b, psi_ya, psi_yb)
    if same and not problem:
        problem = "the two candidate sets hold the same rows: the difference has no sampling distribution to test against"
    if problem:
        warnings.warn(f"frechet_difference_test: {problem}: the standard error, z and the p-values are NaN", RuntimeWarning, stacklevel=2)
        return {"difference": diff, "std_error": NAN, "z": NAN, "p_value": NAN, "p_value_two_sided": NAN}
    se = math.sqrt(var)
    z = diff / se
    return {"difference": diff, "std_error": float(se), "z": z, "p_value": _phi(z), "p_value_two_sided": 2.0 * _phi(-abs(z))}


# ------------------------------------------------------------------ the device side
def _checked_set(data, groups, what, words):
    """(stored rows, n, labels or None) of one set after every host check; no device call."""
    if groups is not None:
        rows, n, labels = labelled_rows(data, groups, what, words)
    else:
        rows, labels = getattr(data, "embeddings", None), None
        n = int(rows.shape[0]) if rows is not None else 0
        if rows is None or n == 0:
            raise ValueError(f"{what} scores the stored rows of {words}, which keeps none "
                             f"(store_embeddings={getattr(data, 'store_embeddings', None)})")
    if getattr(data, "n", None) is None or int(data.n) != n:
        raise ValueError(f"{what}: {words} stores {n} rows but its statistics describe {getattr(data, 'n', None)}: the influence "
                         "values belong to the rows the mean and covariance were taken from")
    d = int(rows.shape[1])
    if n <= d:
        raise ValueError(f"{what}: {words} holds {n} rows of {d} dimensions: with no more rows than dimensions the covariance is "
                         "singular and the optimal-transport map between the two Gaussians is undefined; score small sets with "
                         "frechet_distance_per_group")
    if labels is not None:
        labels = np.asarray(labels.cpu())
        if len(np.unique(labels)) < 2:
            raise ValueError(f"{what}: the labels of {words} name fewer than 2 units: a variance needs at least 2 on every side")
    return rows, n, labels


def _same_width(what, *rows):
    for e in rows[:-1]:
        if e.shape[1] != rows[-1].shape[1]:
            raise ValueError(f"{what}: feature widths differ: {e.shape[1]} and {rows[-1].shape[1]}")


def _device_of(rows):
    if rows.is_cuda:
        return rows.device
    from ..data import default_device
    return torch.device(default_device())


def _pair(x, rows_x, y, rows_y, device, max_iter=NS_MAX_ITER):
    """The solve with its maps and both influence passes of one (candidate, reference) pair.  Returns {"fd", "stop",
    "residual", "psi_x", "psi_y" (device), "sums_x", "sums_y" (device [4])}; with stop != 1 no row pass runs."""
    mu_x, cov_x, mu_y, cov_y = (ensure_tensor(t).to(device, torch.float64) for t in (x.mean, x.cov, y.mean, y.cov))
    mu_x, mu_y = mu_x.reshape(-1), mu_y.reshape(-1)
    res = ops.frechet_maps(mu_x, cov_x, mu_y, cov_y, max_iter, NS_TOL)
    out = {"fd": res["fd"], "stop": res["stop"], "residual": NAN, "psi_x": None, "psi_y": None, "sums_x": None, "sums_y": None}
    if res["stop"] != 1:
        return out
    a, a_inv = res["map_xy"], res["map_yx"]
    eye = torch.eye(a.shape[0], dtype=torch.float64, device=a.device)
    bx, by = eye - a, eye - a_inv
    dmu = mu_x - mu_y
    # c0 = -tr(B cov) (B and cov symmetric: the sum of the elementwise product) and the map's residual: one small read-back
    resid = torch.linalg.matrix_norm(a @ cov_x @ a - cov_y) / torch.linalg.matrix_norm(cov_y)
    c0x, c0y, residual = torch.stack([-(bx * cov_x).sum(), -(by * cov_y).sum(), resid]).cpu().tolist()
    out["residual"] = residual
    out["psi_x"], out["sums_x"] = ops.frechet_influence(ops.as_rows(rows_x.to(device)), mu_x, bx, 2.0 * dmu, c0x)
    out["psi_y"], out["sums_y"] = ops.frechet_influence(ops.as_rows(rows_y.to(device)), mu_y, by, -2.0 * dmu, c0y)
    return out


def _variance_from_sums(s):
    """(s^2(psi) / n, every row finite) from {sum psi, sum psi^2, finite rows, non-finite rows}"""
    total, squares, n, bad = (float(v) for v in s)
    if bad > 0 or n < 2:
        return NAN, False
    return max(squares - total * total / n, 0.0) / (n - 1.0) / n, True


def frechet_distance_with_error(cand: AudioMetricsData, ref: AudioMetricsData, groups=None, ref_groups=None, confidence=0.95,
                                return_rows=False):
    """Frechet distance of candidate set `cand` against reference set `ref` with its closed-form standard error: one solve
    (the chain of frechet_distance; "fad" equals it bit for bit), the two optimal-transport maps and one influence pass per
    set.  Returns {"fad", "fad_std_error", "fad_ci_low", "fad_ci_high": fad -/+ the normal quantile of `confidence` times the
    error, "fad_map_residual": |A cov_x A - cov_y|_F / |cov_y|_F (reported, never thresholded), "fad_units_candidate",
    "fad_units_reference": the sampling units per side}.  groups / ref_groups: one integer label per stored row (the song a
    window comes from; any order, any values) - the labelled units replace the rows as sampling units of that side.  PASS
    THEM WHENEVER THE ROWS ARE WINDOWS OF TRACKS: the row-level error is several times too small there.  return_rows=True
    adds "candidate_influence" f64 [n] and "reference_influence" f64 [m] (numpy, stored row order): which clips push the
    distance up.  Both sets need more rows than dimensions.  A solve that did not converge, a row with a non-finite element
    or a variance of 0 give NaN for the error figures and ONE RuntimeWarning; the distance is still returned.  The interval
    describes sampling variability at this sample size - it does not remove the 1 / N bias (see frechet_distance_inf) - and
    under equal distributions the error tends to 0: it is NOT a test of fad = 0."""
    what = "frechet_distance_with_error"
    confidence = float(confidence)
    if not 0.0 < confidence < 1.0:
        raise ValueError(f"confidence={confidence!r} must lie strictly between 0 and 1")
    rows_x, n, labels_x = _checked_set(cand, groups, what, "its candidate set")
    rows_y, m, labels_y = _checked_set(ref, ref_groups, what, "its reference set")
    _same_width(what, rows_x, rows_y)
    pair = _pair(cand, rows_x, ref, rows_y, _device_of(rows_x))
    out = {"fad": pair["fd"], "fad_std_error": NAN, "fad_ci_low": NAN, "fad_ci_high": NAN, "fad_map_residual": pair["residual"],
           "fad_units_candidate": n if labels_x is None else len(np.unique(labels_x)),
           "fad_units_reference": m if labels_y is None else len(np.unique(labels_y))}
    problem, se = None, NAN
    if pair["stop"] != 1:
        problem = f"the Newton-Schulz solve ended with stop code {pair['stop']} (not converged): the optimal-transport map is undefined"
        if return_rows:
            out.update(candidate_influence=np.full(n, NAN), reference_influence=np.full(m, NAN))
    elif labels_x is None and labels_y is None and not return_rows:
        sums = torch.stack([pair["sums_x"], pair["sums_y"]]).cpu().numpy()            # the one read-back: 64 bytes
        (vx, ok_x), (vy, ok_y) = _variance_from_sums(sums[0]), _variance_from_sums(sums[1])
        if not (ok_x and ok_y):
            problem = "an influence value is not finite (a row with a NaN or inf element)"
        elif not vx + vy > 0.0:
            problem = "the variance estimate is 0"
        else:
            se = math.sqrt(vx + vy)
    else:
        flat = torch.cat([pair["psi_x"], pair["psi_y"]]).cpu().numpy()                # the one read-back
        psi_x, psi_y = flat[:n], flat[n:]
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            se = frechet_standard_error(psi_x, psi_y, labels_x, labels_y)
        if caught:
            problem = str(caught[0].message).split(": ", 1)[1].rsplit(": ", 1)[0]
        if return_rows:
            out.update(candidate_influence=psi_x.copy(), reference_influence=psi_y.copy())
    if problem:
        warnings.warn(f"{what}: {problem}: the standard error and the interval are NaN", RuntimeWarning, stacklevel=2)
    else:
        half = statistics.NormalDist().inv_cdf(0.5 + 0.5 * confidence) * se
        out.update(fad_std_error=se, fad_ci_low=pair["fd"] - half, fad_ci_high=pair["fd"] + half)
    return out


def frechet_distance_compare(model_a: AudioMetricsData, model_b: AudioMetricsData, ref: AudioMetricsData, groups_a=None,
                             groups_b=None, ref_groups=None):
    """Is candidate set `model_a` closer to the reference `ref` than candidate set `model_b`?  Both Frechet distances and the
    test of their difference that accounts for the shared reference rows.  Returns {"fad_a", "fad_b", "fad_difference": fad_a
    - fad_b, "fad_difference_std_error", "fad_z", "fad_p_value": Phi(z) - small means `a` is significantly closer than `b` -,
    "fad_p_value_two_sided"}.  Labels as in frechet_distance_with_error.  Sets of unequal size carry different 1 / N biases:
    report n_a and n_b with the result.  The same object passed as both models, a solve that did not converge, a non-finite
    row or a variance of 0 give NaN for the error, z and the p-values and ONE RuntimeWarning."""
    what = "frechet_distance_compare"
    rows_a, na, labels_a = _checked_set(model_a, groups_a, what, "candidate set A")
    rows_b, nb, labels_b = _checked_set(model_b, groups_b, what, "candidate set B")
    rows_y, m, labels_y = _checked_set(ref, ref_groups, what, "its reference set")
    _same_width(what, rows_a, rows_b, rows_y)
    device = _device_of(rows_y)
    pa = _pair(model_a, rows_a, ref, rows_y, device)
    pb = pa if model_b is model_a else _pair(model_b, rows_b, ref, rows_y, device)
    out = {"fad_a": pa["fd"], "fad_b": pb["fd"], "fad_difference": pa["fd"] - pb["fd"], "fad_difference_std_error": NAN,
           "fad_z": NAN, "fad_p_value": NAN, "fad_p_value_two_sided": NAN}
    problem = None
    if model_b is model_a:
        problem = "the same set was passed as both models: the difference has no sampling distribution to test against"
    elif pa["stop"] != 1 or pb["stop"] != 1:
        problem = (f"a Newton-Schulz solve ended without converging (stop codes {pa['stop']} and {pb['stop']}): the "
                   "optimal-transport map is undefined")
    else:
        flat = torch.cat([pa["psi_x"], pb["psi_x"], pa["psi_y"], pb["psi_y"]]).cpu().numpy()      # the one read-back
        psi_a, psi_b, psi_ya, psi_yb = flat[:na], flat[na:na + nb], flat[na + nb:na + nb + m], flat[na + nb + m:]
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            t = frechet_difference_test(pa["fd"], pb["fd"], psi_a, psi_b, psi_ya, psi_yb, labels_a, labels_b, labels_y)
        if caught:
            problem = str(caught[0].message).split(": ", 1)[1].rsplit(": ", 1)[0]
        else:
            out.update(fad_difference_std_error=t["std_error"], fad_z=t["z"], fad_p_value=t["p_value"],
                       fad_p_value_two_sided=t["p_value_two_sided"])
    if problem:
        warnings.warn(f"{what}: {problem}: the standard error, z and the p-values are NaN", RuntimeWarning, stacklevel=2)
    return out
