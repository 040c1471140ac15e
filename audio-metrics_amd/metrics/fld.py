"""Feature likelihood divergence (Jiralerspong, Bose, Gemp, Qin, Bachrach, Gidel, NeurIPS 2023: "Feature Likelihood
Divergence: Evaluating the Generalization of Generative Models Using Samples") and the authenticity score (Alaa, van
Breugel, Saveliev, van der Schaar, ICML 2022).  Every other distance of this package compares two sets and rewards a model
that replays its training clips; these two take the TRAINING set as well and say whether the generated rows are copies of
it.  The reference has no such functions.  This module restates the paper's construction with the conventions below; it
does not claim agreement with the paper's published numbers (no package of the authors was at hand to compare with).

  sets       gen (M stored rows: the centres g_j), train (N rows), test (T held-out rows); float32, D columns
  normalize  "train" (default): every set is mapped by (row - mean_train) / std_train / sqrt(D), the per-dimension mean and
             unbiased standard deviation of the training set's stored statistics (mean, diag(cov)); a zero standard deviation
             counts as 1.  In f64 with torch ops, rounded to float32 once.  None: the rows as they are.  Centring matters for
             the arithmetic: the f32 d2 loses 2^-24 (D + 16) (|x|^2 + |g|^2), which 1 / (2 sigma^2) multiplies
  mixture    an isotropic Gaussian N(g_j, sigma_j^2 I) on every generated row, weight 1 / M, theta_j = log sigma_j^2 (f64):
             l(x) = logsumexp_j (-h_j d2(x, g_j) - c_j) - log M - (D / 2) log 2 pi,  h_j = 0.5 exp(-theta_j), c_j = (D / 2) theta_j,
             d2 = max(fmaf(-2, <x, g>, |x|^2 + |g|^2), 0) in f32: the bits of knn_search(squared=True)      ops.fld_loglik
  fit        L(theta) = -mean of l over the training rows; full-batch Adam from theta = 0 with lr 0.5, beta (0.9, 0.999),
             eps 1e-8 and bias correction, a fixed number of steps (100), theta clamped to [min_log_variance, 30] after every
             step.  Deterministic: no minibatch, no seed, no shuffle (the paper draws minibatches).  A step is two tile sweeps
             (ops.fld_loglik, ops.fld_grad_step) and reads nothing back; the losses of all steps come back in one read.
             min_log_variance = -10 is a convention of this build: it bounds by how much a centre that sits on a training
             row can amplify the f32 distance error (h <= 1.1e4)
  outputs    per dimension: fld_nll_train = -mean l(train) / D, fld_nll_test = -mean l(test) / D, their difference
             fld_generalization_gap, and fld = 100 (fld_nll_test - baseline_nll); the paper's dataset constant is the caller's
  overfit    o_j = h_j (min_i d2(test_i, g_j) - min_i d2(train_i, g_j)): the centre's best log-density on a training row minus
             its best on a test row; a centre that copies a training clip shrinks its variance onto it and stands out.
             fld_overfit_fraction, the share of centres with o_j > 0, is biased towards 1 when N > T (the nearest of more
             rows is nearer): use held-out and training sets of equal size
  non-finite a row with a NaN or an infinity has l = -inf, is left out of every mean and counted; a centre with one contributes
             0 everywhere, keeps theta = 0 and is counted; one RuntimeWarning names the counts"""
import math
import warnings

import numpy as np
import torch

from .. import hip_ops as ops
from .prdc_groups import grouped_authenticity

_ADAM_B1, _ADAM_B2, _ADAM_EPS = 0.9, 0.999, 1e-8


def fld_adam_step(theta, grad, m, v, step, lr, theta_min):
    """The update of the fit on the host, numpy float64: (theta, m, v) after Adam step `step` (the first is 1) with
    beta = (0.9, 0.999), eps = 1e-8 and bias correction, theta clamped to [theta_min, 30].  The device's merge kernel
    performs these operations in this order, each rounded once."""
    theta, grad, m, v = (np.asarray(a, dtype=np.float64) for a in (theta, grad, m, v))
    step = int(step)
    if step < 1:
        raise ValueError(f"step={step} must be at least 1")
    m = _ADAM_B1 * m + (1.0 - _ADAM_B1) * grad
    v = _ADAM_B2 * v + (1.0 - _ADAM_B2) * (grad * grad)
    mhat, vhat = m / (1.0 - _ADAM_B1 ** step), v / (1.0 - _ADAM_B2 ** step)
    theta = theta - float(lr) * (mhat / (np.sqrt(vhat) + _ADAM_EPS))
    return np.minimum(np.maximum(theta, float(theta_min)), ops.FLD_THETA_MAX), m, v


def fld_gradient(theta, a, b, d, n_finite):
    """dL/dtheta from the two sums of the gradient sweep, numpy float64: -(h B - (D / 2) A) / n_finite, h = 0.5 exp(-theta);
    zeros when no row has a finite log-likelihood."""
    theta, a, b = (np.asarray(t, dtype=np.float64) for t in (theta, a, b))
    if not float(n_finite) > 0.0:
        return np.zeros_like(theta)
    return -(((0.5 * np.exp(-theta)) * b - (0.5 * int(d)) * a) / float(n_finite))


def _numbers(sum_train, n_train, sum_test, n_test, d, baseline_nll):
    nll_train = -(sum_train / n_train) / d if n_train > 0 else math.nan
    nll_test = -(sum_test / n_test) / d if n_test > 0 else math.nan
    return {"fld": 100.0 * (nll_test - baseline_nll), "fld_nll_test": nll_test, "fld_nll_train": nll_train,
            "fld_generalization_gap": nll_test - nll_train, "fld_baseline_nll": baseline_nll}


def fld_from_logliks(train_loglik, test_loglik, D, baseline_nll=0.0):
    """The scalars of the divergence from per-row log-likelihoods, host arithmetic in numpy float64: rows with a
    non-finite value are left out of the means.  {"fld", "fld_nll_test", "fld_nll_train", "fld_generalization_gap",
    "fld_baseline_nll"}, the likelihoods per dimension."""
    d = int(D)
    if d < 1:
        raise ValueError(f"D={D!r} must be at least 1")
    baseline_nll = float(baseline_nll)
    if not math.isfinite(baseline_nll):
        raise ValueError(f"baseline_nll={baseline_nll!r} must be finite")
    tr, te = np.asarray(train_loglik, dtype=np.float64).ravel(), np.asarray(test_loglik, dtype=np.float64).ravel()
    tr, te = tr[np.isfinite(tr)], te[np.isfinite(te)]
    return _numbers(float(tr.sum()), tr.size, float(te.sum()), te.size, d, baseline_nll)


def _rows_of(data, name, what):
    rows = getattr(data, "embeddings", None)
    if rows is None or rows.shape[0] == 0:
        raise ValueError(f"{what} needs the stored rows of its {name} set, which keeps none "
                         f"(store_embeddings={getattr(data, 'store_embeddings', None)})")
    if rows.dtype == torch.float64:
        raise NotImplementedError(f"{what}: the {name} set holds float64 rows; the tile sweeps take float32 rows "
                                  "(the float64 matrix-core form is not implemented)")
    return rows


def _check_fit_arguments(steps, lr, min_log_variance, normalize):
    steps = int(steps)
    if steps < 1:
        raise ValueError(f"steps={steps} must be at least 1")
    lr, min_log_variance = float(lr), float(min_log_variance)
    if not math.isfinite(lr) or lr < 0.0:
        raise ValueError(f"lr={lr!r} must be finite and not negative")
    if not math.isfinite(min_log_variance):
        raise ValueError(f"min_log_variance={min_log_variance!r} must be finite")
    if not ops.FLD_THETA_MIN_LIMIT <= min_log_variance <= ops.FLD_THETA_MAX:
        raise ValueError(f"min_log_variance={min_log_variance!r} must lie in [{ops.FLD_THETA_MIN_LIMIT:.4f}, {ops.FLD_THETA_MAX}]: "
                         "0.5 exp(-theta) has to stay a normal float32 number")
    if normalize not in ("train", None):
        raise ValueError(f"normalize={normalize!r} must be 'train' or None")
    return steps, lr, min_log_variance


def fld_normalization(train):
    """(mean, std) of the default normalisation, float64 device vectors [D]: the training set's stored mean and the square
    root of the diagonal of its stored (unbiased) covariance, a standard deviation that is not > 0 replaced by 1."""
    d = train.embeddings.shape[1]
    mean = train.mean.to(torch.float64).reshape(-1)
    cov = train.cov
    var = torch.diagonal(cov).to(torch.float64) if tuple(cov.shape) == (d, d) else torch.zeros(d, dtype=torch.float64, device=mean.device)
    std = torch.sqrt(var)
    return mean, torch.where(std > 0.0, std, torch.ones_like(std))


def _scaled(rows, mean, std):
    d = rows.shape[1]
    return ops.as_matrix(((rows.to(torch.float64) - mean) / std / math.sqrt(d)).to(torch.float32))


def _prepare(sets, train, normalize, what):
    """The float32 matrices the sweeps read: [rows of every (data, name) in `sets`], normalised once."""
    rows = [_rows_of(data, name, what) for data, name in sets]
    widths = {r.shape[1] for r in rows}
    if len(widths) != 1:
        raise ValueError(f"feature widths differ: {', '.join(str(r.shape[1]) for r in rows)}")
    if normalize is None:
        return [ops.as_matrix(r) for r in rows]
    mean, std = fld_normalization(train)
    return [_scaled(r, mean, std) for r in rows]


def _fit(g, x, steps, lr, theta_min):
    """(theta, loglik of the rows of x at theta, history [steps + 1, 3]) - device tensors, nothing read back."""
    rows = g.shape[0]
    theta, m, v = (torch.zeros(rows, dtype=torch.float64, device=g.device) for _ in range(3))
    history = torch.empty((steps + 1, 3), dtype=torch.float64, device=g.device)
    for step in range(steps):
        ll, _ = ops.fld_loglik(x, g, theta, stats=history[step])
        theta, m, v, _, _ = ops.fld_grad_step(g, x, theta, ll, history[step, 1:2], m, v, step + 1, lr, theta_min)
    ll, _ = ops.fld_loglik(x, g, theta, stats=history[steps])
    return theta, ll, history


def _bad_centres(g):
    return (~torch.isfinite(g).all(dim=1)).sum().to(torch.float64).reshape(1)


def _warn(what, counts):
    named = [f"{n} {name}" for name, n in counts if n]
    if named:
        warnings.warn(f"{what}: non-finite elements in {', '.join(named)}: such rows are left out of every mean, such centres "
                      "contribute 0 and keep theta = 0", RuntimeWarning, stacklevel=3)


def _history_nll(history, d):
    with np.errstate(invalid="ignore", divide="ignore"):
        return -(history[:, 0] / history[:, 1]) / d


def feature_likelihood_fit(gen, train, steps=100, lr=0.5, min_log_variance=-10.0, normalize="train"):
    """Fit the per-centre log-variances of the mixture on the stored rows of `gen` to the stored rows of `train`.  Returns
    {"fld_log_variances": float64 device tensor [M] in stored row order of gen, "fld_nll_train": the per-dimension negative
    log-likelihood of the training rows after the fit, "fld_nll_train_history": numpy [steps + 1], the same before every step
    and after the last (not monotone: Adam at lr 0.5 oscillates), "fld_steps", "fld_rows_nonfinite": training rows left out,
    "fld_centres_nonfinite"}; one read-back."""
    steps, lr, theta_min = _check_fit_arguments(steps, lr, min_log_variance, normalize)
    g, x = _prepare(((gen, "generated"), (train, "training")), train, normalize, "feature_likelihood_fit")
    theta, _, history = _fit(g, x, steps, lr, theta_min)
    host = torch.cat([history.reshape(-1), _bad_centres(g)]).cpu().numpy()
    history, bad_centres = host[:-1].reshape(steps + 1, 3), int(host[-1])
    _warn("feature_likelihood_fit", (("training rows", int(history[-1, 2])), ("generated rows", bad_centres)))
    nll = _history_nll(history, x.shape[1])
    return {"fld_log_variances": theta, "fld_nll_train": float(nll[-1]), "fld_nll_train_history": nll, "fld_steps": steps,
            "fld_rows_nonfinite": int(history[-1, 2]), "fld_centres_nonfinite": bad_centres}


def feature_likelihood_divergence(gen, train, test, steps=100, lr=0.5, min_log_variance=-10.0, normalize="train", baseline_nll=0.0,
                                  return_rows=False):
    """The feature likelihood divergence of the stored rows of `gen` (the model's samples) given the `train` rows the model
    saw and held-out `test` rows.  Returns {"fld": 100 (fld_nll_test - baseline_nll), "fld_nll_test", "fld_nll_train",
    "fld_generalization_gap": test minus train, "fld_overfit_fraction": share of centres with a positive overfit score,
    "fld_baseline_nll", "fld_steps", "fld_rows_nonfinite": (training, test, generated) rows with non-finite elements};
    return_rows=True adds "fld_log_variances" [M], "fld_overfit_score" [M], "fld_nearest_train" [M] (int64: the stored
    training row nearest to each generated row, -1 where there is none), "fld_train_loglik" [N] and "fld_test_loglik" [T] as
    numpy arrays in stored row order.  Lower fld is better; a generator that returns its training set gets a low
    fld_nll_train, a large gap and an overfit fraction near 1.  The overfit fraction is biased towards 1 when the training
    set is larger than the test set: use sets of equal size.  One read-back."""
    steps, lr, theta_min = _check_fit_arguments(steps, lr, min_log_variance, normalize)
    baseline_nll = float(baseline_nll)
    if not math.isfinite(baseline_nll):
        raise ValueError(f"baseline_nll={baseline_nll!r} must be finite")
    g, x, t = _prepare(((gen, "generated"), (train, "training"), (test, "test")), train, normalize, "feature_likelihood_divergence")
    theta, ll_train, history = _fit(g, x, steps, lr, theta_min)
    ll_test, stats_test = ops.fld_loglik(t, g, theta)
    d2_train, nearest = ops.knn_search(g, x, 1, squared=True)
    d2_test, _ = ops.knn_search(g, t, 1, squared=True)
    score = 0.5 * torch.exp(-theta) * (d2_test[:, 0].to(torch.float64) - d2_train[:, 0].to(torch.float64))
    score = torch.where(torch.isnan(score), torch.zeros_like(score), score)       # a centre with no finite distance on either side
    frac = (score > 0.0).to(torch.float64).mean().reshape(1)
    rows, n, nt = g.shape[0], x.shape[0], t.shape[0]
    parts = [history[steps], stats_test, frac, _bad_centres(g)]
    if return_rows:
        parts += [theta, score, nearest[:, 0].to(torch.float64), ll_train, ll_test]
    host = torch.cat(parts).cpu().numpy()                          # the one read-back (indices below 2^53 are exact in f64)
    st_train, st_test, frac, bad_centres = host[0:3], host[3:6], float(host[6]), int(host[7])
    _warn("feature_likelihood_divergence", (("training rows", int(st_train[2])), ("test rows", int(st_test[2])),
                                            ("generated rows", bad_centres)))
    out = _numbers(float(st_train[0]), st_train[1], float(st_test[0]), st_test[1], x.shape[1], baseline_nll)
    out.update({"fld_overfit_fraction": frac, "fld_steps": steps, "fld_rows_nonfinite": (int(st_train[2]), int(st_test[2]), bad_centres)})
    if return_rows:
        cuts = np.cumsum([8, rows, rows, rows, n, nt])
        out["fld_log_variances"] = host[cuts[0]:cuts[1]].copy()
        out["fld_overfit_score"] = host[cuts[1]:cuts[2]].copy()
        out["fld_nearest_train"] = host[cuts[2]:cuts[3]].astype(np.int64)
        out["fld_train_loglik"] = host[cuts[3]:cuts[4]].copy()
        out["fld_test_loglik"] = host[cuts[4]:cuts[5]].copy()
    return out


def authenticity_score(gen, train, return_rows=False, train_groups=None, groups=None):
    """The share of generated rows that are not closer to a training row than that row's own nearest training neighbour
    (Alaa et al. 2022): row j of `gen` is authentic when |g_j - x_i| > |x_i - x_i'|, x_i the training row nearest to g_j
    (ops.knn_search(gen, train, 1)) and x_i' the training row nearest to x_i other than itself (train.get_radii(1): the second
    smallest distance of a row to its own set, a duplicate of the row counting as another row at distance 0).  The rows are
    taken as they are, float32 distances, a strict comparison; a generated row with no finite distance is not authentic.
    Returns {"authenticity": fraction}; return_rows=True adds "authentic" (numpy bool [M]) and "authenticity_nearest_train"
    (int64 [M], -1 where there is none) in stored row order of gen.  One read-back.

    train_groups / groups: one integer label per stored row of train / of gen (the song a window was cut from).  With
    train_groups a training row's own-set neighbour distance is its distance to the nearest training row WITH ANOTHER LABEL
    (metrics/prdc_groups.py: leave_group_out_radii(train, train_groups, 1)) - a sibling window of its own song is no
    neighbour; with groups as well the nearest training row of a generated row is searched among the other labels, compared
    by value (ops.knn_search_groups).  Without the two keywords this is the path above, unchanged."""
    g, x = _rows_of(gen, "generated", "authenticity_score"), _rows_of(train, "training", "authenticity_score")
    if g.shape[1] != x.shape[1]:
        raise ValueError(f"feature widths differ: {g.shape[1]} and {x.shape[1]}")
    if train_groups is not None or groups is not None:
        dist0, idx0, radii = grouped_authenticity("authenticity_score", g, gen, x, train, train_groups, groups)
    else:
        dist, idx = ops.knn_search(g, x, 1)
        dist0, idx0, radii = dist[:, 0], idx[:, 0], train.get_radii(1)
    found = idx0 >= 0
    authentic = found & (dist0 > radii[idx0.clamp(min=0)])
    if not return_rows:
        return {"authenticity": float(authentic.to(torch.float64).mean())}
    host = torch.stack([authentic.to(torch.int64), idx0]).cpu().numpy()
    return {"authenticity": float(host[0].mean()), "authentic": host[0].astype(bool), "authenticity_nearest_train": host[1].copy()}
