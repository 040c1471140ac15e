"""The classifier two-sample test (C2ST; Lopez-Paz & Oquab, ICLR 2017; Friedman 2003) with a linear logistic probe: train a
classifier to tell candidate rows (s = +1) from reference rows (s = -1) and look at its accuracy on rows it has not seen.
50 % means indistinguishable, 100 % means a linear probe on the embeddings separates the two sets completely.

Rows are standardised with the POOLED statistics, x~ = (x - mu) / sigma (mu and sigma^2: the mean and the diagonal of the
covariance of the merged statistics of the two sets, ops.stats_merge; a column of zero variance gets sigma = 1).  The
standardisation is label-free, so taking it from all rows leaks no label.

Folds.  Units are the labels of `groups` / `ref_groups` (the song a window comes from), every row its own unit without them.
Per set the units, in ascending label order, are permuted with numpy.random.default_rng(seed).permutation - the candidate
set first, then the reference, from ONE generator - and the unit at position j goes to fold j % K.  Windows of one track are
near-duplicates: a probe that has seen windows of a track classifies that track's held-out windows trivially, so folds dealt
by row reject equal distributions almost every time.  PASS LABELS WHENEVER THE ROWS ARE WINDOWS OF TRACKS.

Model k is trained on the rows whose fold is not k: theta = (w, b), z = b + w . x~,
  L_k(theta) = 1/2 mean_{cand train} softplus(-z) + 1/2 mean_{ref train} softplus(z) + (l2 / 2) |theta|^2
- class-balanced, the penalty includes the intercept on purpose: L_k is then l2-strongly convex and
|theta - theta*|_2 <= |grad L_k(theta)|_2 / l2.  The K problems advance in lockstep (logistic_lbfgs): one device pass
(ops.logit_pass per set: K skinny f64 products forward, the logistic residual, K skinny products back) evaluates all K models
at their own trial points.  The host folds the standardisation into a = w / sigma and b - a . mu, maps sum r x back to
standardised coordinates and applies the class weights and the penalty: O(K D) per pass.

The out-of-fold logit of a row is z under the model of its own fold; h = 1 if its sign is right, 1/2 at z == 0, 0 otherwise.
  c2st_accuracy = 1/2 (mean h over candidate rows + mean h over reference rows), over ALL rows: descriptive.
The test uses fold 0 ONLY - the textbook C2ST.  The folds' models share training rows, so the z statistic of the accuracy
pooled over all folds has a standard deviation of 1.3 - 1.4 under H0 and rejects twice as often as its level says; the same
statistic on one held-out fold is calibrated.  With acc0 the accuracy on fold 0 and the variance taken about the NULL mean,
  v_side = sum_g (sum_{i in g, fold 0} (h_i - 1/2))^2 / n0^2,   c2st_z = (acc0 - 1/2) / sqrt((v_cand + v_ref) / 4),
  c2st_p_value = Phi(-z)    (small: the sets are distinguishable).
For independent rows v_side is exactly 1 / (4 n0), the textbook null, and it is never 0 at perfect separation."""
import math
import warnings

import numpy as np
import torch

from .. import hip_ops as ops
from ..data import AudioMetricsData, ensure_tensor
from ._groups import labelled_rows
from .fad_stats import _phi, _side_variance

NAN = float("nan")
MAX_FOLDS = ops.LOGIT_MAX_MODELS
LBFGS_MEMORY = 10
ARMIJO_C = 1e-4
MIN_STEP = 2.0 ** -40
ROUNDING_SLACK = 16.0 * 2.0 ** -52


# ------------------------------------------------------------------ host: folds
def c2st_folds(labels_or_n, folds, rng):
    """The fold of every row of ONE set (int32 numpy [n]) - host.  labels_or_n: one integer label per row (any order, any
    values; rows of one label stay together) or the number of rows (every row its own unit).  The units in ascending label
    order are permuted with rng.permutation and the unit at position j goes to fold j % folds.  Fewer units than folds
    raise ValueError."""
    folds = int(folds)
    if not 2 <= folds <= MAX_FOLDS:
        raise ValueError(f"folds={folds!r} must lie in 2..{MAX_FOLDS}")
    if isinstance(labels_or_n, torch.Tensor):
        labels_or_n = labels_or_n.cpu().numpy()
    if np.ndim(labels_or_n) == 0:
        units, inverse = int(labels_or_n), None
    else:
        labels = np.asarray(labels_or_n)
        if labels.ndim != 1 or labels.dtype.kind not in "iu":
            raise ValueError(f"labels must be a vector of integers (one per row), got {labels.dtype} {labels.shape}")
        uniq, inverse = np.unique(labels, return_inverse=True)
        units, inverse = len(uniq), inverse.reshape(-1)
    if units < folds:
        raise ValueError(f"{units} unit(s) cannot be dealt into {folds} folds: every fold needs a unit of every set")
    unit_fold = np.empty(units, dtype=np.int32)
    unit_fold[rng.permutation(units)] = np.arange(units, dtype=np.int32) % folds
    return unit_fold if inverse is None else unit_fold[inverse]


# ------------------------------------------------------------------ host: the summary of out-of-fold logits
def _softplus(t):
    return np.maximum(t, 0.0) + np.log1p(np.exp(-np.abs(t)))


def _hits(z, sign):
    t = sign * z
    return np.where(t > 0.0, 1.0, np.where(t == 0.0, 0.5, 0.0))


def _side(z, fold, groups, name):
    z = np.asarray(z, dtype=np.float64)
    fold = np.asarray(fold)
    if z.ndim != 1 or fold.shape != z.shape:
        raise ValueError(f"{name}: one logit and one fold per row (got shapes {z.shape} and {fold.shape})")
    if groups is None:
        labels = np.arange(len(z))
    else:
        labels = np.asarray(groups.cpu() if isinstance(groups, torch.Tensor) else groups)
        if labels.shape != z.shape or labels.dtype.kind not in "iu":
            raise ValueError(f"{name}: one integer label per row (got {labels.dtype} {labels.shape} for {len(z)} rows)")
    keep = np.isfinite(z) & (fold >= 0)
    return z[keep], fold[keep], labels[keep], groups is None


def _unit_sums(values, labels):
    _, inverse = np.unique(labels, return_inverse=True)
    return np.bincount(inverse.reshape(-1), weights=values)


def _pair_count(zc, zr):
    """#{z_c > z_r} + 1/2 #{z_c == z_r} from midranks: a multiple of 1/2, exact in float64"""
    both = np.concatenate([zc, zr])
    _, inverse, counts = np.unique(both, return_inverse=True, return_counts=True)
    midrank = np.cumsum(counts) - (counts - 1) / 2.0
    return float(midrank[inverse.reshape(-1)[:len(zc)]].sum()) - len(zc) * (len(zc) + 1) / 2.0


def c2st_summary(z_cand, z_ref, fold_cand, fold_ref, groups=None, ref_groups=None):
    """The figures of the classifier two-sample test from the out-of-fold logits of the candidate rows (z_cand, s = +1) and
    the reference rows (z_ref, s = -1) and their folds - host arithmetic, float64 numpy, no GPU.  A row whose logit is not
    finite or whose fold is negative takes part in nothing.  groups / ref_groups: one integer label per row - the labelled
    units replace the rows as sampling units of that side.  Returns {"c2st_accuracy", "c2st_std_error" (cluster-robust,
    about the accuracy's own mean), "c2st_log_loss", "c2st_auc" (per fold, midrank ties, folds weighted by candidate rows x
    reference rows), "c2st_accuracy_holdout", "c2st_holdout_rows": (candidate, reference) rows of fold 0, "c2st_z",
    "c2st_p_value" = Phi(-z): the test on fold 0 alone, its variance taken about the null mean 1/2}.  A side without rows (or
    without rows in fold 0) gives NaN for what needs it."""
    zc, fc, lc, _ = _side(z_cand, fold_cand, groups, "candidate")
    zr, fr, lr, _ = _side(z_ref, fold_ref, ref_groups, "reference")
    hc, hr = _hits(zc, 1.0), _hits(zr, -1.0)
    out = {"c2st_accuracy": NAN, "c2st_std_error": NAN, "c2st_log_loss": NAN, "c2st_auc": NAN, "c2st_accuracy_holdout": NAN,
           "c2st_holdout_rows": (int((fc == 0).sum()), int((fr == 0).sum())), "c2st_z": NAN, "c2st_p_value": NAN}
    if len(zc) and len(zr):
        out["c2st_accuracy"] = 0.5 * (float(hc.sum()) / len(hc) + float(hr.sum()) / len(hr))
        out["c2st_log_loss"] = 0.5 * (float(_softplus(-zc).sum()) / len(zc) + float(_softplus(zr).sum()) / len(zr))
        var = 0.0
        for h, labels in ((hc, lc), (hr, lr)):
            _, inverse = np.unique(labels, return_inverse=True)
            units = int(inverse.max()) + 1
            var += _side_variance(h - h.mean(), inverse.reshape(-1), units) if units > 1 else NAN
        out["c2st_std_error"] = math.sqrt(0.25 * var) if var >= 0.0 else NAN
        pairs, weight = 0.0, 0
        for k in np.union1d(fc, fr):
            a, b = zc[fc == k], zr[fr == k]
            if len(a) and len(b):
                pairs += _pair_count(a, b)
                weight += len(a) * len(b)
        out["c2st_auc"] = pairs / weight if weight else NAN
    n0c, n0r = out["c2st_holdout_rows"]
    if n0c and n0r:
        dc, dr = hc[fc == 0] - 0.5, hr[fr == 0] - 0.5
        acc0 = 0.5 * (float((dc + 0.5).sum()) / n0c + float((dr + 0.5).sum()) / n0r)
        sc, sr = _unit_sums(dc, lc[fc == 0]), _unit_sums(dr, lr[fr == 0])
        v = float(np.sum(sc * sc)) / (n0c * n0c) + float(np.sum(sr * sr)) / (n0r * n0r)
        # v == 0 needs every unit's hits and misses to cancel, and then acc0 is exactly 1/2: z = 0
        z = (acc0 - 0.5) / math.sqrt(0.25 * v) if v > 0.0 else 0.0
        out.update(c2st_accuracy_holdout=acc0, c2st_z=z, c2st_p_value=_phi(-z))
    return out


# ------------------------------------------------------------------ host: K L-BFGS problems in lockstep
def _two_loop(g, hist, precondition):
    """-H g with the L-BFGS inverse Hessian of the stored pairs around the initial inverse Hessian `precondition`"""
    q = g.copy()
    alphas = []
    for s, y, rho in reversed(hist):
        a = rho * float(s @ q)
        alphas.append(a)
        q -= a * y
    q = precondition(q)
    for (s, y, rho), a in zip(hist, reversed(alphas)):
        q += (a - rho * float(y @ q)) * s
    return -q


def logistic_lbfgs(evaluate, K, P, precondition=None, tol=1e-8, max_passes=500):
    """Minimise K smooth convex functions of P parameters each, in lockstep - host numpy around evaluate(theta [K, P]) ->
    (loss [K], grad [K, P]), which evaluates every model at its own point in ONE pass.  L-BFGS with a memory of 10 pairs;
    `precondition` applies the initial inverse Hessian to a vector [P] (None: the identity); Armijo backtracking (c = 1e-4,
    halving, with 16 ulps of the loss as slack; a trial whose gradient norm is already <= tol is taken as well); start at 0.  A model stops when |grad|_2 <=
    tol and then keeps its point: its trial point in later passes is that point.  Returns {"theta" [K, P], "loss" [K],
    "gradient_norm" [K], "converged" bool [K], "passes": calls of evaluate}; after max_passes the best accepted points are
    returned with converged False where the rule was not met."""
    K, P, max_passes = int(K), int(P), int(max_passes)
    if max_passes < 1:
        raise ValueError(f"max_passes={max_passes!r} must be at least 1")
    if precondition is None:
        precondition = lambda v: v                                       # noqa: E731
    x = np.zeros((K, P))
    f, g = (np.array(t, dtype=np.float64) for t in evaluate(x.copy()))
    passes = 1
    norm = np.linalg.norm(g, axis=1)
    done = norm <= tol
    stuck = np.zeros(K, dtype=bool)
    hist = [[] for _ in range(K)]
    direction = np.zeros((K, P))
    step = np.ones(K)
    for k in range(K):
        if not done[k]:
            direction[k] = _two_loop(g[k], hist[k], precondition)
    while passes < max_passes and not (done | stuck).all():
        active = ~(done | stuck)
        trial = x.copy()
        trial[active] += step[active, None] * direction[active]
        ft, gt = (np.array(t, dtype=np.float64) for t in evaluate(trial.copy()))
        passes += 1
        for k in np.flatnonzero(active):
            slope = float(g[k] @ direction[k])
            trial_norm = float(np.linalg.norm(gt[k]))
            # near the optimum the decrease falls below the rounding of the loss itself: a few ulps of slack keep the
            # quasi-Newton steps coming, and the stop rule is on the gradient
            slack = ROUNDING_SLACK * abs(f[k])
            if np.isfinite(ft[k]) and (ft[k] <= f[k] + ARMIJO_C * step[k] * slope + slack or trial_norm <= tol):
                s, y = trial[k] - x[k], gt[k] - g[k]
                sy = float(s @ y)
                if sy > 1e-12 * float(np.linalg.norm(s) * np.linalg.norm(y)):
                    hist[k].append((s, y, 1.0 / sy))
                    del hist[k][:-LBFGS_MEMORY]
                x[k], f[k], g[k], norm[k] = trial[k], ft[k], gt[k], trial_norm
                done[k] = trial_norm <= tol
                if not done[k]:
                    direction[k] = _two_loop(g[k], hist[k], precondition)
                    if float(g[k] @ direction[k]) >= 0.0:                # not a descent direction: start the memory again
                        hist[k].clear()
                        direction[k] = -precondition(g[k])
                    step[k] = 1.0
            else:
                step[k] *= 0.5
                if step[k] < MIN_STEP:
                    if hist[k]:                                          # retry from the preconditioned gradient
                        hist[k].clear()
                        direction[k] = -precondition(g[k])
                        step[k] = 1.0
                    else:
                        stuck[k] = True                                  # the loss no longer resolves a decrease
    return {"theta": x, "loss": f, "gradient_norm": norm, "converged": done.copy(), "passes": passes}


# ------------------------------------------------------------------ the device side
def _rows_and_labels(data, groups, what, name):
    if groups is not None:
        rows, n, labels = labelled_rows(data, groups, what, f"its {name} set")
        labels = np.asarray(labels.cpu())
    else:
        rows, labels = getattr(data, "embeddings", None), None
        n = int(rows.shape[0]) if rows is not None else 0
        if rows is None or n == 0:
            raise ValueError(f"{what} scores the stored rows of its {name} set, which keeps none "
                             f"(store_embeddings={getattr(data, 'store_embeddings', None)})")
    if getattr(data, "n", None) is None or int(data.n) != n:
        raise ValueError(f"{what}: its {name} set stores {n} rows but its statistics describe {getattr(data, 'n', None)}: the "
                         "standardisation belongs to the rows the mean and covariance were taken from")
    return rows, n, labels


def _device_of(rows):
    if rows.is_cuda:
        return rows.device
    from ..data import default_device
    return torch.device(default_device())


def pooled_standardisation(cand, ref, rows_x=None, rows_y=None, device=None):
    """(mu [D], sigma [D], correlation [D, D]) of the pooled rows as float64 numpy: the mean, the square root of the diagonal
    (1 where it is not positive) and the correlation matrix of the merged statistics of the two sets (ops.stats_merge), one
    read-back.  Where the stored statistics are not finite (a row with a NaN or inf element went into them) the mean and
    the covariance are taken again from the rows without such an element - a rare path, in float64 torch."""
    rows_x = cand.embeddings if rows_x is None else rows_x
    rows_y = ref.embeddings if rows_y is None else rows_y
    device = _device_of(rows_x) if device is None else device
    mx, cx, my, cy = (ensure_tensor(t).to(device, torch.float64) for t in (cand.mean, cand.cov, ref.mean, ref.cov))
    mean, cov = ops.stats_merge(int(cand.n), mx.reshape(-1), cx, int(ref.n), my.reshape(-1), cy)
    flat = torch.cat([mean.reshape(-1), cov.reshape(-1)]).cpu().numpy()
    if not np.isfinite(flat).all():
        both = torch.cat([rows_x.to(device, torch.float64), rows_y.to(device, torch.float64)])
        both = both[torch.isfinite(both).all(dim=1)]
        mean = both.mean(dim=0)
        cov = torch.cov(both.T).reshape(mean.numel(), mean.numel()) if both.shape[0] > 1 else torch.zeros_like(cov)
        flat = torch.cat([mean.reshape(-1), cov.reshape(-1)]).cpu().numpy()
    d = int(mean.numel())
    mu, cov = flat[:d].copy(), flat[d:].reshape(d, d)
    var = np.diag(cov).copy()
    sigma = np.where(var > 0.0, np.sqrt(np.where(var > 0.0, var, 1.0)), 1.0)
    corr = np.where((var > 0.0)[:, None] & (var > 0.0)[None, :], cov / np.outer(sigma, sigma), 0.0)
    return mu, sigma, corr


def classifier_two_sample_test(cand: AudioMetricsData, ref: AudioMetricsData, groups=None, ref_groups=None, folds=5, l2=1e-3, seed=0,
                               tol=1e-8, max_passes=500, return_rows=False):
    """Can a linear probe on the embeddings tell candidate set `cand` from reference set `ref`?  K = `folds` L2-regularised
    logistic models, each trained on the rows outside its fold (one fused device pass per set and evaluation), the
    out-of-fold logit of every row, and the classifier two-sample test on fold 0 (see the module text for every definition).

    groups / ref_groups: one integer label per stored row (the song a window comes from; any order, any values) - folds are
    dealt by label and the variances take the labelled units as sampling units.  PASS THEM WHENEVER THE ROWS ARE WINDOWS OF
    TRACKS.  Fewer than `folds` units on a side raise ValueError.  Both sets hold float32 rows or both float64 rows (all
    arithmetic is float64 either way); a mixed pair raises NotImplementedError before any device call.

    Returns {"c2st_accuracy", "c2st_std_error", "c2st_log_loss", "c2st_auc": cross-fitted over ALL rows, descriptive;
    "c2st_accuracy_holdout", "c2st_holdout_rows", "c2st_z", "c2st_p_value": the test, on fold 0 alone - a small p says the sets
    are distinguishable; "c2st_passes": device passes of the optimiser (the out-of-fold logits take one more),
    "c2st_converged" bool [K], "c2st_gradient_norm" [K], "c2st_rows_nonfinite"}.  return_rows=True adds
    "c2st_candidate_logit" [n], "c2st_reference_logit" [m] (float64, stored row order), "c2st_candidate_fold",
    "c2st_reference_fold" (int32; -1 for a row that takes no part), "c2st_weights" [K, D] and "c2st_intercepts" [K] in the coordinates of the ROWS: z =
    intercept + weights . x.  A model that has not reached |grad L_k|_2 <= tol after max_passes gives ONE RuntimeWarning; the
    values are still returned.  A row with a NaN or inf element takes part in nothing: its logit is NaN, it is counted in
    c2st_rows_nonfinite and ONE RuntimeWarning names the count."""
    what = "classifier_two_sample_test"
    K = int(folds)
    if K != folds or not 2 <= K <= MAX_FOLDS:
        raise ValueError(f"folds={folds!r} must be an integer in 2..{MAX_FOLDS}")
    l2, tol = float(l2), float(tol)
    if not (l2 > 0.0 and math.isfinite(l2)):
        raise ValueError(f"l2={l2!r} must be positive: the penalty is what makes every model's optimum unique")
    if not tol > 0.0:
        raise ValueError(f"tol={tol!r} must be positive")
    if int(max_passes) < 1:
        raise ValueError(f"max_passes={max_passes!r} must be at least 1")
    rows_x, n, labels_x = _rows_and_labels(cand, groups, what, "candidate")
    rows_y, m, labels_y = _rows_and_labels(ref, ref_groups, what, "reference")
    for rows, name, other in ((rows_x, "candidate", rows_y), (rows_y, "reference", rows_x)):
        if rows.dtype not in (torch.float32, torch.float64) or rows.dtype != other.dtype:
            raise NotImplementedError(f"{what}: the {name} set holds {rows.dtype} rows and the other set {other.dtype} rows; both "
                                      "sets must hold float32 rows or both float64 rows (a mixed pair is not implemented)")
    if rows_x.shape[1] != rows_y.shape[1]:
        raise ValueError(f"{what}: feature widths differ: {rows_x.shape[1]} and {rows_y.shape[1]}")
    D = int(rows_x.shape[1])
    rng = np.random.default_rng(seed)
    fold_x = c2st_folds(n if labels_x is None else labels_x, K, rng)
    fold_y = c2st_folds(m if labels_y is None else labels_y, K, rng)

    device = _device_of(rows_x)
    rows_x, rows_y = ops.as_rows(rows_x.to(device)), ops.as_rows(rows_y.to(device))
    mu, sigma, corr = pooled_standardisation(cand, ref, rows_x, rows_y, device)
    # the initial inverse Hessian (M / 4 + l2 I)^-1, M = blockdiag(pooled correlation matrix, 1): one D x D factorisation
    evals, evecs = np.linalg.eigh(corr)
    scale = 1.0 / (np.maximum(evals, 0.0) / 4.0 + l2)

    def precondition(v):
        out = np.empty_like(v)
        out[:D] = evecs @ (scale * (evecs.T @ v[:D]))
        out[D] = v[D] / (0.25 + l2)
        return out

    sides = [{"rows": rows_x, "fold": fold_x.copy(), "label": 1}, {"rows": rows_y, "fold": fold_y.copy(), "label": 0}]
    state = {"nonfinite": None}

    def upload_folds():
        for s in sides:
            s["fold_dev"] = ops.upload_host_array(s["fold"].astype(np.int32), device)
            # training rows of model k: the rows that take part and are not in fold k
            s["train"] = float((s["fold"] >= 0).sum()) - np.bincount(s["fold"][s["fold"] >= 0], minlength=K)[:K].astype(np.float64)
            if (s["train"] < 1.0).any():
                raise ValueError(f"{what}: a model is left without training rows of a set once the rows with a non-finite "
                                 "element are set aside")

    def device_pass(theta, want_z):
        a = theta[:, :D] / sigma
        coef = ops.upload_host_array(np.concatenate([a, (theta[:, D] - a @ mu)[:, None]], axis=1), device)
        got = [ops.logit_pass(s["rows"], s["fold_dev"], s["label"], coef, want_z=want_z) for s in sides]
        flat = torch.cat([t.reshape(-1) for sums, _, counts in got for t in (sums, counts)]).cpu().numpy()      # the one read-back
        size = K * (D + 2) + 2
        parts = [flat[i * size:(i + 1) * size] for i in range(2)]
        return [p[:-2].reshape(K, D + 2) for p in parts], [p[-2:] for p in parts], [z for _, z, _ in got]

    def evaluate(theta):
        sums, counts, zs = device_pass(theta, state["nonfinite"] is None)
        if state["nonfinite"] is None:                                    # the first pass finds the rows that take no part
            state["nonfinite"] = int(counts[0][1] + counts[1][1])
            if state["nonfinite"]:
                for s, z in zip(sides, zs):
                    s["fold"][np.isnan(z.cpu().numpy())] = -1
                upload_folds()
        loss = 0.5 * l2 * np.sum(theta * theta, axis=1)
        grad = l2 * theta
        for s, t in zip(sides, sums):
            weight = 0.5 / s["train"]
            grad[:, :D] += weight[:, None] * (t[:, :D] - t[:, D:D + 1] * mu[None, :]) / sigma[None, :]
            grad[:, D] += weight * t[:, D]
            loss += weight * t[:, D + 1]
        return loss, grad

    upload_folds()
    fit = logistic_lbfgs(evaluate, K, D + 1, precondition, tol, max_passes)
    theta = fit["theta"]
    _, _, zs = device_pass(theta, True)
    flat = torch.cat(zs).cpu().numpy()
    z_x, z_y = flat[:n].copy(), flat[n:].copy()
    out = c2st_summary(z_x, z_y, sides[0]["fold"], sides[1]["fold"], labels_x, labels_y)
    out.update(c2st_passes=fit["passes"], c2st_converged=fit["converged"], c2st_gradient_norm=fit["gradient_norm"],
               c2st_rows_nonfinite=state["nonfinite"])
    if return_rows:
        a = theta[:, :D] / sigma
        out.update(c2st_candidate_logit=z_x, c2st_reference_logit=z_y, c2st_candidate_fold=sides[0]["fold"], c2st_reference_fold=sides[1]["fold"],
                   c2st_weights=a, c2st_intercepts=theta[:, D] - a @ mu)
    if state["nonfinite"]:
        warnings.warn(f"{what}: {state['nonfinite']} row(s) hold a NaN or inf element and take part in nothing: their logits are "
                      "NaN", RuntimeWarning, stacklevel=2)
    if not fit["converged"].all():
        warnings.warn(f"{what}: {int((~fit['converged']).sum())} of {K} models have not reached |grad|_2 <= {tol:g} after "
                      f"{fit['passes']} passes (largest gradient norm {float(fit['gradient_norm'].max()):.3g}); the values are "
                      "returned as they stand", RuntimeWarning, stacklevel=2)
    return out
