"""Float64 numpy oracle of the classifier two-sample test: the fused pass of csrc/logit.hip with math.fsum, a Newton solve of
every fold's regularised logistic loss to |grad|_2 <= 1e-13, and the summary formulas written out directly (pair counts for
the AUC, loops over the units for the variances).  Nothing here imports the package."""
import math

import numpy as np

U = 2.0 ** -53


# ------------------------------------------------------------------ data
def law(rng, d, spread=1.0):
    """(mixing matrix, mean) of a Gaussian law"""
    return np.eye(d) + 0.3 * rng.standard_normal((d, d)), spread * rng.standard_normal(d)


def draw(rng, n, law_, shift=0.0):
    a, mu = law_
    return rng.standard_normal((n, a.shape[0])) @ a.T + mu + shift


def draw_songs(rng, songs, windows, law_, window_spread=0.3, shift=0.0):
    """(rows, labels): `songs` centres from the law, `windows` rows around each, window_spread as wide as the song spread"""
    a, mu = law_
    d = a.shape[0]
    centres = rng.standard_normal((songs, d)) @ a.T + mu + shift
    rows = np.repeat(centres, windows, axis=0) + window_spread * (rng.standard_normal((songs * windows, d)) @ a.T)
    return rows, np.repeat(np.arange(songs), windows)


def pooled(x, y):
    """(mu, sigma) of the pooled rows, numpy float64; a column of zero variance gets sigma 1"""
    both = np.concatenate([x, y]).astype(np.float64)
    var = both.var(axis=0, ddof=1)
    return both.mean(axis=0), np.where(var > 0.0, np.sqrt(np.where(var > 0.0, var, 1.0)), 1.0)


def folds(labels_or_n, k, rng):
    """the fold dealing of the issue, written out with a loop"""
    if np.ndim(labels_or_n) == 0:
        n = int(labels_or_n)
        perm = rng.permutation(n)
        out = np.empty(n, dtype=np.int32)
        for j, unit in enumerate(perm):
            out[unit] = j % k
        return out
    labels = np.asarray(labels_or_n)
    uniq = sorted(set(labels.tolist()))
    perm = rng.permutation(len(uniq))
    fold_of = {}
    for j, unit in enumerate(perm):
        fold_of[uniq[unit]] = j % k
    return np.array([fold_of[v] for v in labels.tolist()], dtype=np.int32)


# ------------------------------------------------------------------ the pass
def softplus(t):
    return max(t, 0.0) + math.log1p(math.exp(-abs(t)))


def logit_pass(rows, fold, label, coef):
    """The pass of am_logit_pass_* in float64 with math.fsum (the products are rounded once each, the sums are exact).
    Returns {"sums" [K, D + 2], "z" [N]: the row's own-fold logit or NaN, "counts" [2], "z_all" [N, K], "z_abs" [N, K]:
    sum_d |a_d x_d| + |b|, "sums_abs" [K, D + 2]: the sums of the absolute terms, "sums_dz" [K, D + 2]: what an error of the
    size of the z bound passes on (|dr/dz| <= 1/4, |dloss/dz| <= 1), "terms" [K]: training rows of the model}."""
    x = np.asarray(rows, dtype=np.float64)
    coef = np.asarray(coef, dtype=np.float64)
    n, d = x.shape
    k_models = coef.shape[0]
    s = 1.0 if label else -1.0
    finite = np.isfinite(x).all(axis=1)
    z_all = np.full((n, k_models), np.nan)
    z_abs = np.zeros((n, k_models))
    for i in np.flatnonzero(finite):
        for k in range(k_models):
            prods = (coef[k, :d] * x[i]).tolist()
            z_all[i, k] = math.fsum(prods + [coef[k, d]])
            z_abs[i, k] = math.fsum([abs(p) for p in prods] + [abs(coef[k, d])])
    fold = np.asarray(fold)
    part = finite & (fold >= 0) & (fold <= k_models)
    z_own = np.full(n, np.nan)
    own = part & (fold < k_models)
    z_own[own] = z_all[own, fold[own]]
    sums = np.zeros((k_models, d + 2))
    sums_abs = np.zeros((k_models, d + 2))
    sums_dz = np.zeros((k_models, d + 2))
    terms = np.zeros(k_models)
    for k in range(k_models):
        idx = np.flatnonzero(part & (fold != k))
        terms[k] = len(idx)
        if not len(idx):
            continue
        t = s * z_all[idx, k]
        r = np.array([-s / (1.0 + math.exp(v)) if v < 700.0 else -s * 0.0 for v in t])
        loss = np.array([softplus(-v) for v in t])
        dz = (d + 2) * U * z_abs[idx, k]
        xs = x[idx]
        for j in range(d):
            sums[k, j] = math.fsum((r * xs[:, j]).tolist())
            sums_abs[k, j] = math.fsum(np.abs(r * xs[:, j]).tolist())
            sums_dz[k, j] = math.fsum((0.25 * dz * np.abs(xs[:, j])).tolist())
        sums[k, d], sums_abs[k, d], sums_dz[k, d] = math.fsum(r.tolist()), math.fsum(np.abs(r).tolist()), math.fsum((0.25 * dz).tolist())
        sums[k, d + 1], sums_abs[k, d + 1], sums_dz[k, d + 1] = math.fsum(loss.tolist()), math.fsum(np.abs(loss).tolist()), math.fsum(dz.tolist())
    counts = np.array([float(part.sum()), float((~finite).sum())])
    return dict(sums=sums, z=z_own, counts=counts, z_all=z_all, z_abs=z_abs, sums_abs=sums_abs, sums_dz=sums_dz, terms=terms)


def z_bound(z_abs, d):
    """|z - exact| <= (D + 2) 2^-53 (sum_d |a_d x_d| + |b|)"""
    return (d + 2) * U * z_abs


def sums_bound(ref):
    """per sum: (terms + 8) 2^-53 sum |terms| plus what the z bound passes on"""
    return (ref["terms"][:, None] + 8.0) * U * ref["sums_abs"] + ref["sums_dz"]


def host_pass(rows, fold, label, coef, want_z=True):
    """logit_pass in the calling convention of hip_ops.logit_pass, on torch host tensors (the *_cpu tests patch it in)"""
    import torch
    ref = logit_pass(rows.numpy(), fold.numpy(), label, coef.numpy())
    return torch.as_tensor(ref["sums"]), torch.as_tensor(ref["z"]) if want_z else None, torch.as_tensor(ref["counts"])


def fast_pass(rows, fold, label, coef, want_z=True):
    """The same pass with numpy's own sums, vectorised: for the calibration runs, where the figures are rates over hundreds
    of fits and the last bits do not matter"""
    import torch
    x, fold, coef = rows.numpy().astype(np.float64), fold.numpy(), coef.numpy()
    n, d = x.shape
    k_models = coef.shape[0]
    s = 1.0 if label else -1.0
    finite = np.isfinite(x).all(axis=1)
    xz = np.where(finite[:, None], x, 0.0)
    z = xz @ coef[:, :d].T + coef[:, d]
    part = finite & (fold >= 0) & (fold <= k_models)
    trains = part[:, None] & (fold[:, None] != np.arange(k_models)[None, :])
    t = s * z
    r = np.where(trains, -s / (1.0 + np.exp(np.minimum(t, 700.0))), 0.0)
    loss = np.where(trains, np.maximum(-t, 0.0) + np.log1p(np.exp(-np.abs(t))), 0.0)
    sums = np.concatenate([r.T @ xz, r.sum(axis=0)[:, None], loss.sum(axis=0)[:, None]], axis=1)
    own = part & (fold < k_models)
    z_own = np.full(n, np.nan)
    z_own[own] = z[own, fold[own]]
    counts = np.array([float(part.sum()), float((~finite).sum())])
    return torch.as_tensor(sums), torch.as_tensor(z_own) if want_z else None, torch.as_tensor(counts)


# ------------------------------------------------------------------ the models
def loss_grad_hess(theta, xc, xr, l2):
    """L_k, its gradient and Hessian at theta = (w, b) for the standardised training rows of the two classes"""
    out_l, out_g, out_h = 0.5 * l2 * float(theta @ theta), l2 * theta.copy(), l2 * np.eye(len(theta))
    for x, s in ((xc, 1.0), (xr, -1.0)):
        x1 = np.concatenate([x, np.ones((len(x), 1))], axis=1)
        t = s * (x1 @ theta)
        p = 1.0 / (1.0 + np.exp(np.clip(t, -700.0, 700.0)))
        out_l += 0.5 * float(np.mean(np.maximum(-t, 0.0) + np.log1p(np.exp(-np.abs(t)))))
        out_g += 0.5 * (-s * p) @ x1 / len(x)
        out_h += 0.5 * (x1 * (p * (1.0 - p))[:, None]).T @ x1 / len(x)
    return out_l, out_g, out_h


def newton(xc, xr, l2, tol=1e-13, max_iter=100):
    """(theta, |grad|_2): damped Newton from 0 to |grad L|_2 <= tol"""
    theta = np.zeros(xc.shape[1] + 1)
    f, g, h = loss_grad_hess(theta, xc, xr, l2)
    for _ in range(max_iter):
        if np.linalg.norm(g) <= tol:
            break
        step = np.linalg.solve(h, -g)
        t = 1.0
        while t > 2.0 ** -30:
            f2, g2, h2 = loss_grad_hess(theta + t * step, xc, xr, l2)
            if f2 <= f + 1e-4 * t * float(g @ step) or np.linalg.norm(g2) < np.linalg.norm(g):
                break
            t *= 0.5
        theta, f, g, h = theta + t * step, f2, g2, h2
    return theta, float(np.linalg.norm(g))


def fit(x, y, fold_x, fold_y, k_models, l2, mu, sigma):
    """(theta [K, D + 1], gradient norms [K], out-of-fold logits of x, of y) with the standardisation (mu, sigma); rows with
    a non-finite element take part in nothing (logit NaN)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    ok_x, ok_y = np.isfinite(x).all(axis=1), np.isfinite(y).all(axis=1)
    xs, ys = (x - mu) / sigma, (y - mu) / sigma
    thetas, norms = [], []
    zx, zy = np.full(len(x), np.nan), np.full(len(y), np.nan)
    for k in range(k_models):
        theta, g = newton(xs[ok_x & (fold_x != k)], ys[ok_y & (fold_y != k)], l2)
        thetas.append(theta)
        norms.append(g)
        held_x, held_y = ok_x & (fold_x == k), ok_y & (fold_y == k)
        zx[held_x] = xs[held_x] @ theta[:-1] + theta[-1]
        zy[held_y] = ys[held_y] @ theta[:-1] + theta[-1]
    return np.array(thetas), np.array(norms), zx, zy


# ------------------------------------------------------------------ the summary
def phi(z):
    return 0.5 * math.erfc(-z / math.sqrt(2.0))


def hit(z, s):
    t = s * z
    return 1.0 if t > 0.0 else (0.5 if t == 0.0 else 0.0)


def summary(zc, zr, fc, fr, gc=None, gr=None):
    """every figure of c2st_summary, by loops"""
    sides = []
    for z, f, g, s in ((zc, fc, gc, 1.0), (zr, fr, gr, -1.0)):
        g = list(range(len(z))) if g is None else np.asarray(g).tolist()
        rows = [(float(z[i]), int(f[i]), g[i], hit(float(z[i]), s)) for i in range(len(z)) if np.isfinite(z[i]) and f[i] >= 0]
        sides.append(rows)
    means = [sum(r[3] for r in rows) / len(rows) for rows in sides]
    out = {"c2st_accuracy": 0.5 * (means[0] + means[1])}
    out["c2st_log_loss"] = 0.5 * (math.fsum(softplus(-r[0]) for r in sides[0]) / len(sides[0]) + math.fsum(softplus(r[0]) for r in sides[1]) / len(sides[1]))
    var = 0.0
    for rows, mean in zip(sides, means):
        per = {}
        for r in rows:
            per[r[2]] = per.get(r[2], 0.0) + (r[3] - mean)
        units = len(per)
        var += units / (units - 1.0) * sum(v * v for v in per.values()) / (float(len(rows)) * len(rows))
    out["c2st_std_error"] = math.sqrt(0.25 * var)
    pairs, weight = 0.0, 0
    for k in sorted({r[1] for rows in sides for r in rows}):
        a, b = [r[0] for r in sides[0] if r[1] == k], [r[0] for r in sides[1] if r[1] == k]
        for u in a:
            for v in b:
                pairs += 1.0 if u > v else (0.5 if u == v else 0.0)
        weight += len(a) * len(b)
    out["c2st_auc"] = pairs / weight
    held = [[r for r in rows if r[1] == 0] for rows in sides]
    n0 = [len(h) for h in held]
    out["c2st_holdout_rows"] = (n0[0], n0[1])
    acc0 = 0.5 * (sum(r[3] for r in held[0]) / n0[0] + sum(r[3] for r in held[1]) / n0[1])
    v = 0.0
    for rows, n in zip(held, n0):
        per = {}
        for r in rows:
            per[r[2]] = per.get(r[2], 0.0) + (r[3] - 0.5)
        v += sum(t * t for t in per.values()) / (n * n)
    z = (acc0 - 0.5) / math.sqrt(0.25 * v) if v > 0.0 else 0.0
    out.update(c2st_accuracy_holdout=acc0, c2st_z=z, c2st_p_value=phi(-z))
    return out
