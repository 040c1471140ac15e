"""Host oracle of the per-group Frechet distance (numpy float64, no GPU): an SVD form that shares no step with the device's
Gram-matrix / Jacobi route.  With S the symmetric square root of cov_y (eigh, eigenvalues clipped at 0) and Xc the centred
rows of a group of n rows, cov_x cov_y has the non-zero eigenvalues of (Xc S)^T (Xc S) / (n - 1), so

    tr sqrt(cov_x cov_y) = sum svdvals(Xc S) / sqrt(n - 1).

Singular values carry an ABSOLUTE error of a few ulps of the largest one, so the null directions add nothing of the order
sqrt(eps) that the square root of an eigenvalue's rounding dust would."""
import numpy as np


def reference_stats(y):
    """(mu_y, cov_y) of the reference rows in f64, unbiased, exactly symmetric."""
    y = np.asarray(y, dtype=np.float64)
    mu = y.mean(axis=0)
    yc = y - mu
    cov = yc.T @ yc / (len(y) - 1)
    return mu, (cov + cov.T) / 2


def sqrt_psd(cov):
    w, v = np.linalg.eigh(cov)
    return (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T


def group_oracle(x, mu_y, cov_y, root_y=None):
    """{"fd", "tr_sqrt", "scale"} of one group of rows x [n, D] (any float dtype; the VALUES are taken as given) against
    the reference statistics.  scale = |dmu|^2 + tr cov_x + tr cov_y, the size of the terms whose rounding the result
    carries: tolerances are stated relative to it."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    root = sqrt_psd(cov_y) if root_y is None else root_y
    mu_x = x.mean(axis=0)
    xc = x - mu_x
    dmu2 = float(((mu_x - mu_y) ** 2).sum())
    tr_y = float(np.trace(cov_y))
    if n == 1:
        return {"fd": dmu2 + tr_y, "tr_sqrt": 0.0, "scale": dmu2 + tr_y}
    tr_x = float((xc ** 2).sum() / (n - 1))
    tr_sqrt = float(np.linalg.svd(xc @ root, compute_uv=False).sum() / np.sqrt(n - 1))
    return {"fd": dmu2 + tr_x + tr_y - 2.0 * tr_sqrt, "tr_sqrt": tr_sqrt, "scale": dmu2 + tr_x + tr_y}


def groups_oracle(x, offsets, mu_y, cov_y, idx=None):
    """group_oracle for the groups x[idx[offsets[b]:offsets[b + 1]]] (idx None: stored order): arrays fd, tr_sqrt, scale."""
    root = sqrt_psd(cov_y)
    out = {"fd": [], "tr_sqrt": [], "scale": []}
    for b in range(len(offsets) - 1):
        sel = slice(offsets[b], offsets[b + 1])
        rows = x[sel] if idx is None else x[np.asarray(idx)[sel]]
        r = group_oracle(rows, mu_y, cov_y, root)
        for k in out:
            out[k].append(r[k])
    return {k: np.asarray(v) for k, v in out.items()}


def factor_tr_sqrt(x, y):
    """tr sqrt(cov_x cov_y) from the ROWS of both sets, without forming cov_y: with Xc [n, D] and Yc [m, D] the centred rows,
    cov_x cov_y has the non-zero eigenvalues of (Xc Yc^T)^T (Xc Yc^T) / ((n - 1)(m - 1)), so the value is the sum of the
    singular values of Xc Yc^T / sqrt((n - 1)(m - 1)).  For a reference of fewer rows than dimensions this form is free of
    the +-eps |cov_y| eigenvalues that the float64 cov_y carries in its null space and whose square roots (1e-8 each)
    sqrt_psd keeps when they come out positive."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, m = len(x), len(y)
    if n == 1:
        return 0.0
    xc, yc = x - x.mean(axis=0), y - y.mean(axis=0)
    return float(np.linalg.svd(xc @ yc.T, compute_uv=False).sum() / np.sqrt((n - 1.0) * (m - 1.0)))
