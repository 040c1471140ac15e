"""numpy float64 oracles of the Vendi score (audio_metrics_amd.metrics.vendi): eigvalsh of K / n with the zero rule, and - for
the cosine kernel - the squared singular values of the normalised rows as a second, independent oracle."""
import math

import numpy as np

EPS = 2.0 ** -52


def group_zero_tol(n):
    """the per-group kernel's rule: eigenvalues <= 4 n 2^-52 lambda_max count as zero"""
    return 4.0 * n * EPS


def kernel_matrix(x, kernel, bandwidth=None):
    x = np.asarray(x, dtype=np.float64)
    g = x @ x.T
    diag = np.diag(g).copy()
    if kernel == "cosine":
        s = np.sqrt(diag)
        k = g / (s[:, None] * s[None, :])
    else:
        assert kernel == "gaussian" and bandwidth is not None
        d2 = np.maximum((diag[:, None] + diag[None, :]) - 2.0 * g, 0.0)
        k = np.exp(-d2 / (2.0 * float(bandwidth) ** 2))
    np.fill_diagonal(k, 1.0)
    return 0.5 * (k + k.T)


def eigenvalues(x, kernel, bandwidth=None):
    """eigenvalues of K / n, descending (LAPACK eigvalsh)"""
    k = kernel_matrix(x, kernel, bandwidth)
    return np.linalg.eigvalsh(k / len(k))[::-1].copy()


def svd_eigenvalues(x):
    """cosine kernel only: the min(n, D) squared singular values of the normalised rows, over n, descending"""
    x = np.asarray(x, dtype=np.float64)
    xh = x / np.linalg.norm(x, axis=1, keepdims=True)
    s = np.linalg.svd(xh, compute_uv=False)
    return np.sort(s * s / len(x))[::-1].copy()


def apply_zero_rule(lam, zero_tol, clearance=1e3):
    """(kept eigenvalues, descending).  Asserts the condition every comparison against this oracle rests on: no eigenvalue
    lies near the threshold - the smallest kept one is at least `clearance` times the threshold and every dropped one is at
    or below it, so kept and dropped are `clearance` apart and a 1e-12 lambda_max difference between two solvers cannot move
    an eigenvalue across.  (LAPACK returns the exact nulls of duplicate rows at a few 2^-52 lambda_max, the threshold for
    two or three rows is only 8 - 12 times 2^-52: the dropped side cannot be asked to lie 1e3 BELOW the threshold.)"""
    lam = np.sort(np.asarray(lam, dtype=np.float64))[::-1]
    thr = zero_tol * lam[0]
    keep = lam > thr
    kept, dropped = lam[keep], lam[~keep]
    assert kept.size and kept[-1] >= clearance * thr, ("an eigenvalue lies within %g of the zero threshold" % clearance, kept[-1], thr)
    assert dropped.size == 0 or np.abs(dropped).max() <= thr, (dropped, thr)
    return kept


def score(kept, q):
    """the Vendi score of order q of the kept eigenvalues (descending)"""
    kept = np.asarray(kept, dtype=np.float64)
    if q == 1.0:
        return math.exp(-float(np.sum(kept * np.log(kept))))
    if math.isinf(q):
        return 1.0 / float(kept[0])
    return float(np.sum(kept ** q)) ** (1.0 / (1.0 - q))


def oracle(x, kernel, bandwidth=None, zero_tol=None, orders=(1.0,), clearance=1e3):
    """dict(lam: all n eigenvalues descending with the dropped ones as 0, kept, rank, scores: {q: value}, entropy)"""
    n = len(x)
    lam = eigenvalues(x, kernel, bandwidth)
    kept = apply_zero_rule(lam, group_zero_tol(n) if zero_tol is None else zero_tol, clearance)
    full = np.zeros(n)
    full[:kept.size] = kept
    return {"lam": full, "kept": kept, "rank": int(kept.size), "scores": {q: score(kept, q) for q in orders},
            "entropy": -float(np.sum(kept * np.log(kept)))}


def log_score_bound(kept, eig_tol):
    """|ln VS - ln VS_oracle| <= sum_i eig_tol lambda_0 (|ln lambda_i| + 1) for eigenvalues within eig_tol lambda_0 of the
    oracle's: d(-l ln l) / dl = -(ln l + 1).  Computed from the oracle's own kept eigenvalues."""
    kept = np.asarray(kept, dtype=np.float64)
    return float(np.sum(eig_tol * kept[0] * (np.abs(np.log(kept)) + 1.0)))


# ---------------------------------------------------------------- the row families of the GPU tests
def family_rows(kind, n, d, rng):
    x = rng.standard_normal((n, d))
    if kind == "song":
        x = rng.standard_normal(d)[None, :] + 0.3 * x
    elif kind == "dups":
        for i in range(2, n, 3):                          # every third row repeats the one before it
            x[i] = x[i - 1]
    else:
        assert kind == "randn"
    return x
