"""float64 numpy oracle of the Frechet-distance error bars (metrics/fad_stats.py): M^(1/2) and M^(-1/2) of M = cov_x cov_y
from the eigendecomposition of cov_x cov_y (a product of two symmetric positive definite matrices: real positive eigenvalues,
diagonalisable), the optimal-transport maps, the influence values, the plain and the cluster-robust variance, the two-model
test.  Nothing here shares code with the package."""
import math

import numpy as np


def stats(x):
    x = np.asarray(x, dtype=np.float64)
    return x.mean(axis=0), np.atleast_2d(np.cov(x, rowvar=False, ddof=1))


def product_powers(cov_x, cov_y):
    """(M^(1/2), M^(-1/2)) of M = cov_x cov_y"""
    w, v = np.linalg.eig(cov_x @ cov_y)
    w, v = w.astype(np.complex128), v.astype(np.complex128)
    vinv = np.linalg.inv(v)
    return ((v * np.sqrt(w)) @ vinv).real, ((v / np.sqrt(w)) @ vinv).real


def frechet(mu_x, cov_x, mu_y, cov_y):
    w = np.linalg.eigvals(cov_x @ cov_y)
    d = mu_x - mu_y
    return float(d @ d + np.trace(cov_x) + np.trace(cov_y) - 2.0 * np.sqrt(w.astype(np.complex128)).real.sum())


def maps(cov_x, cov_y):
    """(A, A^-1): the symmetric positive definite A with A cov_x A = cov_y, A = cov_y M^(-1/2), A^-1 = cov_x M^(-1/2)^T"""
    _, minus_half = product_powers(cov_x, cov_y)
    a, a_inv = cov_y @ minus_half, cov_x @ minus_half.T
    return 0.5 * (a + a.T), 0.5 * (a_inv + a_inv.T)


def influence_terms(mu_x, cov_x, mu_y, cov_y):
    """((B, lin, c0) of the candidate side, (B, lin, c0) of the reference side)"""
    a, a_inv = maps(cov_x, cov_y)
    eye = np.eye(len(mu_x))
    bx, by = eye - a, eye - a_inv
    dmu = mu_x - mu_y
    return (bx, 2.0 * dmu, -float(np.trace(bx @ cov_x))), (by, -2.0 * dmu, -float(np.trace(by @ cov_y)))


def psi(x, mu, b, lin, c0):
    c = np.asarray(x, dtype=np.float64) - mu
    return np.einsum("ij,ij->i", c @ b, c) + c @ lin + c0


def psi_bound(x, mu, b, lin, c0):
    """|c|^T |B| |c| + |lin|^T |c| + |c0| per row: the scale of the float64 rounding bound of psi"""
    c = np.abs(np.asarray(x, dtype=np.float64) - mu)
    return np.einsum("ij,ij->i", c @ np.abs(b), c) + c @ np.abs(lin) + abs(c0)


def influences(x, y):
    """(fd, psi_x [n], psi_y [m]) of candidate rows x against reference rows y"""
    mu_x, cov_x = stats(x)
    mu_y, cov_y = stats(y)
    tx, ty = influence_terms(mu_x, cov_x, mu_y, cov_y)
    return frechet(mu_x, cov_x, mu_y, cov_y), psi(x, mu_x, *tx), psi(y, mu_y, *ty)


def variance_rows(p):
    """s^2(psi) / n, rows as the sampling units"""
    p = np.asarray(p, dtype=np.float64)
    return float(p.var(ddof=1) / len(p))


def variance_groups(p, labels):
    """G / (G - 1) sum_g (sum_{i in g} psi_i)^2 / n^2, the labelled groups as the sampling units"""
    p, labels = np.asarray(p, dtype=np.float64), np.asarray(labels)
    sums = [p[labels == g].sum() for g in sorted(set(labels.tolist()))]
    g = len(sums)
    return float(g / (g - 1.0) * sum(s * s for s in sums) / float(len(p)) ** 2)


def side_variance(p, labels=None):
    return variance_rows(p) if labels is None else variance_groups(p, labels)


def standard_error(psi_x, psi_y, groups_x=None, groups_y=None):
    return math.sqrt(side_variance(psi_x, groups_x) + side_variance(psi_y, groups_y))


def phi(z):
    return 0.5 * math.erfc(-z / math.sqrt(2.0))


def difference_test(fad_a, fad_b, psi_a, psi_b, psi_ya, psi_yb, groups_a=None, groups_b=None, groups_y=None):
    var = side_variance(psi_a, groups_a) + side_variance(psi_b, groups_b) + \
        side_variance(np.asarray(psi_ya) - np.asarray(psi_yb), groups_y)
    diff = fad_a - fad_b
    z = diff / math.sqrt(var)
    return {"difference": diff, "std_error": math.sqrt(var), "z": z, "p_value": phi(z), "p_value_two_sided": 2.0 * phi(-abs(z))}


def compare(a, b, y, groups_a=None, groups_b=None, groups_y=None):
    fa, psi_a, psi_ya = influences(a, y)
    fb, psi_b, psi_yb = influences(b, y)
    return fa, fb, difference_test(fa, fb, psi_a, psi_b, psi_ya, psi_yb, groups_a, groups_b, groups_y)


def law(rng, d, spread=0.5, shift=0.5):
    """A Gaussian law as (mixing matrix, mean): rows are randn @ mix + mean, mix = spread * randn + I"""
    return spread * rng.standard_normal((d, d)) + np.eye(d), shift * rng.standard_normal(d)


def draw(rng, n, mix_mean):
    mix, mean = mix_mean
    return rng.standard_normal((n, len(mean))) @ mix + mean


def draw_songs(rng, songs, windows, mix_mean, window_spread=0.3):
    """(rows, labels): `songs` centres from the law, `windows` rows per song spread window_spread as wide around each"""
    mix, mean = mix_mean
    d = len(mean)
    centres = rng.standard_normal((songs, d)) @ mix + mean
    rows = np.repeat(centres, windows, axis=0) + window_spread * (rng.standard_normal((songs * windows, d)) @ mix)
    return rows, np.repeat(np.arange(songs), windows)


def with_condition(rng, d, cond, scale=1.0):
    """A symmetric positive definite d x d matrix with eigenvalues spaced geometrically over [scale, scale * cond] in a
    random orthonormal basis"""
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    w = scale * cond ** (np.arange(d) / max(d - 1, 1))
    m = (q * w) @ q.T
    return 0.5 * (m + m.T)
