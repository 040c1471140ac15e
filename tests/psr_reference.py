"""Numpy oracle of the probabilistic scoring rule behind P-precision / P-recall (csrc/psr.hip, metrics/pprecall.py): no
torch, no GPU.

  psr_f64      the definition in float64 on the float32 rows
  psr_from_d2  the device contract applied to a given float32 matrix of squared distances
  error_bound  what the float32 distances and factors of the device may cost a row's PSR against psr_f64
  latent_rows  rows of low intrinsic dimension, where PSR takes values strictly inside (0, 1)"""
import numpy as np

EPS32 = 2.0 ** -24
LATENT_SEED = 99


def latent_rows(n, D, q, seed, shift):
    """n rows on a q-dimensional linear latent (the same for every seed) plus a little isotropic noise, float32."""
    A = np.random.default_rng(LATENT_SEED).standard_normal((q, D))
    r = np.random.default_rng(seed)
    return ((r.standard_normal((n, q)) + shift) @ A + 0.02 * r.standard_normal((n, D))).astype(np.float32)


def latent_pair(n, m, D, q=3):
    """The x (seed 1, shift 0.5) and y (seed 2, shift 0) of the tests."""
    return latent_rows(n, D, q, 1, 0.5), latent_rows(m, D, q, 2, 0.0)


def knn_radii_f64(y, k):
    """Distance of every row to its k-th nearest other row, float64."""
    y = np.asarray(y, dtype=np.float64)
    nrm = (y * y).sum(1)
    d2 = np.maximum(nrm[:, None] + nrm[None, :] - 2.0 * (y @ y.T), 0.0)
    np.fill_diagonal(d2, np.inf)
    return np.sqrt(np.sort(d2, axis=1)[:, k - 1])


def psr_f64(x, y, R):
    """(psr [n], count [n], d [n, m]) in float64: d2 = |x|^2 + |y|^2 - 2 x.y clamped at 0, in range iff d < R."""
    x, y, R = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), float(R)
    d2 = np.maximum((x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2.0 * (x @ y.T), 0.0)
    d = np.sqrt(d2)
    inside = d < R
    factors = np.where(inside, d / R, 1.0)
    return 1.0 - np.prod(factors, axis=1), inside.sum(1).astype(np.int64), d


def threshold(R):
    """T: the smallest float32 >= R * R (the product in float64)."""
    r2 = float(R) * float(R)
    T = np.float32(r2)
    if float(T) < r2:
        T = np.nextafter(T, np.float32(np.inf))
    return T


def psr_from_d2(d2_f32, R):
    """The device contract on a float32 d2 matrix: (psr [n], count [n], prod [n]).  In range iff d2 < T; factor =
    min(float32 sqrt * float32(1 / R), 1) in float32; the product of those factors in float64."""
    d2 = np.asarray(d2_f32)
    assert d2.dtype == np.float32
    T = threshold(R)
    with np.errstate(invalid="ignore"):
        inside = d2 < T                                    # NaN and +inf are never in range
    safe = np.where(inside, d2, np.float32(0.0))
    f = np.minimum(np.sqrt(safe) * np.float32(1.0 / float(R)), np.float32(1.0))
    assert f.dtype == np.float32
    prod = np.prod(np.where(inside, f.astype(np.float64), 1.0), axis=1)
    return 1.0 - prod, inside.sum(1).astype(np.int64), prod


def d2_delta(x, y):
    """delta = 2^-24 (D + 16) (max |x|^2 + max |y|^2): the bound on the float32 d2 of the tile engine (the soft-min tests
    use the same one)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return EPS32 * (x.shape[1] + 16) * ((x * x).sum(1).max() + (y * y).sum(1).max())


def error_bound(x, y, d, R):
    """Per-row bound on |psr_device - psr_f64|:  sum_{j : d_ij < R + delta / R} min(delta / d_ij, sqrt(delta)) / R
    + 2 c_i 2^-24, from |sqrt(d^2 + e) - d| <= min(|e| / d, sqrt |e|) and |delta prod| <= sum |delta factor| for factors
    <= 1; the second term is the float32 rounding of a factor (square root, 1 / R, multiply).  Finite at d = 0."""
    R = float(R)
    delta = d2_delta(x, y)
    near = d < R + delta / R
    with np.errstate(divide="ignore"):
        per_pair = np.minimum(delta / d, np.sqrt(delta)) / R
    return np.where(near, per_pair, 0.0).sum(1) + 2.0 * (d < R).sum(1) * EPS32
