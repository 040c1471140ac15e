"""Float64 numpy oracle of the feature likelihood divergence (audio_metrics_amd.metrics.fld restated with stored N x M
matrices): a mixture of isotropic Gaussians, one on every generated row g_j with variance exp(theta_j).

  normalisation   (row - mean) / std / sqrt(D) with the training set's mean and unbiased variance per dimension, a zero
                  standard deviation counting as 1; in f64, rounded to float32 once (the rows the device reads)
  z_ij = -h_j d2_ij - c_j,  h_j = 0.5 exp(-theta_j),  c_j = (D / 2) theta_j,  d2 in f64 from the float32 rows as given
  l_i  = logsumexp_j z_ij - log M - (D / 2) log 2 pi;   a row with a non-finite element has l = -inf, a centre with one
         contributes 0 and M still counts it
  L    = -mean of the finite l_i;   r_ij = exp(z_ij - lse_i),  A_j = sum_i r_ij,  B_j = sum_i r_ij d2_ij,
  dL/dtheta_j = -(h_j B_j - (D / 2) A_j) / N_finite
  fit  full-batch Adam from theta = 0: lr 0.5, beta (0.9, 0.999), eps 1e-8, bias-corrected, clamp to [theta_min, 30]"""
import math
import os

import numpy as np

THETA_MAX = 30.0
B1, B2, EPS = 0.9, 0.999, 1e-8


def normalize(rows, mean, var):
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    std = np.sqrt(var)
    std = np.where(std > 0.0, std, 1.0)
    d = rows.shape[1]
    return ((np.asarray(rows).astype(np.float64) - mean) / std / math.sqrt(d)).astype(np.float32)


def clustered(seed, d, n, m, t, copies, clusters=8):
    """(train, test, gen) float32 after the default normalisation; the first `copies` generated rows are training rows
    plus 1e-3 noise."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((clusters, d)) * 3.0

    def draw(k):
        return (centres[rng.integers(0, clusters, k)] + rng.standard_normal((k, d))).astype(np.float32)
    train, test, gen = draw(n), draw(t), draw(m)
    gen[:copies] = train[rng.choice(n, copies, replace=False)] + (1e-3 * rng.standard_normal((copies, d))).astype(np.float32)
    mean, var = train.astype(np.float64).mean(0), train.astype(np.float64).var(0, ddof=1)
    return tuple(normalize(a, mean, var) for a in (train, test, gen))


def sq_dists(x, g):
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = (x * x).sum(1)[:, None] + (g * g).sum(1)[None, :] - 2.0 * (x @ g.T)
    return np.maximum(d2, 0.0)


def _finite_rows(a):
    return np.isfinite(np.asarray(a, dtype=np.float64)).all(axis=1)


def _terms(x, g, theta):
    """(z [N, M] with -inf in the columns of non-finite centres, d2 with 0 there, finite-row mask)."""
    theta = np.asarray(theta, dtype=np.float64)
    d = x.shape[1]
    okx, okg = _finite_rows(x), _finite_rows(g)
    xs = np.where(okx[:, None], np.asarray(x, dtype=np.float64), 0.0)
    gs = np.where(okg[:, None], np.asarray(g, dtype=np.float64), 0.0)
    d2 = sq_dists(xs, gs)
    z = -(0.5 * np.exp(-theta))[None, :] * d2 - (0.5 * d * theta)[None, :]
    z[:, ~okg] = -np.inf
    d2[:, ~okg] = 0.0
    return z, d2, okx


def _lse(z):
    mx = z.max(axis=1)
    safe = np.where(np.isfinite(mx), mx, 0.0)
    with np.errstate(divide="ignore"):
        return safe + np.log(np.exp(z - safe[:, None]).sum(axis=1))


def mixture_constant(m, d):
    return math.log(m) + 0.5 * d * math.log(2.0 * math.pi)


def loglik(x, g, theta):
    """l_i for every row of x, -inf for rows with a non-finite element."""
    z, _, okx = _terms(x, g, theta)
    out = _lse(z) - mixture_constant(g.shape[0], x.shape[1])
    out[~okx] = -np.inf
    return out


def loss(x, g, theta):
    ll = loglik(x, g, theta)
    return -ll[np.isfinite(ll)].mean()


def grad_sums(x, g, theta):
    """(A [M], B [M], dL/dtheta [M]) over the rows of x with a finite log-likelihood."""
    theta = np.asarray(theta, dtype=np.float64)
    z, d2, okx = _terms(x, g, theta)
    lse = _lse(z)
    keep = okx & np.isfinite(lse)
    r = np.exp(z[keep] - lse[keep, None])
    a, b = r.sum(axis=0), (r * d2[keep]).sum(axis=0)
    n = int(keep.sum())
    grad = -((0.5 * np.exp(-theta)) * b - 0.5 * x.shape[1] * a) / n if n else np.zeros_like(a)
    return a, b, grad


def gradient(theta, a, b, d, n_finite):
    """The gradient from the two sums, in the device's order of operations."""
    theta = np.asarray(theta, dtype=np.float64)
    if not n_finite > 0:
        return np.zeros_like(theta)
    return -(((0.5 * np.exp(-theta)) * b - (0.5 * d) * a) / n_finite)


def adam_step(theta, grad, m, v, step, lr, theta_min):
    m = B1 * m + (1.0 - B1) * grad
    v = B2 * v + (1.0 - B2) * (grad * grad)
    mhat, vhat = m / (1.0 - B1 ** step), v / (1.0 - B2 ** step)
    theta = theta - lr * (mhat / (np.sqrt(vhat) + EPS))
    return np.minimum(np.maximum(theta, theta_min), THETA_MAX), m, v


def fit(x, g, steps=100, lr=0.5, theta_min=-10.0):
    """(theta after `steps` steps, the loss before every step and after the last: [steps + 1])."""
    m_rows = g.shape[0]
    theta, m, v = np.zeros(m_rows), np.zeros(m_rows), np.zeros(m_rows)
    history = []
    for step in range(1, steps + 1):
        history.append(loss(x, g, theta))
        theta, m, v = adam_step(theta, grad_sums(x, g, theta)[2], m, v, step, lr, theta_min)
    history.append(loss(x, g, theta))
    return theta, np.array(history)


def overfit_scores(g, train, test, theta):
    h = 0.5 * np.exp(-np.asarray(theta, dtype=np.float64))
    return h * (sq_dists(test, g).min(axis=0) - sq_dists(train, g).min(axis=0))


def authenticity(gen, train):
    """(authentic [M] bool, nearest training row [M], |d_gen - d_train| / max of the two [M]: small where the strict
    comparison is a tie to float32 accuracy)."""
    cross = np.sqrt(sq_dists(gen, train))
    own = np.sqrt(sq_dists(train, train))
    np.fill_diagonal(own, np.inf)
    nearest = cross.argmin(axis=1)
    d_gen, d_train = cross.min(axis=1), own.min(axis=1)[nearest]
    margin = np.abs(d_gen - d_train) / np.maximum(np.maximum(d_gen, d_train), 1e-300)
    return d_gen > d_train, nearest, margin


def delta(d, x2max, g2max, hmax, lse, cmax):
    """Worst-case error of the device's l_i against this oracle on the same float32 rows:
    2^-24 ((D + 16) (max |x|^2 + max |g|^2) h_max  - the f32 dot product and d2, times the largest bandwidth factor -
           + 4 (|lse_i| + max |c|))                - the roundings of h, c and z."""
    return 2.0 ** -24 * ((d + 16) * (x2max + g2max) * hmax + 4.0 * (np.abs(lse) + cmax))


ACCURACY_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fld", "accuracy.txt")


def record_accuracy(section, lines):
    """Replace one section ("## title" and the lines under it) of profiles/fld/accuracy.txt, keeping the others: the GPU
    tests write what they measured there.  A tree that cannot be written to is not an error of the test."""
    sections, title = {}, None
    try:
        with open(ACCURACY_FILE) as f:
            for line in f.read().splitlines():
                if line.startswith("## "):
                    title = line[3:]
                    sections[title] = []
                elif title is not None and line.strip():
                    sections[title].append(line)
    except OSError:
        pass
    sections[section] = list(lines)
    try:
        os.makedirs(os.path.dirname(ACCURACY_FILE), exist_ok=True)
        with open(ACCURACY_FILE, "w") as f:
            for title in sorted(sections):
                f.write("## %s\n%s\n\n" % (title, "\n".join(sections[title])))
    except OSError:
        pass
