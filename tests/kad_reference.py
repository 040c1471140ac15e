"""Kernel-audio-distance test support, host only: float64 oracles of the pairwise order statistic and of the three
whole-set Gaussian kernel sums, in the arithmetic the library documents (include/audio_metrics_hip.h):

  d2(a, b) = max((|a|^2 + |b|^2) - 2 a.b, 0),  key = rn32(d2) with NaN / +inf -> +inf,  K = exp(-d2 gamma).

Used by tests/test_gpu_kad.py (the kernels against the oracles) and tests/test_kad_cpu.py (the oracles themselves)."""
import numpy as np


def sq_norms(a):
    a = np.asarray(a, dtype=np.float64)
    return (a * a).sum(1)


def d2_matrix(a, b, dots=None):
    """f64 squared distances; `dots(a, b)`: an emulated f32 dot-product matrix to use instead of the f64 one."""
    a64, b64 = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        d = a64 @ b64.T if dots is None else dots(np.asarray(a), np.asarray(b))
        return np.maximum((sq_norms(a64)[:, None] + sq_norms(b64)[None, :]) - 2.0 * d, 0.0)   # np.maximum keeps a NaN


def pair_values(x, dots=None):
    """f64 d2 of the N (N - 1) / 2 unordered pairs i < j, sorted ascending, NaN as +inf (the key of such a pair)."""
    d2 = d2_matrix(x, x, dots)
    v = d2[np.triu_indices(d2.shape[0], 1)]
    v = np.where(np.isnan(v), np.inf, v)
    return np.sort(v)


def lower_median_rank(pairs):
    return (pairs - 1) // 2


def as_key(v):
    """rn32 of an f64 order statistic (overflow -> +inf, as the conversion does)."""
    with np.errstate(over="ignore"):
        return np.float32(v)


def weighted_order_statistic(values, weights, rank):
    """The element of 0-based `rank` in the multiset that holds values[i] weights[i] times (Python integers: no overflow)."""
    order = np.argsort(np.asarray(values, dtype=np.float64), kind="stable")
    run = 0
    for i in order:
        run += int(weights[i])
        if rank < run:
            return float(values[i])
    raise ValueError(f"rank {rank} of {run} elements")


def group_pairs(points, counts):
    """(values, weights) of the pairwise d2 multiset of a set that holds points[g] counts[g] times: c_g (c_g - 1) / 2 zeros per
    group and c_g c_h copies of every cross distance g < h - no N^2 work."""
    d2 = d2_matrix(points, points)
    values, weights = [], []
    for g in range(len(counts)):
        values.append(0.0)
        weights.append(int(counts[g]) * (int(counts[g]) - 1) // 2)
        for h in range(g + 1, len(counts)):
            values.append(float(d2[g, h]))
            weights.append(int(counts[g]) * int(counts[h]))
    return values, weights


def mmd_parts(x, y, gamma, dots=None):
    """(means, scale): means = [Sxx / (n (n - 1)), Syy / (m (m - 1)), Sxy / (n m)] in f64 - Sxx, Syy over ordered pairs
    i != j - and scale = mean |K| over the three blocks (the unit of the exact-data tolerance, as in tests/test_gpu_kd.py)."""
    n, m = len(x), len(y)
    with np.errstate(over="ignore", invalid="ignore"):
        kxx, kyy, kxy = (np.exp(-d2_matrix(a, b, dots) * gamma) for a, b in ((x, x), (y, y), (x, y)))
    means = np.array([(kxx.sum() - np.trace(kxx)) / (n * (n - 1.0)), (kyy.sum() - np.trace(kyy)) / (m * (m - 1.0)),
                      kxy.sum() / (float(n) * m)])
    return means, float(np.mean([np.abs(k).mean() for k in (kxx, kyy, kxy)]))


def mmd2(means):
    return float(means[0] + means[1] - 2.0 * means[2])


def device_means(sums, n, m):
    """the same normalisation of a device {Sxx, Syy, Sxy}"""
    s = np.asarray(sums, dtype=np.float64)
    return np.array([s[0] / (n * (n - 1.0)), s[1] / (m * (m - 1.0)), s[2] / (float(n) * m)])
