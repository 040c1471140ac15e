"""Two-sided row sums and the KAD error statistics, host only: the float64 oracle of am_mmd_rbf_rows_f32 in the arithmetic the
library documents (include/audio_metrics_hip.h),

  d2(a, b) = max((|a|^2 + |b|^2) - 2 a.b, 0),  K = exp(-d2 gamma),
  w_i = sum_{j != i} K(x_i, x_j),  c_i = sum_j K(x_i, y_j),  v_j = sum_{l != j} K(y_j, y_l),  r_j = sum_i K(x_i, y_j),

and the two host statistics of metrics/kad_stats.py written as direct loops.

Used by tests/test_gpu_mmd_rows.py and tests/test_gpu_kad_stats.py (the kernels and front ends against the oracle) and
tests/test_mmd_rows_cpu.py (the oracle itself)."""
import math

import numpy as np

import kad_reference as ka

BLOCK = 2048          # rows of a block per step: no matrix larger than BLOCK x the other set exists


def _kernel(a, b, gamma, dots):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp(-ka.d2_matrix(a, b, dots) * gamma)


def row_sums(x, y, gamma, dots=None, same=False):
    """dict of float64 arrays "w", "c" [n], "v", "r" [m] and "scale" = mean |K| over the three blocks (the unit of the
    exact-data tolerance, as in kad_reference.mmd_parts).  The diagonal of Kxx / Kyy is dropped by index, whatever its value.
    `dots(a, b)`: an emulated f32 dot-product matrix.  same=True: y IS x (the YY block is not computed again)."""
    x, y = np.asarray(x), np.asarray(y)
    n, m = len(x), len(y)

    def within(a):
        s, total = np.zeros(len(a)), 0.0
        for lo in range(0, len(a), BLOCK):
            k = _kernel(a[lo:lo + BLOCK], a, gamma, dots)
            total += np.abs(k).sum()
            k[np.arange(k.shape[0]), lo + np.arange(k.shape[0])] = 0.0
            s[lo:lo + BLOCK] = k.sum(1)
        return s, total / (float(len(a)) * len(a))
    w, abs_xx = within(x)
    v, abs_yy = (w.copy(), abs_xx) if same else within(y)
    c, r, abs_xy = np.zeros(n), np.zeros(m), 0.0
    for lo in range(0, n, BLOCK):
        k = _kernel(x[lo:lo + BLOCK], y, gamma, dots)
        c[lo:lo + BLOCK] = k.sum(1)
        r += k.sum(0)
        abs_xy += np.abs(k).sum()
    return dict(w=w, c=c, v=v, r=r, scale=float(np.mean([abs_xx, abs_yy, abs_xy / (float(n) * m)])))


def normalised(s):
    """(w / (n - 1), c / m, v / (m - 1), r / n) of a dict of row sums or of the device pair (out_x [n, 2], out_y [m, 2])"""
    if isinstance(s, dict):
        w, c, v, r = s["w"], s["c"], s["v"], s["r"]
    else:
        ox, oy = (np.asarray(t, dtype=np.float64) for t in s)
        w, c, v, r = ox[:, 0], ox[:, 1], oy[:, 0], oy[:, 1]
    n, m = len(w), len(v)
    return w / (n - 1.0), c / float(m), v / (m - 1.0), r / float(n)


def _sample_variance(a):
    mean = sum(a) / len(a)
    return sum((t - mean) ** 2 for t in a) / (len(a) - 1.0)


def standard_error(w, c, v, r):
    """(mmd2, se) by direct loops over Python floats"""
    n, m = len(w), len(v)
    mmd2 = sum(w) / (n * (n - 1.0)) + sum(v) / (m * (m - 1.0)) - 2.0 * sum(c) / (float(n) * m)
    a = [float(w[i]) / (n - 1.0) - float(c[i]) / m for i in range(n)]
    b = [float(v[j]) / (m - 1.0) - float(r[j]) / n for j in range(m)]
    return mmd2, math.sqrt(4.0 * _sample_variance(a) / n + 4.0 * _sample_variance(b) / m)


def difference_test(w_a, c_a, r_a, w_b, c_b, r_b):
    """(diff, se, z, p one-sided, p two-sided) by direct loops; a variance of 0 gives NaN for z and the p-values"""
    na, nb, m = len(w_a), len(w_b), len(r_a)
    diff = (sum(w_a) / (na * (na - 1.0)) - 2.0 * sum(c_a) / (float(na) * m)) - (sum(w_b) / (nb * (nb - 1.0)) - 2.0 * sum(c_b) / (float(nb) * m))
    a = [float(w_a[i]) / (na - 1.0) - float(c_a[i]) / m for i in range(na)]
    b = [float(w_b[i]) / (nb - 1.0) - float(c_b[i]) / m for i in range(nb)]
    rho = [float(r_b[j]) / nb - float(r_a[j]) / na for j in range(m)]
    var = 4.0 * _sample_variance(a) / na + 4.0 * _sample_variance(b) / nb + 4.0 * _sample_variance(rho) / m
    if var == 0.0:
        return diff, 0.0, float("nan"), float("nan"), float("nan")
    z = diff / math.sqrt(var)
    phi = lambda t: 0.5 * math.erfc(-t / math.sqrt(2.0))
    return diff, math.sqrt(var), z, phi(z), 2.0 * phi(-abs(z))
