"""Per-group kernel-audio-distance test support, host only: the float64 oracle of the per-group Gaussian kernel sums, in
the arithmetic the library documents (include/audio_metrics_hip.h, am_mmd_rbf_groups_f32):

  d2(a, b) = max((|a|^2 + |b|^2) - 2 a.b, 0),  K = exp(-d2 gamma),
  c_i = sum_j K(x_i, y_j),  w_i = sum_{j in group(i), j != i} K(x_i, x_j),  Sxy_b = sum_{i in b} c_i,  Sxx_b = sum_{i in b} w_i.

Used by tests/test_gpu_kad_groups.py (the kernels against the oracle) and tests/test_kad_groups_cpu.py (the oracle itself)."""
import numpy as np

import kad_reference as ka


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def group_sums(x, offsets, y, gamma, dots=None):
    """x: the candidate rows in LIST order (group b = x[offsets[b]:offsets[b + 1]]).  Returns a dict of float64 arrays:
    "sxx", "sxy" [B]; "w", "c" [n] (row sums in list order); "mean_xx" = Sxx_b / (n_b (n_b - 1)) (NaN for one row) and
    "mean_xy" = Sxy_b / (n_b m) [B]; and "scale" = mean |K| over the group blocks and the cross block (the unit of the
    exact-data tolerance, as in kad_reference.mmd_parts).  `dots(a, b)`: an emulated f32 dot-product matrix."""
    x, y = np.asarray(x), np.asarray(y)
    offsets = np.asarray(offsets, dtype=np.int64)
    n, m, nb = len(x), len(y), len(offsets) - 1
    with np.errstate(over="ignore", invalid="ignore"):
        kxy = np.exp(-ka.d2_matrix(x, y, dots) * gamma)
    c = kxy.sum(1)
    w = np.zeros(n)
    sxx, sxy, abs_xx = np.zeros(nb), np.zeros(nb), []
    for b in range(nb):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        with np.errstate(over="ignore", invalid="ignore"):
            kxx = np.exp(-ka.d2_matrix(x[lo:hi], x[lo:hi], dots) * gamma)
        off = kxx.copy()
        np.fill_diagonal(off, 0.0)                                   # the valid diagonal is dropped, whatever its value
        w[lo:hi] = off.sum(1)
        sxx[b], sxy[b] = w[lo:hi].sum(), c[lo:hi].sum()
        abs_xx.append(np.abs(kxx).mean())
    sizes = np.diff(offsets).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_xx = np.where(sizes > 1, sxx / (sizes * (sizes - 1.0)), np.nan)
    scale = float(np.mean([np.mean(abs_xx), np.abs(kxy).mean()]))
    return dict(sxx=sxx, sxy=sxy, w=w, c=c, mean_xx=mean_xx, mean_xy=sxy / (sizes * float(m)), scale=scale)


def device_means(out_groups, sizes, m):
    """the same normalisation of a device [B, 2] record {Sxx_b, Sxy_b}: (mean_xx, mean_xy)"""
    g = np.asarray(out_groups, dtype=np.float64)
    sizes = np.asarray(sizes, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(sizes > 1, g[:, 0] / (sizes * (sizes - 1.0)), np.nan), g[:, 1] / (sizes * float(m))


def row_means(rows, offsets, m):
    """per-row normalisation of {w_i, c_i} in list order: w_i / (n_b - 1) (NaN for a group of one) and c_i / m"""
    r = np.asarray(rows, dtype=np.float64)
    per_row = np.repeat(np.diff(offsets), np.diff(offsets)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(per_row > 1, r[:, 0] / (per_row - 1.0), np.nan), r[:, 1] / float(m)


def mmd2_per_group(mean_xx, mean_xy, mean_yy):
    return mean_xx + mean_yy - 2.0 * mean_xy
