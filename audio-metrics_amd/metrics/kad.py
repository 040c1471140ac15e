"""Kernel Audio Distance (Chung et al. 2025, "KAD: No More FAD!"): the unbiased MMD^2 between the WHOLE candidate set and
the WHOLE reference set under a Gaussian kernel whose bandwidth is the median pairwise distance of the reference set.

  d2(a, b) = max((|a|^2 + |b|^2) - 2 a.b, 0)            f64, f64 norms, f32 matrix-core dot product (float32 rows);
                                                         two float64 sets: the f64 matrix cores, every step in f64
  bw^2     = rn32(lower median of d2 over the m (m - 1) / 2 unordered reference pairs)        (ops.pairwise_select_sq)
  k(a, b)  = exp(-d2(a, b) / (2 bw^2))                                                        (ops.mmd_rbf_sums)
  mmd^2    = Sxx / (n (n - 1)) + Syy / (m (m - 1)) - 2 Sxy / (n m),     kad = scale * mmd^2

Unlike the subset kernel distance (metrics/kd.py) nothing is sampled, so the value has no seed and no subset size, and -
the reason the field adopted it - no bias in the sample size.  The reference-side half (the median and Syy) depends on
the reference set alone and is kept on it: a big cached reference against a small candidate set costs the cross block."""
import math
import struct
import warnings

import numpy as np
import torch

from .. import hip_ops as ops
from ..data import AudioMetricsData
from ._groups import labelled_rows, sort_into_groups

KAD_SCALE = 100.0
CACHE_ATTR = "_kad_cache"         # on the reference AudioMetricsData; NOT part of serialize(): the file layout stays as it is


def _gamma_bits(gamma):
    return struct.pack("<d", float(gamma))


class _ReferenceCache:
    """What KAD derives from a reference set alone, valid for exactly the rows it was computed from: (number of rows,
    _content_version) - every append bumps the version, so both entries are recomputed after an add (the radii cache's
    "survives appends" quirk is the reference's own and is not copied here)."""

    def __init__(self, key):
        self.key = key
        self.bw2 = None            # 0-dim float32 device tensor: median squared distance
        self.bw2_host = None       # its value, once a result has been read back
        self.syy = {}              # gamma bits -> 0-dim float64 device tensor
        self.vrow = {}             # gamma bits -> float64 [m] device tensor: the row sums v_j of Kyy (metrics/kad_stats.py)
        self.cells = {}            # (gamma bits, unit_rows) -> float64 [U, U] device tensor: the unit-pair sums of Kyy (metrics/kad_perm.py)
        self.sinkhorn = {}         # (blur, scaling, rtol, max_iter, diam2) -> the reference's own solve (metrics/sinkhorn.py)
        self.sliced = {}           # (seed, n_projections) -> (chunk size, the sorted projections in chunks) (metrics/sliced.py)
        self.rff = {}              # (bandwidth source, n_features, seed) -> float64 [2R, 2R] device tensor: the moment matrix S (metrics/fkea.py)


def reference_cache(y):
    rows = y.embeddings
    key = (int(rows.shape[0]), int(getattr(y, "_content_version", -1)))
    cache = getattr(y, CACHE_ATTR, None)
    if cache is None or cache.key != key:
        cache = _ReferenceCache(key)
        setattr(y, CACHE_ATTR, cache)
    return cache


def _rows_of(data, name):
    rows = getattr(data, "embeddings", None)
    if rows is None:
        raise ValueError(f"kernel_audio_distance needs the stored rows of its {name} set, which keeps none "
                         f"(store_embeddings={getattr(data, 'store_embeddings', None)})")
    if rows.shape[0] < 2:
        raise ValueError(f"kernel_audio_distance needs at least 2 rows in the {name} set (it holds {rows.shape[0]}): the "
                         "unbiased MMD^2 divides by n (n - 1)")
    return rows


def _same_row_type(what, ex, ey):
    """float32 rows in both sets (the f32 tile engine) or float64 rows in both (the f64 matrix-core forms: every step in
    f64, the bandwidth still the float32 rounding of the f64 median); a mixed pair is refused before any device call."""
    for rows, name, other in ((ex, "candidate", ey), (ey, "reference", ex)):
        if rows.dtype == torch.float64 and other.dtype != torch.float64:
            raise NotImplementedError(f"{what}: the {name} set holds float64 rows and the other set {other.dtype} rows; both "
                                      "sets must hold float32 rows or both float64 rows (a mixed pair is not implemented)")


def _resolve_bandwidth(bandwidth, y, ey):
    """(cache, bw, gamma, bw2_dev) for `bandwidth` against the reference-side cache of y.  A number fixes bw and gamma and
    leaves bw2_dev None; None takes the median squared distance of the reference rows ey as the device scalar bw2_dev
    (computed once per content of y), and gamma stays None until a result has been read back once."""
    bw = gamma = bw2_dev = None
    if bandwidth is not None:
        bw = float(bandwidth)
        if not math.isfinite(bw) or bw <= 0.0:
            raise ValueError(f"bandwidth={bandwidth!r} must be a finite positive number")
        gamma = 1.0 / (2.0 * bw * bw)
    cache = reference_cache(y)
    if gamma is None:
        if cache.bw2 is None:
            cache.bw2 = ops.pairwise_select_sq(ey)
        bw2_dev = cache.bw2
        if cache.bw2_host is not None:                     # the bits the device forms from the same float32: 0.5 / (double)bw2
            _check_bandwidth(cache.bw2_host)
            gamma = 0.5 / cache.bw2_host
    return cache, bw, gamma, bw2_dev


def _finish_bandwidth(cache, bw, gamma, bw2_dev, bw2_v, fresh_syy):
    """After the read-back: the bandwidth the device used (bw2_v, where it came from bw2_dev) goes into the cache and is
    checked, and a freshly computed Syy is stored under the gamma it belongs to.  Returns bw."""
    if bw2_dev is not None:
        cache.bw2_host = bw2_v
        _check_bandwidth(bw2_v)
        gamma = 0.5 / bw2_v
        bw = math.sqrt(bw2_v)
    if fresh_syy is not None:
        cache.syy[_gamma_bits(gamma)] = fresh_syy
    return bw


def kernel_audio_distance(x: AudioMetricsData, y: AudioMetricsData, bandwidth=None, scale=KAD_SCALE):
    """KAD of candidate set `x` against reference set `y`.  bandwidth=None: the median pairwise distance of `y`; a number
    fixes it.  Returns {"kad": scale * mmd^2, "kad_mmd2": mmd^2, "kad_bandwidth": bw}."""
    ex, ey = _rows_of(x, "candidate"), _rows_of(y, "reference")
    _same_row_type("kernel_audio_distance", ex, ey)
    if ex.shape[1] != ey.shape[1]:
        raise ValueError(f"feature widths differ: {ex.shape[1]} and {ey.shape[1]}")
    n, m = int(ex.shape[0]), int(ey.shape[0])
    cache, bw, gamma, bw2_dev = _resolve_bandwidth(bandwidth, y, ey)
    syy = cache.syy.get(_gamma_bits(gamma)) if gamma is not None else None
    blocks = ops.MMD_XX | ops.MMD_XY | (0 if syy is not None else ops.MMD_YY)
    if bw2_dev is not None:
        sums = ops.mmd_rbf_sums(ex, ey, bw2=bw2_dev, blocks=blocks)
    else:
        sums = ops.mmd_rbf_sums(ex, ey, gamma=gamma, blocks=blocks)
    fresh_syy = syy is None
    if fresh_syy:
        syy = sums[1].clone()
    tail = bw2_dev.to(torch.float64) if bw2_dev is not None else torch.zeros((), dtype=torch.float64, device=sums.device)
    sxx, sxy, syy_v, bw2_v = torch.stack([sums[0], sums[2], syy, tail]).cpu().tolist()       # the one read-back
    bw = _finish_bandwidth(cache, bw, gamma, bw2_dev, bw2_v, syy if fresh_syy else None)
    mmd2 = sxx / (n * (n - 1.0)) + syy_v / (m * (m - 1.0)) - 2.0 * sxy / (float(n) * m)
    return {"kad": float(scale) * mmd2, "kad_mmd2": mmd2, "kad_bandwidth": bw}


def combine_group_sums(sxx, sxy, sizes, syy, m, scale=KAD_SCALE):
    """(kad_per_group, mmd2_per_group) from the per-group kernel sums - host arithmetic, float64 numpy:
        mmd2_b = Sxx_b / (n_b (n_b - 1)) + Syy / (m (m - 1)) - 2 Sxy_b / (n_b m).
    A group of one row has no unbiased estimate: its value is NaN, and ONE RuntimeWarning per call says how many such groups
    there are.  A NaN sum (a non-finite row in that group) stays the NaN of that group alone."""
    sxx, sxy = np.asarray(sxx, dtype=np.float64), np.asarray(sxy, dtype=np.float64)
    n = np.asarray(sizes, dtype=np.float64)
    single = n < 2
    pairs = np.where(single, np.nan, n * (n - 1.0))
    mmd2 = sxx / pairs + float(syy) / (m * (m - 1.0)) - 2.0 * sxy / (n * float(m))
    if single.any():
        warnings.warn(f"kernel_audio_distance_per_group: {int(single.sum())} of {len(n)} groups hold a single row and have no "
                      "unbiased MMD^2 (it divides by n (n - 1)); their value is NaN", RuntimeWarning, stacklevel=3)
    return float(scale) * mmd2, mmd2


def kernel_audio_distance_per_group(x: AudioMetricsData, y: AudioMetricsData, groups, bandwidth=None, scale=KAD_SCALE,
                                    return_rows=False):
    """KAD of every group of x's stored rows, each on its own, against the whole reference set y (the per-song score: the
    unbiased MMD^2 has no bias in the group size, so groups of different sizes compare).  `groups`: one integer label per
    stored row of x (numpy or torch, any order, any values).  One library call for all groups (ops.mmd_rbf_group_sums: the
    Gram work of one cross block); the bandwidth and Syy come from - and go into - the reference-side cache that
    kernel_audio_distance uses.  Returns {"kad_per_group": f64 [B], "kad_mmd2_per_group": f64 [B], "group_labels": [B]
    ascending, "group_sizes": int64 [B], "kad_bandwidth": float}; return_rows=True adds "row_cross_mean": f64 [n] in STORED
    row order, c_i / m = the reference's kernel density at each candidate row.  A group of one row gets NaN and the call
    one RuntimeWarning."""
    rows, n, labels = labelled_rows(x, groups, "kernel_audio_distance_per_group", "its candidate set")
    ey = _rows_of(y, "reference")
    _same_row_type("kernel_audio_distance_per_group", rows, ey)
    if rows.shape[1] != ey.shape[1]:
        raise ValueError(f"feature widths differ: {rows.shape[1]} and {ey.shape[1]}")
    m = int(ey.shape[0])
    cache, bw, gamma, bw2_dev = _resolve_bandwidth(bandwidth, y, ey)
    order, _, group_labels, sizes = sort_into_groups(labels.to(rows.device, torch.int64))
    offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    width = {"bw2": bw2_dev} if bw2_dev is not None else {"gamma": gamma}
    syy = cache.syy.get(_gamma_bits(gamma)) if gamma is not None else None
    fresh_syy = syy is None
    if fresh_syy:
        syy = ops.mmd_rbf_sums(ey, ey, blocks=ops.MMD_YY, **width)[1].clone()
    res = ops.mmd_rbf_group_sums(rows, order, offs, ey, rows=return_rows, **width)
    out_groups, check = res[0], res[-1]
    tail = bw2_dev.to(torch.float64) if bw2_dev is not None else torch.zeros((), dtype=torch.float64, device=out_groups.device)
    parts = [out_groups.reshape(-1), torch.stack([syy, tail])]
    if return_rows:
        stored = torch.empty(n, dtype=torch.float64, device=out_groups.device)
        stored[order] = res[1][:, 1] / float(m)            # list order -> stored order
        parts.append(stored)
    flat = torch.cat(parts).cpu().numpy()                   # the one read-back of results
    check()
    nb = len(sizes)
    syy_v, bw2_v = float(flat[2 * nb]), float(flat[2 * nb + 1])
    bw = _finish_bandwidth(cache, bw, gamma, bw2_dev, bw2_v, syy if fresh_syy else None)
    sums = flat[:2 * nb].reshape(nb, 2)
    kad, mmd2 = combine_group_sums(sums[:, 0], sums[:, 1], sizes, syy_v, m, scale)
    out = {"kad_per_group": kad, "kad_mmd2_per_group": mmd2, "group_labels": group_labels, "group_sizes": sizes, "kad_bandwidth": bw}
    if return_rows:
        out["row_cross_mean"] = flat[2 * nb + 2:].copy()
    return out


def _check_bandwidth(bw2):
    if not math.isfinite(bw2):
        raise ValueError("kernel_audio_distance: the median pairwise distance of the reference set is not finite - at least "
                         "half of its row pairs involve a row with non-finite elements (NaN / inf embeddings)")
    if bw2 <= 0.0:
        raise ValueError("kernel_audio_distance: the median pairwise distance of the reference set is 0 - more than half of "
                         "its row pairs coincide (duplicate rows); pass bandwidth= to fix the kernel width")
