"""How much a Kernel Audio Distance depends on its kernel: the unbiased MMD^2 of metrics/kad.py over a grid of bandwidths,
under a Gaussian or a Laplacian kernel, and the energy distance - the MMD of k(a, b) = -|a - b|, which has no bandwidth.

  d2(a, b) = max((|a|^2 + |b|^2) - 2 a.b, 0)            f64, f64 norms, f32 matrix-core dot product (float32 rows only)
  bw^2     = the median squared distance of the reference rows, or bandwidth^2                (as kernel_audio_distance)
  gaussian   k_c = exp(-d2 / (2 bw^2 c^2))         laplacian   k_c = exp(-sqrt(d2) / (c bw))         c over `scales`
  mmd^2_c  = Sxx_c / (n (n - 1)) + Syy_c / (m (m - 1)) - 2 Sxy_c / (n m)

MMD^2 is linear in the kernel: the MMD^2 under the mixture kernel mean_c k_c (MMD-GAN, aggregated MMD tests) is the mean of
the per-scale values, which is what "kad_multiscale" reports.  All scales of a call share one Gram pass per four scales
(ops.mmd_multi_sums); the Gaussian value at c = 1 is kernel_audio_distance's, bit for bit.  The reference-side half - the
median and Syy per kernel and scale - is kept on the reference set in the cache kernel_audio_distance uses."""
import math
import struct

import numpy as np
import torch

from .. import hip_ops as ops
from ..data import AudioMetricsData
from . import kad

DEFAULT_SCALES = (0.25, 0.5, 1.0, 2.0, 4.0)
MAX_SCALES = 16
MULTISCALE_KERNELS = ("gaussian", "laplacian")


def _rows_of(what, data, name):
    rows = getattr(data, "embeddings", None)
    if rows is None:
        raise ValueError(f"{what} needs the stored rows of its {name} set, which keeps none "
                         f"(store_embeddings={getattr(data, 'store_embeddings', None)})")
    if rows.shape[0] < 2:
        raise ValueError(f"{what} needs at least 2 rows in the {name} set (it holds {rows.shape[0]}): the unbiased MMD^2 "
                         "divides by n (n - 1)")
    return rows


def _float32_pair(what, x, y):
    """The stored rows of both sets, validated before anything touches the device."""
    ex, ey = _rows_of(what, x, "candidate"), _rows_of(what, y, "reference")
    for rows, name in ((ex, "candidate"), (ey, "reference")):
        if rows.dtype == torch.float64:
            raise NotImplementedError(f"{what} takes float32 rows: the {name} set holds float64 rows (the float64 matrix-core "
                                      "form is not implemented)")
    if ex.shape[1] != ey.shape[1]:
        raise ValueError(f"feature widths differ: {ex.shape[1]} and {ey.shape[1]}")
    return ex, ey


def _parameter(kernel, bw2, c):
    """The kernel parameter of scale c in the order the device forms it (include/audio_metrics_hip.h)."""
    return 0.5 / (bw2 * (c * c)) if kernel == "gaussian" else 1.0 / (c * math.sqrt(bw2))


def _syy_key(kernel, parameter=0.0):
    """Key of a cached Syy.  A Gaussian entry is keyed by its gamma alone: kernel_audio_distance's entries are the same
    bits and are shared in both directions."""
    bits = struct.pack("<d", float(parameter))
    return bits if kernel == "gaussian" else (kernel, bits)


def _require_finite(what, values):
    if not np.isfinite(values).all():
        raise ValueError(f"{what}: a kernel sum is not finite - the sets hold non-finite rows (NaN / inf embeddings)")


def _sums_with_cached_syy(cache, ex, ey, kernel, scales, keys, bw2):
    """([S] Sxx, [S] Sxy, [S] Syy device vectors, fresh): one ops.mmd_multi_sums call, without the YY block when the cache
    holds Syy under every key (keys=None: the parameters are not known on the host yet)."""
    cached = [cache.syy.get(k) for k in keys] if keys is not None else [None]
    fresh = any(v is None for v in cached)
    blocks = ops.MMD_XX | ops.MMD_XY | (ops.MMD_YY if fresh else 0)
    sums = ops.mmd_multi_sums(ex, ey, kernel, scales, bw2=bw2, blocks=blocks)
    syy = sums[1].clone() if fresh else torch.stack(cached)
    return sums[0], sums[2], syy, fresh


def kernel_audio_distance_multiscale(x: AudioMetricsData, y: AudioMetricsData, scales=DEFAULT_SCALES, kernel="gaussian",
                                     bandwidth=None, scale=kad.KAD_SCALE):
    """KAD of candidate set `x` against reference set `y` over a grid of bandwidths c * bw, c in `scales` (1 to 16 finite
    positive numbers), bw the median pairwise distance of `y` or `bandwidth`; kernel "gaussian" or "laplacian".  Returns
    {"kad_multiscale": scale * mean_c mmd^2_c (the MMD^2 under the mixture of the S kernels), "kad_per_scale": f64 [S],
    "kad_mmd2_per_scale": f64 [S], "kad_scales": f64 [S], "kad_bandwidth": bw, "kad_kernel": kernel}."""
    what = "kernel_audio_distance_multiscale"
    if kernel not in MULTISCALE_KERNELS:
        raise ValueError(f"kernel={kernel!r} is not one of {list(MULTISCALE_KERNELS)} (the energy kernel has no bandwidth: "
                         "energy_distance)")
    grid = ops.mmd_scales(scales)
    if len(grid) > MAX_SCALES:
        raise ValueError(f"scales holds {len(grid)} entries, at most {MAX_SCALES} are taken")
    ex, ey = _float32_pair(what, x, y)
    n, m = int(ex.shape[0]), int(ey.shape[0])
    cache, bw, _, bw2_dev = kad._resolve_bandwidth(bandwidth, y, ey)
    bw2 = bw * bw if bw is not None else cache.bw2_host            # None: the median has not been read back yet
    keys = [_syy_key(kernel, _parameter(kernel, bw2, c)) for c in grid] if bw2 is not None else None
    sxx, sxy, syy, fresh = _sums_with_cached_syy(cache, ex, ey, kernel, grid, keys, bw2_dev if bw2_dev is not None else bw2)
    tail = bw2_dev.to(torch.float64).reshape(1) if bw2_dev is not None else torch.zeros(1, dtype=torch.float64, device=sxx.device)
    flat = torch.cat([sxx, sxy, syy, tail]).cpu().numpy()           # the one read-back
    s = len(grid)
    if bw2_dev is not None:
        bw2 = float(flat[3 * s])
        bw = kad._finish_bandwidth(cache, bw, None, bw2_dev, bw2, None)      # checks the median, remembers its value
    if fresh:
        for j, c in enumerate(grid):
            cache.syy[_syy_key(kernel, _parameter(kernel, bw2, c))] = syy[j]
    _require_finite(what, flat[:3 * s])
    mmd2 = flat[:s] / (n * (n - 1.0)) + flat[2 * s:3 * s] / (m * (m - 1.0)) - 2.0 * flat[s:2 * s] / (float(n) * m)
    return {"kad_multiscale": float(scale) * float(np.mean(mmd2)), "kad_per_scale": float(scale) * mmd2, "kad_mmd2_per_scale": mmd2,
            "kad_scales": np.asarray(grid, dtype=np.float64), "kad_bandwidth": bw, "kad_kernel": kernel}


def energy_distance(x: AudioMetricsData, y: AudioMetricsData):
    """Energy distance (Szekely and Rizzo) between the stored rows of two sets, in the unbiased (i != j) normalisation of
    kernel_audio_distance: {"energy_distance": 2 E|x - y| - E|x - x'| - E|y - y'|, "energy_mean_xy", "energy_mean_xx",
    "energy_mean_yy"} - the three mean Euclidean distances.  It is the MMD^2 of k(a, b) = -|a - b|: no bandwidth, no scale.
    The reference-side mean is kept on `y` until its rows change."""
    what = "energy_distance"
    ex, ey = _float32_pair(what, x, y)
    n, m = int(ex.shape[0]), int(ey.shape[0])
    cache = kad.reference_cache(y)
    key = _syy_key("energy")
    sxx, sxy, syy, fresh = _sums_with_cached_syy(cache, ex, ey, "energy", [1.0], [key], None)
    if fresh:
        cache.syy[key] = syy[0]
    sxx_v, sxy_v, syy_v = torch.cat([sxx, sxy, syy]).cpu().tolist()  # the one read-back
    _require_finite(what, [sxx_v, sxy_v, syy_v])
    mean_xx, mean_yy, mean_xy = -sxx_v / (n * (n - 1.0)), -syy_v / (m * (m - 1.0)), -sxy_v / (float(n) * m)
    return {"energy_distance": 2.0 * mean_xy - mean_xx - mean_yy, "energy_mean_xy": mean_xy, "energy_mean_xx": mean_xx,
            "energy_mean_yy": mean_yy}
