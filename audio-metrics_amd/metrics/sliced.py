"""Sliced Wasserstein distance (Rabin et al., SSVM 2011; Bonneel et al., JMIV 2015; the SWD column of GAN evaluations): the
mean, over random unit directions, of the exact 1-D W_p^p between the two sets projected on the direction.  Optimal
transport between the two sets AS THEY ARE like the Sinkhorn divergence, but without a blur, without iterations and at
O(L N (D + log N)): the one transport distance of this package that runs at 100 000 x 100 000 rows on every call.  The
reference has no such function.

  directions  numpy.random.default_rng(seed).standard_normal((L, D)), every row normalised in f64 and rounded to float32
              once (sliced_directions: host arithmetic, the same on every machine)
  per chunk of chunk_projections directions
    project   z[l, i] = <theta_l, x_i> in f32 on the exact tile engine              ops.sliced_project
    sort      every row of z ascending, keys only, in place                         ops.sort_rows
    merge     W_p^p of the two sorted rows on the merged grid {i / n} u {j / m}, f64  ops.sliced_w
  swd_pp = mean_l W_p^p(l),  swd = swd_pp^(1 / p)

A projection's bits do not depend on its neighbours in the call, the sort is exact and the merge is per row, so the
per-projection values do not depend on chunk_projections.  One read-back at the end: L doubles and L counts.

Scale.  For a pure mean shift c, E_theta <theta, c>^2 = |c|^2 / D: D swd^2 at p = 2 is the quantity in FAD's units."""
import math
import warnings

import numpy as np
import torch

from .. import hip_ops as ops
from .kad import reference_cache


def sliced_directions(d, n_projections, seed):
    """float32 numpy [n_projections, d]: standard normal draws of numpy.random.default_rng(seed), every row divided by its f64
    norm and rounded to float32 once.  Host only."""
    d, n_projections = int(d), int(n_projections)
    if d < 1 or n_projections < 1:
        raise ValueError(f"sliced_directions: d={d} and n_projections={n_projections} must be at least 1")
    g = np.random.default_rng(seed).standard_normal((n_projections, d))
    return (g / np.sqrt((g * g).sum(axis=1, keepdims=True))).astype(np.float32)


def _rows_of(data, name):
    rows = getattr(data, "embeddings", None)
    if rows is None or rows.shape[0] == 0:
        raise ValueError(f"sliced_wasserstein_distance needs the stored rows of its {name} set, which keeps none "
                         f"(store_embeddings={getattr(data, 'store_embeddings', None)})")
    return rows


def sliced_summary(per_projection, p, nonfinite=0):
    """The result dict from the L per-projection W_p^p values (host arithmetic, f64).  swd_std_error = s(W_p^p) /
    (sqrt(L) p swd^(p - 1)), s the sample standard deviation: the Monte-Carlo error of the slicing by the delta method, NaN
    for L = 1 or swd = 0.  nonfinite > 0 makes swd (and what derives from it) NaN."""
    w = np.asarray(per_projection, dtype=np.float64)
    n = int(w.shape[0])
    if nonfinite > 0:
        swd_pp = swd = wmax = err = math.nan
        imax = -1
    else:
        swd_pp = float(w.mean())
        swd = swd_pp if p == 1 else math.sqrt(swd_pp)
        imax = int(np.argmax(w))
        wmax = float(w[imax]) if p == 1 else math.sqrt(float(w[imax]))
        err = math.nan
        if n > 1 and swd > 0.0:
            err = float(w.std(ddof=1)) / (math.sqrt(n) * p * swd ** (p - 1))
    return {"swd": swd, "swd_pp": swd_pp, "swd_p": p, "swd_n_projections": n, "swd_max": wmax, "swd_max_index": imax,
            "swd_std_error": err}


def _sorted_projections(rows, theta):
    z = ops.sliced_project(rows, theta)
    return ops.sort_rows(z, out=z)


def sliced_wasserstein_distance(cand, ref, n_projections=512, p=2, seed=0, cache_reference=True, chunk_projections=128,
                                return_projections=False):
    """The sliced p-Wasserstein distance of candidate set `cand` against reference set `ref` (stored float32 rows, uniform
    weights), p = 1 or 2, over n_projections directions of sliced_directions(D, n_projections, seed).  Returns {"swd": the
    distance, in the units of the embeddings, "swd_pp": the mean per-projection W_p^p = swd^p, "swd_p", "swd_n_projections",
    "swd_seed", "swd_max": the largest per-projection W_p (a lower bound of the max-sliced distance), "swd_max_index",
    "swd_std_error": the Monte-Carlo error of the slicing - NOT the sampling error of the sets}; return_projections=True
    adds "swd_per_projection" (float64 numpy [L], W_p^p) and "swd_directions" (float32 numpy [L, D]).
    A non-finite projection anywhere gives swd = NaN (the per-projection values stay) and one RuntimeWarning naming the
    count.  The work runs in chunks of chunk_projections directions: four [chunk, rows] float32 matrices, 205 MB at 128 x
    100 000 rows; the values do not depend on the chunking.  cache_reference=True keeps the reference's sorted projections
    on `ref` under (seed, n_projections) - 4 L m bytes, 205 MB at 512 x 100 000 - until rows are appended; a cached call
    returns the bits of an uncached one."""
    ex, ey = _rows_of(cand, "candidate"), _rows_of(ref, "reference")
    for rows, name in ((ex, "candidate"), (ey, "reference")):
        if rows.dtype == torch.float64:
            raise NotImplementedError(f"sliced_wasserstein_distance: the {name} set holds float64 rows; sliced_project takes "
                                      "float32 rows (the float64 matrix-core form is not implemented)")
    if ex.shape[1] != ey.shape[1]:
        raise ValueError(f"feature widths differ: {ex.shape[1]} and {ey.shape[1]}")
    if p not in (1, 2):
        raise ValueError(f"p={p!r} must be 1 or 2")
    n_projections, chunk = int(n_projections), int(chunk_projections)
    if n_projections < 1:
        raise ValueError(f"n_projections={n_projections} must be at least 1")
    if chunk < 1:
        raise ValueError(f"chunk_projections={chunk} must be at least 1")
    n, m, d = int(ex.shape[0]), int(ey.shape[0]), int(ex.shape[1])
    if n * m >= 1 << 53:
        raise ValueError(f"n * m = {n} * {m} must stay below 2^53 (the coupling's weights are exact integers)")
    directions = sliced_directions(d, n_projections, seed)

    same = cand is ref or ex is ey
    ex = ops.as_matrix(ex, "cand")                      # rows the library can take as they are: converted once, not per chunk
    ey = ex if same else ops.as_matrix(ey, "ref")
    theta = ops.upload_host_array(directions, ex.device)
    store = reference_cache(ref).sliced if cache_reference else None
    key = (seed, n_projections)
    cached = _cached_reader(store.get(key), chunk) if store is not None else None
    values, counts, kept = [], [], []
    for lo in range(0, n_projections, chunk):
        t = theta[lo:lo + chunk]
        zy = cached(lo, lo + t.shape[0]) if cached is not None else _sorted_projections(ey, t)
        zx = zy if same else _sorted_projections(ex, t)
        w, bad = ops.sliced_w(zx, zy, p)
        values.append(w)
        counts.append(bad)
        if store is not None and cached is None:
            kept.append(zy)
    if store is not None and cached is None:
        store[key] = (chunk, kept)
    per = torch.cat(values).cpu().numpy()               # the one read-back: L doubles and L counts
    nonfinite = int(torch.cat(counts).to(torch.int64).sum().cpu())
    out = sliced_summary(per, p, nonfinite)
    out["swd_seed"] = seed
    if nonfinite > 0:
        warnings.warn(f"sliced_wasserstein_distance: {nonfinite} non-finite projected values (a NaN or an infinity in the "
                      "rows); swd is NaN", RuntimeWarning, stacklevel=2)
    if return_projections:
        out["swd_per_projection"] = per
        out["swd_directions"] = directions
    return out


def _cached_reader(entry, chunk):
    """(lo, hi) -> the reference's sorted projections lo .. hi - 1 from a cache entry (the chunk size it was stored under, its
    chunks); None without an entry.  Another chunking than the stored one reads from one concatenated copy."""
    if entry is None:
        return None
    stored_chunk, chunks = entry
    if stored_chunk == chunk or len(chunks) == 1 and chunk >= chunks[0].shape[0]:
        return lambda lo, hi: chunks[lo // chunk]
    whole = torch.cat(chunks)
    return lambda lo, hi: whole[lo:hi]
