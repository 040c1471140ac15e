"""Debiased Sinkhorn divergence (Feydy et al., AISTATS 2019: "Interpolating between optimal transport and MMD using Sinkhorn
divergences"; the algorithm of GeomLoss): entropic optimal transport between the two sets AS THEY ARE - no Gaussian fitted
to them (FAD is the 2-Wasserstein distance between two fitted Gaussians), no kernel bandwidth.  The reference has no such
function.

  cost      C(a, b) = d2(a, b) / 2,  d2 = max(fmaf(-2, <a, b>, |a|^2 + |b|^2), 0) in f32: the bits of knn_search(squared=True)
  soft-min  T_eps(Y, g)(x_i) = -eps log((1 / m) sum_j exp((g_j - C(x_i, y_j)) / eps))      ops.softmin: one Gram sweep over
            recomputed 128 x 128 tiles with a log-sum-exp epilogue, no n x m matrix; uniform weights 1 / n and 1 / m
  schedule  eps_0 = diam2 = sum_k (max_k - min_k)^2 (the squared bounding-box diagonal), eps_{t+1} = eps_t scaling^2 while
            that stays above blur^2, then one last entry blur^2                            sinkhorn_schedule

Three independent solves, each from zero potentials: one step per schedule entry, then further steps at blur^2 until
max |change| <= rtol max |potential| or until max_iter steps in all.
  XY  alternating:  f <- T(Y, g)(X), then g <- T(X, f)(Y) with the new f;  f* = T(Y, g)(X) and g* = T(X, f)(Y) both from the
      last (f, g);  OT_xy = mean f* + mean g*
  XX  symmetric and averaged:  p <- (p + T(X, p)(X)) / 2;  p* = T(X, p)(X);  OT_xx = 2 mean p*
  YY  the same on the reference: q*, OT_yy = 2 mean q*

  S = OT_xy - OT_xx / 2 - OT_yy / 2 = mean(f* - p*) + mean(g* - q*),     sinkhorn_w2 = sqrt(2 max(S, 0))
in the units of the embeddings.  The steps of the eps-scaling read nothing back; a step at the final blur^2 reads back two
scalars.  The YY solve depends on the reference rows alone and is kept on the reference set beside the KAD cache."""
import math
import struct
import warnings

import torch

from .. import hip_ops as ops
from .kad import _check_bandwidth, _resolve_bandwidth, reference_cache


def sinkhorn_schedule(diam2, blur, scaling):
    """The temperatures of one solve, a list of floats: diam2, diam2 scaling^2, diam2 scaling^4, ... while above blur^2, then
    blur^2 (a diam2 that is not above blur^2 leaves the one entry blur^2).  Host arithmetic, repeated multiplication in f64."""
    diam2, blur, scaling = float(diam2), float(blur), float(scaling)
    if not math.isfinite(diam2) or diam2 < 0.0:
        raise ValueError(f"diam2={diam2!r} must be finite and not negative")
    if not math.isfinite(blur) or blur <= 0.0:
        raise ValueError(f"blur={blur!r} must be a finite positive number")
    if not 0.0 < scaling < 1.0:
        raise ValueError(f"scaling={scaling!r} must lie in (0, 1)")
    last = blur * blur
    if last <= 0.0 or not math.isfinite(last):
        raise ValueError(f"blur={blur!r}: blur^2 is not a positive float64 number")
    out, eps, ratio = [], diam2, scaling * scaling
    while eps > last:
        out.append(eps)
        eps *= ratio
    out.append(last)
    return out


def _rows_of(data, name):
    rows = getattr(data, "embeddings", None)
    if rows is None or rows.shape[0] == 0:
        raise ValueError(f"sinkhorn_divergence needs the stored rows of its {name} set, which keeps none "
                         f"(store_embeddings={getattr(data, 'store_embeddings', None)})")
    return rows


def _box(rows):
    """(column minima, column maxima) as float64 device vectors."""
    return rows.amin(dim=0).to(torch.float64), rows.amax(dim=0).to(torch.float64)


def _diam2(lo, hi):
    return ((hi - lo) ** 2).sum()


def _read(*scalars):
    return torch.stack(scalars).cpu().tolist()


def _solve_self(rows, schedule, rtol, max_iter):
    """The symmetric, averaged solve of one set against itself: (p*, steps, converged)."""
    p = torch.zeros(rows.shape[0], dtype=torch.float64, device=rows.device)
    steps = 0
    for eps in schedule[:-1]:
        p = ops.softmin(rows, rows, p, eps, prev=p, damping=0.5)[0]
        steps += 1
    eps, converged = schedule[-1], False
    while True:
        p, change, magnitude = ops.softmin(rows, rows, p, eps, prev=p, damping=0.5)
        steps += 1
        c, m = _read(change, magnitude)
        if c <= rtol * m:
            converged = True
            break
        if steps >= max_iter:
            break
    return ops.softmin(rows, rows, p, eps)[0], steps, converged


def _solve_cross(ex, ey, schedule, rtol, max_iter):
    """The alternating solve between the two sets: (f*, g*, f, steps, converged)."""
    f = torch.zeros(ex.shape[0], dtype=torch.float64, device=ex.device)
    g = torch.zeros(ey.shape[0], dtype=torch.float64, device=ex.device)
    steps = 0
    for eps in schedule[:-1]:
        f = ops.softmin(ex, ey, g, eps)[0]
        g = ops.softmin(ey, ex, f, eps)[0]
        steps += 1
    eps, converged = schedule[-1], False
    while True:
        f, cf, mf = ops.softmin(ex, ey, g, eps, prev=f)
        g, cg, mg = ops.softmin(ey, ex, f, eps, prev=g)
        steps += 1
        c, m = _read(torch.maximum(cf, cg), torch.maximum(mf, mg))
        if c <= rtol * m:
            converged = True
            break
        if steps >= max_iter:
            break
    return ops.softmin(ex, ey, g, eps)[0], ops.softmin(ey, ex, f, eps)[0], f, steps, converged


def _key(*numbers):
    return struct.pack("<%dd" % len(numbers), *(float(v) for v in numbers))


def sinkhorn_divergence(x, y, blur=None, blur_factor=0.25, scaling=0.5, rtol=1e-5, max_iter=200, return_potentials=False):
    """The debiased Sinkhorn divergence of candidate set `x` against reference set `y` (stored float32 rows, uniform
    weights).  blur=None: blur_factor times the reference's median pairwise distance (the cached median of
    kernel_audio_distance); a number fixes it, in the units of the embeddings.  Returns {"sinkhorn_divergence": S,
    "sinkhorn_w2": sqrt(2 max(S, 0)), "sinkhorn_ot_xy", "sinkhorn_ot_xx", "sinkhorn_ot_yy", "sinkhorn_blur",
    "sinkhorn_iterations": (xy, xx, yy) steps, "sinkhorn_converged": (xy, xx, yy), "sinkhorn_marginal_error": max_i
    |exp((f_i - f*_i) / blur^2) - 1|, the row-marginal error of the XY plan}; return_potentials=True adds
    "candidate_potential" = f* - p* (float64 numpy [n]) and "reference_potential" = g* - q* ([m]) in stored row order, whose
    means add up to S.  A solve that reaches max_iter gives one RuntimeWarning and converged False.  The reference's own solve
    is cached on `y` and dropped when rows are appended; a cached call returns the bits of an uncached one."""
    ex, ey = _rows_of(x, "candidate"), _rows_of(y, "reference")
    for rows, name in ((ex, "candidate"), (ey, "reference")):
        if rows.dtype == torch.float64:
            raise NotImplementedError(f"sinkhorn_divergence: the {name} set holds float64 rows; softmin takes float32 rows "
                                      "(the float64 matrix-core form is not implemented)")
    if ex.shape[1] != ey.shape[1]:
        raise ValueError(f"feature widths differ: {ex.shape[1]} and {ey.shape[1]}")
    if blur is not None and (not math.isfinite(float(blur)) or float(blur) <= 0.0):
        raise ValueError(f"blur={blur!r} must be a finite positive number")
    if blur is None and (not math.isfinite(float(blur_factor)) or float(blur_factor) <= 0.0):
        raise ValueError(f"blur_factor={blur_factor!r} must be a finite positive number")
    scaling, rtol, max_iter = float(scaling), float(rtol), int(max_iter)
    if not 0.0 < scaling < 1.0:
        raise ValueError(f"scaling={scaling!r} must lie in (0, 1)")
    if max_iter < 1:
        raise ValueError(f"max_iter={max_iter} must be at least 1")
    if not rtol >= 0.0:
        raise ValueError(f"rtol={rtol!r} must not be negative")
    # bounding boxes: of each set for its own solve, of the pooled rows for the cross solve - one read-back, which also
    # tells whether every element is finite (a NaN or an infinity in a column makes its range NaN or infinite)
    same = x is y or ex is ey
    (xlo, xhi), (ylo, yhi) = _box(ex), (_box(ex) if same else _box(ey))
    d_xx, d_yy, d_xy = _read(_diam2(xlo, xhi), _diam2(ylo, yhi), _diam2(torch.minimum(xlo, ylo), torch.maximum(xhi, yhi)))
    if not (math.isfinite(d_xx) and math.isfinite(d_yy) and math.isfinite(d_xy)):
        raise ValueError("sinkhorn_divergence: the rows hold non-finite elements (a NaN or an infinity has no transport cost)")
    if blur is None:
        cache, _, _, bw2_dev = _resolve_bandwidth(None, y, ey)
        if cache.bw2_host is None:
            cache.bw2_host = float(bw2_dev.cpu())
        _check_bandwidth(cache.bw2_host)
        blur = float(blur_factor) * math.sqrt(cache.bw2_host)
    blur = float(blur)

    ex = ops.as_matrix(ex, "x")                         # rows the library can take as they are: converted once, not per step
    ey = ex if same else ops.as_matrix(ey, "y")
    f_star, g_star, f, it_xy, ok_xy = _solve_cross(ex, ey, sinkhorn_schedule(d_xy, blur, scaling), rtol, max_iter)
    p_star, it_xx, ok_xx = _solve_self(ex, sinkhorn_schedule(d_xx, blur, scaling), rtol, max_iter)
    store = reference_cache(y).sinkhorn
    key = _key(blur, scaling, rtol, max_iter, d_yy)
    if key not in store:
        q_star, it_yy, ok_yy = _solve_self(ey, sinkhorn_schedule(d_yy, blur, scaling), rtol, max_iter)
        store[key] = (q_star, q_star.mean(), it_yy, ok_yy)
    q_star, q_mean, it_yy, ok_yy = store[key]

    eps = blur * blur
    marginal = torch.expm1((f - f_star) / eps).abs().max()
    mf, mg, mp, mq, marginal = _read(f_star.mean(), g_star.mean(), p_star.mean(), q_mean, marginal)      # the one read-back of results
    ot_xy, ot_xx, ot_yy = mf + mg, 2.0 * mp, 2.0 * mq
    s = ot_xy - 0.5 * ot_xx - 0.5 * ot_yy
    missed = [name for name, ok in (("XY", ok_xy), ("XX", ok_xx), ("YY", ok_yy)) if not ok]
    if missed:
        warnings.warn(f"sinkhorn_divergence: the {', '.join(missed)} solve{'s' if len(missed) > 1 else ''} did not reach "
                      f"rtol={rtol:g} in max_iter={max_iter} steps", RuntimeWarning, stacklevel=2)
    out = {"sinkhorn_divergence": s, "sinkhorn_w2": math.sqrt(2.0 * max(s, 0.0)), "sinkhorn_ot_xy": ot_xy, "sinkhorn_ot_xx": ot_xx,
           "sinkhorn_ot_yy": ot_yy, "sinkhorn_blur": blur, "sinkhorn_iterations": (it_xy, it_xx, it_yy),
           "sinkhorn_converged": (ok_xy, ok_xx, ok_yy), "sinkhorn_marginal_error": marginal}
    if return_potentials:
        out["candidate_potential"] = (f_star - p_star).cpu().numpy()
        out["reference_potential"] = (g_star - q_star).cpu().numpy()
    return out
