"""The Vendi score (Friedman & Dieng, TMLR 2023; orders q: Pasarkar & Dieng 2023): a reference-free diversity number, "the
effective number of distinct samples" among n rows.

  G        = X X^T, accumulated in f64 (float32 rows are converted on load, which is exact)
  cosine     K_ij = G_ij / (sqrt(G_ii) sqrt(G_jj))
  gaussian   K_ij = exp(-gamma max(G_ii + G_jj - 2 G_ij, 0)),  gamma = 1 / (2 bw^2), the rows as they are (as for KAD)
  K_ii     = 1 exactly; M = K / n is symmetric PSD with trace 1 and eigenvalues lambda_i
  zero rule  eigenvalues <= zero_tol * lambda_max count as zero; rank = the number that remain
  order 1    exp(-sum lambda ln lambda);   order inf: 1 / lambda_max;   other q > 0: (sum lambda^q)^(1 / (1 - q))

The zero rule is part of the definition, not a nicety: for q < 1 a null eigenvalue that comes out as 1e-17 instead of 0
contributes (1e-17)^0.1 = 0.02, and duplicated windows - normal in these sets - make exact null vectors.  zero_tol depends
on the route, because the two eigensolvers resolve null eigenvalues differently:
  "groups"   n <= 128: the per-group kernel (one group), LDS Jacobi, zero_tol = 4 n 2^-52
  "moment"   cosine, n > D: the D x D dual form S = (1 / n) sum x_i x_i^T / |x_i|^2, eigenvalues from am_eigh_sym_f64,
             zero_tol = 1e-10 (that solver's pinned accuracy)
  "gram"     n <= 2048: K / n itself, eigenvalues from am_eigh_sym_f64, zero_tol = 1e-10
A Gaussian kernel on more than 2048 rows has no route here.  The device computes order 1 of the group route itself; every
other order is host arithmetic on the eigenvalues that are read back."""
import math
import types
import warnings

import numpy as np
import torch

from .. import hip_ops as ops
from ._groups import labelled_rows, sort_into_groups
from .kad import _check_bandwidth, _finish_bandwidth, _resolve_bandwidth

ROUTES = ("groups", "moment", "gram")
WHOLE_SET_ZERO_TOL = 1e-10          # am_eigh_sym_f64's pinned accuracy relative to lambda_0 (tests/test_gpu_pca.py: E1)
last_info = {}                      # of the last per-group call: sweeps, residuals and stop codes per group, in label order


def _check_orders(orders):
    try:
        out = tuple(float(q) for q in (orders if np.ndim(orders) else (orders,)))
    except (TypeError, ValueError):
        raise ValueError(f"orders={orders!r} must be positive numbers") from None
    if not out or any(not q > 0.0 for q in out):
        raise ValueError(f"orders={orders!r} must be positive numbers (q > 0; float('inf') is allowed)")
    return out


def _check_kernel(kernel, bandwidth):
    if kernel not in ops.VENDI_KERNELS:
        raise ValueError(f"kernel={kernel!r} must be one of {sorted(ops.VENDI_KERNELS)}")
    if bandwidth is None:
        return None
    bw = float(bandwidth)
    if not math.isfinite(bw) or bw <= 0.0:
        raise ValueError(f"bandwidth={bandwidth!r} must be a finite positive number")
    return bw if kernel == "gaussian" else None


def vendi_from_eigenvalues(lam, orders=(1.0,), zero_tol=0.0):
    """The Vendi scores of the given orders from the eigenvalues of K / n - numpy float64, no GPU.  Eigenvalues <=
    zero_tol * lambda_max are dropped; every sum runs over the rest in descending order.  Returns an array [len(orders)];
    a non-finite eigenvalue gives NaN."""
    orders = _check_orders(orders)
    lam = np.sort(np.asarray(lam, dtype=np.float64).ravel())[::-1]
    if lam.size == 0:
        raise ValueError("no eigenvalues")
    if not np.isfinite(lam).all():
        return np.full(len(orders), np.nan)
    keep = lam[lam > float(zero_tol) * lam[0]]
    if keep.size == 0:
        return np.full(len(orders), np.nan)
    out = np.empty(len(orders))
    for i, q in enumerate(orders):
        if q == 1.0:
            out[i] = math.exp(-np.cumsum(keep * np.log(keep))[-1])
        elif math.isinf(q):
            out[i] = 1.0 / keep[0]
        else:
            out[i] = np.cumsum(keep ** q)[-1] ** (1.0 / (1.0 - q))
    return out


def _stored_rows(x, what):
    """(the rows of x - a 2-D tensor or an AudioMetricsData with stored rows -, the set object a bandwidth cache may live
    on or None); no device call."""
    if torch.is_tensor(x):
        rows, owner = x, None
    else:
        rows, owner = getattr(x, "embeddings", None), x
    if rows is None or rows.dim() != 2 or rows.shape[0] == 0:
        raise ValueError(f"{what} scores the rows of its first argument, which is empty or keeps none "
                         f"(shape {tuple(rows.shape) if rows is not None else None})")
    return rows, owner


def _width(kernel, bw, rows, owner):
    """The keyword arguments of the kernel width for the hip_ops calls, and what is needed to report the bandwidth after the
    read-back: (kwargs, state).  bandwidth=None under the Gaussian kernel is the median pairwise distance of the rows
    themselves - through the reference-side cache of KAD when x is a set, so either fills it for the other."""
    if kernel != "gaussian":
        return {}, None
    if bw is not None:
        return {"gamma": 1.0 / (2.0 * bw * bw)}, (None, bw, None, None)
    if owner is None:
        bw2_dev = ops.pairwise_select_sq(rows)
        return {"gamma_dev": bw2_dev}, (None, None, None, bw2_dev)
    cache, _, gamma, bw2_dev = _resolve_bandwidth(None, owner, rows)
    return {"gamma_dev": bw2_dev}, (cache, None, gamma, bw2_dev)


def _check_median_rows(kernel, bw, n):
    if kernel == "gaussian" and bw is None and n < 2:
        raise ValueError("bandwidth=None takes the median pairwise distance of the rows, which needs at least 2 rows")


def _bandwidth_tail(state, device):
    """one more double for the read-back: the device's median squared distance, or 0"""
    if state is not None and state[3] is not None:
        return state[3].to(torch.float64).reshape(1)
    return torch.zeros(1, dtype=torch.float64, device=device)


def _report_bandwidth(state, bw2_v):
    if state is None:
        return None
    cache, bw, gamma, bw2_dev = state
    if bw2_dev is None:
        return bw
    if cache is not None:
        return _finish_bandwidth(cache, bw, gamma, bw2_dev, bw2_v, None)
    _check_bandwidth(bw2_v)
    return math.sqrt(bw2_v)


def _choose_route(route, kernel, n, d):
    cap_g, cap_m = ops.vendi_groups_max_rows(), ops.vendi_gram_max_rows()
    if route is not None and route not in ROUTES:
        raise ValueError(f"route={route!r} must be None or one of {ROUTES}")
    if route is None:
        if n <= cap_g:
            route = "groups"
        elif kernel == "cosine" and (n > d or n > cap_m):
            route = "moment"
        else:
            route = "gram"
    if route == "groups" and n > cap_g:
        raise ValueError(f"route='groups' takes at most {cap_g} rows, got {n}")
    if route == "moment" and kernel != "cosine":
        raise ValueError("route='moment' is the cosine kernel's dual form; the Gaussian kernel has none")
    if route == "gram" and n > cap_m:
        raise ValueError(f"the {kernel} kernel on {n} rows: the Gram route is capped at {cap_m} rows"
                         + (" and the Gaussian kernel has no other route" if kernel == "gaussian" else ""))
    return route


def vendi_score(x, kernel="cosine", orders=(1.0,), bandwidth=None, route=None, return_eigenvalues=False):
    """The Vendi score of the rows of x (an AudioMetricsData with stored rows, or a float32 / float64 device tensor
    [n, D]).  kernel: "cosine" or "gaussian" (bandwidth=None: the median pairwise distance of the rows; a number fixes it).
    orders: the orders q > 0 to report (float('inf') allowed).  route: None picks "groups" for n <= 128, "moment" for the
    cosine kernel with n > D, else "gram" (n <= 2048); a name forces one.  Returns {"vendi": the order-1 score,
    "vendi_orders": orders, "vendi_per_order": f64 [len(orders)], "vendi_rank": int, "vendi_kernel", "vendi_route",
    "vendi_bandwidth": float or None}, plus "vendi_eigenvalues" (descending, those the zero rule drops as 0.0) when asked.
    A row of zero norm (cosine) or with a non-finite element gives NaN scores, rank 0 and one RuntimeWarning."""
    bw = _check_kernel(kernel, bandwidth)
    orders = _check_orders(orders)
    rows, owner = _stored_rows(x, "vendi_score")
    n, d = int(rows.shape[0]), int(rows.shape[1])
    route = _choose_route(route, kernel, n, d)
    _check_median_rows(kernel, bw, n)
    rows = ops.as_rows(rows)
    width, state = _width(kernel, bw, rows, owner)
    if route == "groups":
        rec, evals, check = ops.vendi_groups(rows, None, [0, n], kernel, **width)
        flat = torch.cat([rec.reshape(-1), evals, _bandwidth_tail(state, rows.device)]).cpu().numpy()     # the one read-back
        check()
        rec_h, lam, bw2_v = flat[:8], flat[8:8 + n].copy(), float(flat[-1])
        stop = int(rec_h[6])
        if stop == 2:
            raise ops._lib.HipLibraryError(f"vendi_score: the Jacobi sweeps did not converge ({int(rec_h[4])} sweeps, residual {rec_h[5]:.3g})")
        bad = stop == 4
        if not bad:
            per_order = np.array([rec_h[0] if q == 1.0 else vendi_from_eigenvalues(lam, (q,), 0.0)[0] for q in orders])
            vendi_1, rank = float(rec_h[0]), int(rec_h[2])
    else:
        if route == "gram":
            mat, check = ops.vendi_gram(rows, None, kernel, **width)
        else:
            mat, check = ops.vendi_moment(rows)
        bad_row = check()                                     # in front of the solver, which refuses a non-finite matrix
        evals, _ = ops.eigh_descending(mat)
        flat = torch.cat([evals, _bandwidth_tail(state, rows.device)]).cpu().numpy()
        lam, bw2_v = flat[:-1][:min(n, flat.size - 1)].copy(), float(flat[-1])
        bad = bad_row is not None
        if not bad:
            keep = lam > WHOLE_SET_ZERO_TOL * lam[0]
            lam = np.where(keep, lam, 0.0)
            rank = int(keep.sum())
            per_order = vendi_from_eigenvalues(lam, orders, 0.0)
            vendi_1 = float(per_order[orders.index(1.0)]) if 1.0 in orders else float(vendi_from_eigenvalues(lam, (1.0,), 0.0)[0])
    bw_out = _report_bandwidth(state, bw2_v)
    if bad:
        warnings.warn("vendi_score: a row has zero norm (cosine kernel) or a non-finite element: the score is NaN",
                      RuntimeWarning, stacklevel=2)
        per_order, vendi_1, rank, lam = np.full(len(orders), np.nan), float("nan"), 0, np.full(lam.shape, np.nan)
    out = {"vendi": vendi_1, "vendi_orders": orders, "vendi_per_order": per_order, "vendi_rank": rank, "vendi_kernel": kernel,
           "vendi_route": route, "vendi_bandwidth": bw_out}
    if return_eigenvalues:
        out["vendi_eigenvalues"] = lam
    return out


def vendi_score_per_group(x, groups, kernel="cosine", orders=(1.0,), bandwidth=None):
    """The Vendi score of every group of x's rows, each on its own ("how different are the generations of this prompt from
    each other?").  `groups`: one integer label per row (numpy or torch, any order, any values); x as vendi_score takes it.
    One library call for all groups, no gathered copy; a group of more than 128 rows raises ValueError naming its label -
    there is no second route.  bandwidth=None under the Gaussian kernel: the median pairwise distance of ALL rows of x, one
    width for every group.  Returns {"vendi_per_group": f64 [B] (one order) or [len(orders), B], "vendi_rank_per_group":
    int64 [B], "vendi_entropy_per_group": f64 [B], "group_labels": [B] ascending, "group_sizes": int64 [B], "vendi_orders",
    "vendi_kernel", "vendi_bandwidth"}; last_info carries "sweeps", "resids" and "stops" per group.  A group with a row of
    zero norm (cosine) or a non-finite element gets NaN (rank 0) and the call one RuntimeWarning; no other group is
    affected."""
    bw = _check_kernel(kernel, bandwidth)
    orders = _check_orders(orders)
    if torch.is_tensor(x):
        owner, holder = None, types.SimpleNamespace(embeddings=x if x.dim() == 2 else None, store_embeddings=True)
    else:
        owner = holder = x
    rows, n, labels = labelled_rows(holder, groups, "vendi_score_per_group", "its first argument")
    order, _, group_labels, sizes = sort_into_groups(labels.to(rows.device, torch.int64))
    cap = ops.vendi_groups_max_rows()
    if (sizes > cap).any():
        g = int(np.flatnonzero(sizes > cap)[0])
        raise ValueError(f"group {int(group_labels[g])} holds {int(sizes[g])} rows; vendi_score_per_group takes groups of at most "
                         f"{cap} rows (score a larger set with vendi_score)")
    _check_median_rows(kernel, bw, n)
    rows = ops.as_rows(rows)
    width, state = _width(kernel, bw, rows, owner)
    offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    rec, evals, check = ops.vendi_groups(rows, order, offs, kernel, **width)
    nb = len(sizes)
    flat = torch.cat([rec.reshape(-1), evals, _bandwidth_tail(state, rows.device)]).cpu().numpy()         # the one read-back
    check()
    rec_h, lam, bw2_v = flat[:8 * nb].reshape(nb, 8), flat[8 * nb:8 * nb + n], float(flat[-1])
    bw_out = _report_bandwidth(state, bw2_v)
    stops = rec_h[:, 6].astype(np.int64)
    last_info.clear()
    last_info.update(sweeps=rec_h[:, 4].astype(np.int64).tolist(), resids=rec_h[:, 5].tolist(), stops=stops.tolist(),
                     group_labels=group_labels.tolist(), group_sizes=sizes.tolist())
    capped = np.flatnonzero(stops == 2)
    if len(capped):
        raise ops._lib.HipLibraryError(f"vendi_score_per_group: the Jacobi sweeps of group {int(group_labels[capped[0]])} did not converge "
                                       f"(groups with stop code 2: {group_labels[capped].tolist()})")
    bad = stops == 4
    scores = np.empty((len(orders), nb))
    for i, q in enumerate(orders):
        if q == 1.0:
            scores[i] = rec_h[:, 0]
        else:
            scores[i] = [np.nan if bad[g] else vendi_from_eigenvalues(lam[offs[g]:offs[g + 1]], (q,), 0.0)[0] for g in range(nb)]
    scores[:, bad] = np.nan
    if bad.any():
        warnings.warn(f"vendi_score_per_group: {int(bad.sum())} of {nb} groups hold a row of zero norm (cosine kernel) or with a "
                      "non-finite element; their score is NaN", RuntimeWarning, stacklevel=2)
    return {"vendi_per_group": scores[0] if len(orders) == 1 else scores, "vendi_rank_per_group": rec_h[:, 2].astype(np.int64),
            "vendi_entropy_per_group": rec_h[:, 1].copy(), "group_labels": group_labels, "group_sizes": sizes, "vendi_orders": orders,
            "vendi_kernel": kernel, "vendi_bandwidth": bw_out}
