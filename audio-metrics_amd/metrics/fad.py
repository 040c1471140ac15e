"""Frechet distance on the device (reference src/audio_metrics/metrics/fad.py:8-31)."""
import numpy as np
import torch

from .. import hip_ops as ops
from ..data import AudioMetricsData, ensure_tensor
from ._groups import labelled_rows, sort_into_groups

NS_MAX_ITER = 64
NS_TOL = 1e-13

FAD_INF_STEPS = 15       # subset sizes of the extrapolation (Chong & Forster, CVPR 2020: 15 points ...
FAD_INF_MIN_N = 5000     # ... from 5000 rows to the whole set, evenly spaced)

last_info = {}     # iterations / residual of the most recent call (diagnostics)

RANK_DEFICIENT_NOTE = (
    "Frechet distance of a set with no more rows than dimensions ({n} rows, {d} dimensions) from float32 statistics: the "
    "reference's own value here contains the square roots of the rounding dust its float32 torch.cov leaves in the null space "
    "(fad.py:30) - it moves by up to 1.5e-4 relative with the batch size of its add() calls and by 2.6e-4 ... 3.6e-4 between "
    "float32 and float64 rows.  This build returns the dust-free value (= the reference fed float64 rows, to 1e-7); expect up "
    "to 4e-4 relative deviation from what the reference prints for float32 rows.")


def warn_if_rank_deficient(n_x, n_y, d, rows_dtype=None):
    """One RuntimeWarning per call where the reference's float32 result is not defined to 1e-4 (not silently).
    rows_dtype = dtype of the rows the statistics came from, when known: float64 rows carry no such dust."""
    import warnings
    if rows_dtype == torch.float64 or n_x is None or n_y is None:
        return
    n = min(int(n_x), int(n_y))
    if 1 < n <= int(d):
        warnings.warn(RANK_DEFICIENT_NOTE.format(n=n, d=int(d)), RuntimeWarning, stacklevel=3)


def frechet_distance(x: AudioMetricsData, y: AudioMetricsData, device=None):
    dtypes = {getattr(x, "stats_rows_dtype", None), getattr(y, "stats_rows_dtype", None)}
    warn_if_rank_deficient(getattr(x, "n", None), getattr(y, "n", None), ensure_tensor(x.mean).numel(),
                           torch.float64 if dtypes == {torch.float64} else None)
    return _frechet_distance(x.mean, x.cov, y.mean, y.cov, device=device)


def _frechet_distance(mu_x, sigma_x, mu_y, sigma_y, device=None) -> float:
    """|mu_x-mu_y|^2 + tr(sigma_x) + tr(sigma_y) - 2 tr sqrt(sigma_x sigma_y), f64.
    ``device`` selects the MI355X to run on (the reference's optional kwarg,
    fad.py:24-27); host tensors are uploaded."""
    if device is None:
        device = next((t.device for t in (mu_x, sigma_x, mu_y, sigma_y)
                       if isinstance(t, torch.Tensor) and t.is_cuda), None)
    if device is None:
        from ..data import default_device
        device = default_device()
    mu_x, sigma_x, mu_y, sigma_y = (ensure_tensor(t).to(device, torch.float64) for t in (mu_x, sigma_x, mu_y, sigma_y))
    res = ops.frechet(mu_x, sigma_x, mu_y, sigma_y, NS_MAX_ITER, NS_TOL)
    last_info.clear()
    last_info.update(res)
    return res["fd"]


# ------------------------------------------------------------------ FAD-infinity
def fad_inf_subset_indices(n, sizes, seed, device):
    """One random subset of range(n) per entry of `sizes`, each drawn WITHOUT replacement and independently of the others:
    the leading sizes[b] entries of a device-side permutation from a generator seeded with `seed` (reproducible per seed,
    device and sizes; no host work in front of the kernels).  Returns (idx, offsets): the subsets concatenated in one int64
    device tensor, and the B + 1 host offsets of am_stats_gather_f32."""
    device = torch.device(device)
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    offsets = [0]
    for m in sizes:
        if not 1 <= int(m) <= int(n):
            raise ValueError(f"subset size {int(m)} outside [1, {int(n)}]")
        offsets.append(offsets[-1] + int(m))
    idx = torch.empty(offsets[-1], dtype=torch.int64, device=device)
    for b, m in enumerate(sizes):
        idx[offsets[b]:offsets[b + 1]] = torch.randperm(int(n), generator=gen, device=device)[:int(m)]
    return idx, offsets


def fit_inverse_n(sizes, values):
    """Ordinary least squares values_i ~ slope / sizes_i + intercept in f64 on the host: (intercept, slope, r2)."""
    sizes = np.asarray(sizes, dtype=np.float64)
    values = np.asarray(values, dtype=np.float64)
    design = np.stack([1.0 / sizes, np.ones_like(sizes)], axis=1)
    (slope, intercept), *_ = np.linalg.lstsq(design, values, rcond=None)
    ss_res = float(np.sum((values - design @ np.array([slope, intercept])) ** 2))
    ss_tot = float(np.sum((values - values.mean()) ** 2))
    r2 = 1.0 - ss_res / ss_tot if ss_tot > 0.0 else float("nan")
    return float(intercept), float(slope), r2


def frechet_distance_inf(x: AudioMetricsData, y: AudioMetricsData, steps=FAD_INF_STEPS, min_n=FAD_INF_MIN_N, seed=0, device=None):
    """Sample-size-extrapolated Frechet distance (Chong & Forster, "Effectively Unbiased FID and Inception Score", CVPR
    2020): the distance of `steps` random subsets of x's stored rows (sizes evenly spaced from min_n to all of them)
    against y's full-set statistics, fitted as slope / n + intercept; the intercept is the value at infinite sample size.
    The subsets' statistics come from ONE gathered-statistics call on the stored matrix and their distances from ONE
    batched solve.  Returns {"fad_inf", "fad_inf_slope", "fad_inf_r2"}; last_info carries the per-subset figures."""
    rows = getattr(x, "embeddings", None)
    n = int(rows.shape[0]) if rows is not None else (0 if getattr(x, "n", None) is None else int(x.n))
    if int(steps) < 2:
        raise ValueError(f"frechet_distance_inf needs at least 2 subset sizes to fit a line (steps={steps})")
    if int(min_n) < 2 or int(min_n) > n:
        raise ValueError(f"min_n={min_n} must lie in [2, {n}] (the subsampled set holds {n} rows)")
    if rows is None:
        raise ValueError(f"frechet_distance_inf subsamples the stored rows of its first argument, which keeps none "
                         f"(n={n}, store_embeddings={getattr(x, 'store_embeddings', None)})")
    steps, min_n = int(steps), int(min_n)
    d = int(rows.shape[1])
    sizes = np.linspace(min_n, n, steps).round().astype(int)
    warn_if_rank_deficient(int(sizes[0]), getattr(y, "n", None), d,
                           torch.float64 if rows.dtype == torch.float64 and getattr(y, "stats_rows_dtype", None) == torch.float64 else None)
    if device is None:
        device = rows.device if rows.is_cuda else None
    if device is None:
        from ..data import default_device
        device = default_device()
    device = torch.device(device)
    rows = ops.as_rows(rows.to(device))
    mu_y, cov_y = (ensure_tensor(t).to(device, torch.float64) for t in (y.mean, y.cov))
    idx, offsets = fad_inf_subset_indices(n, sizes, seed, device)
    means, covs, check = ops.stats_gather(rows, idx, offsets, defer_check=True)
    res = ops.frechet_batch(means, covs, mu_y.reshape(-1), cov_y, NS_MAX_ITER, NS_TOL)
    check()
    fads = [r["fd"] for r in res]
    intercept, slope, r2 = fit_inverse_n(sizes, fads)
    last_info.clear()
    last_info.update(sizes=[int(m) for m in sizes], fads=fads, iters=[r["iters"] for r in res], stops=[r["stop"] for r in res],
                     resids=[r["resid"] for r in res], seed=int(seed))
    return {"fad_inf": intercept, "fad_inf_slope": slope, "fad_inf_r2": r2}


# ------------------------------------------------------------------ per-group ("per-song") Frechet distance
def frechet_distance_per_group(x: AudioMetricsData, y: AudioMetricsData, groups, device=None):
    """Frechet distance of every group of x's stored rows, each on its own, against y's full-set statistics (the
    "individual" / per-song score of the evaluation toolkits).  `groups`: one integer label per stored row of x (numpy or
    torch, any order, any values).  Groups of up to hip_ops.frechet_groups_max_rows() rows take the dual form - the
    eigenvalues of the n x n matrix Xc cov_y Xc^T / (n - 1), one library call for all of them, no covariance per group;
    larger groups take the gathered statistics and the batched Newton-Schulz solve, in chunks of groups.  Returns
    {"fad_per_group": f64 [B], "group_labels": [B] ascending, "group_sizes": int64 [B]}; last_info carries, per group in
    label order, "routes" ("dual" / "batch"), "sweeps" (Jacobi sweeps; None on the batch route), "iters" (Newton-Schulz
    iterations; None on the dual route), "resids" and "stops".  A group whose solve did not end well raises HipLibraryError
    naming its label: on the dual route any stop code other than 1 (2 = sweep cap, 4 = non-finite input); on the batch
    route the codes of am_frechet_batch_f64 that are no result - 0 (iteration cap reached) and 4 (non-finite product) -
    while its other stopping rules (1 converged, 2 trace stalled, 3 zero product) are regular ends there; a non-finite value
    raises on either route.  The dual form is
    the dust-free definition for a group with fewer rows than dimensions, so no rank-deficiency warning is raised here."""
    rows, n, labels = labelled_rows(x, groups, "frechet_distance_per_group", "its first argument")
    d = int(rows.shape[1])
    d_y = int(ensure_tensor(y.mean).numel())
    if d_y != d:
        raise ValueError(f"feature widths differ: the rows have {d} columns, the reference statistics {d_y}")
    if device is None:
        device = rows.device if rows.is_cuda else None
    if device is None:
        from ..data import default_device
        device = default_device()
    device = torch.device(device)
    rows = ops.as_rows(rows.to(device))
    mu_y, cov_y = (ensure_tensor(t).to(device, torch.float64) for t in (y.mean, y.cov))
    mu_y = mu_y.reshape(-1)
    order, counts, group_labels, sizes = sort_into_groups(labels.to(device, torch.int64))
    nb = len(sizes)
    cap = ops.frechet_groups_max_rows()
    small = sizes <= cap
    if small.all():
        idx_small, idx_large = order, None
    else:
        on_dev = torch.repeat_interleave(torch.as_tensor(small, device=device), counts)
        idx_small, idx_large = order[on_dev], order[~on_dev]
    fads = np.empty(nb, dtype=np.float64)
    steps, resids, stops = np.zeros(nb, dtype=np.int64), np.zeros(nb), np.zeros(nb, dtype=np.int64)
    rec_small = check_small = None
    if small.any():
        offs = np.concatenate([[0], np.cumsum(sizes[small])])
        rec_small, check_small = ops.frechet_groups(rows, idx_small, offs.tolist(), mu_y, cov_y)
    large = np.flatnonzero(~small)
    if len(large):
        per_set = max(int(ops._lib.load().am_frechet_batch_workspace_bytes(1, d)), 1)
        chunk = max(1, min(65535, ops.FRECHET_BATCH_WS_CAP // per_set))
        offs = np.concatenate([[0], np.cumsum(sizes[large])])
        for c0 in range(0, len(large), chunk):
            c1 = min(len(large), c0 + chunk)
            means, covs, check = ops.stats_gather(rows, idx_large[offs[c0]:offs[c1]], (offs[c0:c1 + 1] - offs[c0]).tolist(),
                                                  defer_check=True)
            rec_large = torch.empty((c1 - c0, 5), dtype=torch.float64, device=device)
            try:
                ops.frechet_batch(means, covs, mu_y, cov_y, NS_MAX_ITER, NS_TOL, out=rec_large)
            except ops._lib.HipLibraryError:                  # a stop code 4 in the chunk: every record is written all the same,
                pass                                          # and the group is named by its label below
            check()
            rec = rec_large.cpu().numpy()
            where = large[c0:c1]
            fads[where], steps[where], resids[where], stops[where] = rec[:, 0], rec[:, 2].astype(np.int64), rec[:, 3], rec[:, 4].astype(np.int64)
    if rec_small is not None:
        rec = rec_small.cpu().numpy()
        check_small()
        where = np.flatnonzero(small)
        fads[where], steps[where], resids[where], stops[where] = rec[:, 0], rec[:, 2].astype(np.int64), rec[:, 3], rec[:, 4].astype(np.int64)
    routes = ["dual" if s else "batch" for s in small]
    last_info.clear()
    last_info.update(sweeps=[int(v) if s else None for v, s in zip(steps, small)],
                     iters=[None if s else int(v) for v, s in zip(steps, small)], resids=resids.tolist(), stops=stops.tolist(), routes=routes,
                     group_labels=group_labels.tolist(), group_sizes=sizes.tolist())
    bad = [g for g in range(nb) if (stops[g] != 1 if small[g] else stops[g] in (0, 4)) or not np.isfinite(fads[g])]
    if bad:
        g = bad[0]
        raise ops._lib.HipLibraryError(f"frechet_distance_per_group: group with label {int(group_labels[g])} ({int(sizes[g])} rows, "
                                       f"{routes[g]} route) ended with stop code {int(stops[g])} "
                                       f"(labels of all such groups: {[int(group_labels[i]) for i in bad]})")
    return {"fad_per_group": fads, "group_labels": group_labels, "group_sizes": sizes}
