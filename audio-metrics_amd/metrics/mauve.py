"""K-means clustering of stored rows and the MAUVE score (Pillutla et al., NeurIPS 2021; applied to embeddings of generated
music as "MAUVE Audio Divergence" by Huang et al. 2025): pool the candidate and the reference rows, quantise them with
k-means, histogram each set over the clusters and integrate the divergence frontier of the two histograms.

  kmeans     Lloyd iterations on the device: ops.kmeans_assign (the f32 tile engine, no N x K matrix) then
             ops.kmeans_update (f64 means, rounded once), until no label changes; one scalar read back per iteration
  histograms torch.bincount of the labels of each set - the only read-back of mauve_score besides the convergence flags
  frontier   float64 numpy over K bins (mauve_from_histograms, a pure function)

The reference has no clustering and no MAUVE.  The rows are clustered as they are: the PCA step and the normalisation of
the `mauve-text` package are not applied, and agreement with that package's (or faiss's) numbers is not claimed."""
import numpy as np
import torch

from .. import hip_ops as ops
from ..data import AudioMetricsData

MAUVE_SCALING = 5.0
MAUVE_POINTS = 25


def _float32_rows(rows, what, name="rows"):
    if isinstance(rows, AudioMetricsData):
        stored = rows.embeddings
        if stored is None:
            raise ValueError(f"{what} needs the stored rows of its {name}, which keeps none "
                             f"(store_embeddings={getattr(rows, 'store_embeddings', None)})")
        rows = stored
    if not torch.is_tensor(rows):
        raise ValueError(f"{what} takes a device tensor or an AudioMetricsData, got {type(rows).__name__}")
    if rows.dtype == torch.float64:
        raise NotImplementedError(f"{what}: {name} holds float64 rows; the k-means kernels take float32 rows (the float64 "
                                  "matrix-core form is not implemented)")
    if rows.dim() != 2:
        raise ValueError(f"{what}: {name} must be 2-D, got shape {tuple(rows.shape)}")
    return rows


def _check_clusters(what, n_clusters, n_rows):
    k = int(n_clusters)
    if k < 1:
        raise ValueError(f"{what}: n_clusters={n_clusters} must be at least 1")
    if k > n_rows:
        raise ValueError(f"{what}: n_clusters={k} exceeds the number of rows ({n_rows})")
    return k


def _lloyd(x, c, max_iter):
    """One run from the centroids c.  An iteration is an assign and - unless the assign repeated the labels of the one
    before it, which ends the run - an update.  A run that reaches max_iter ends with one more assign, so that labels,
    inertia and centroids belong together; the inertia of every assign stays on the device until the run is over."""
    history, previous, converged, n_iter = [], None, False, 0
    while n_iter < max_iter:
        labels, _, inertia = ops.kmeans_assign(x, c)
        history.append(inertia)
        n_iter += 1
        if previous is not None and bool(torch.equal(labels, previous)):       # the read-back of the iteration: one scalar
            converged = True
            break
        c, _ = ops.kmeans_update(x, labels, c)
        previous = labels
    if not converged:
        labels, _, inertia = ops.kmeans_assign(x, c)
        history.append(inertia)
    counts = torch.bincount(labels + 1, minlength=c.shape[0] + 1)[1:]          # (a label of -1 counts nowhere)
    history = [float(v) for v in torch.stack(history).cpu().tolist()]
    return {"centroids": c, "labels": labels, "counts": counts, "inertia": history[-1], "inertia_history": history,
            "n_iter": n_iter, "converged": converged}


def kmeans(rows, n_clusters, max_iter=100, n_init=1, seed=0, init=None):
    """Lloyd's k-means of float32 rows (a device tensor, or an AudioMetricsData with stored rows) into n_clusters clusters.
    Initial centroids: n_clusters distinct rows drawn by a CPU torch.Generator seeded with `seed` (restart r of n_init:
    seed + r), or the [n_clusters, D] tensor `init`.  Returns {"centroids": float32 [K, D] and "labels": int64 [N] on the
    device, "counts": int64 [K] on the device, "inertia": float, "inertia_history": one float per assign, "n_iter": assigns
    run before the stop (a run that did not converge has one closing assign more in its history), "converged": whether the
    run stopped because no label changed}; n_init > 1 keeps the run with the lowest inertia.  Ties go to the smallest
    centroid index, a cluster that loses all its rows keeps its centroid, and two runs with the same arguments return the
    same bits."""
    x = _float32_rows(rows, "kmeans")
    n = int(x.shape[0])
    k = _check_clusters("kmeans", n_clusters, n)
    max_iter, n_init = int(max_iter), int(n_init)
    if max_iter < 1 or n_init < 1:
        raise ValueError(f"kmeans: max_iter={max_iter} and n_init={n_init} must be at least 1")
    if init is not None:
        if not torch.is_tensor(init) or init.dim() != 2 or tuple(init.shape) != (k, x.shape[1]):
            raise ValueError(f"kmeans: init must be a [{k}, {x.shape[1]}] tensor, got "
                             f"{tuple(getattr(init, 'shape', ()))}")
        if init.dtype == torch.float64:
            raise NotImplementedError("kmeans: init holds float64 rows; the k-means kernels take float32 rows")
    if not bool(torch.isfinite(x).all()):
        raise ValueError("kmeans: the rows hold non-finite elements (a NaN or an infinity has no nearest centroid)")
    if x.dtype != torch.float32:
        x = x.to(torch.float32)
    best = None
    for r in range(1 if init is not None else n_init):
        if init is not None:
            c = init.to(device=x.device, dtype=torch.float32)
        else:
            gen = torch.Generator(device="cpu")
            gen.manual_seed(int(seed) + r)
            c = x[torch.randperm(n, generator=gen)[:k].to(x.device)]
        run = _lloyd(x, c, max_iter)
        if best is None or run["inertia"] < best["inertia"]:
            best = run
    return best


def _kl(a, b):
    """sum a log(a / b) with 0 log 0 = 0 (b > 0 wherever a > 0)."""
    keep = a > 0
    return float(np.sum(a[keep] * np.log(a[keep] / b[keep])))


def mauve_from_histograms(p_counts, q_counts, scaling=MAUVE_SCALING, n_points=MAUVE_POINTS, return_points=False):
    """The MAUVE score of two histograms over the same bins, float64 on the host:  p = p_counts / sum, q = q_counts / sum;
    for lambda in linspace(1e-6, 1 - 1e-6, n_points) the mixture r = lambda p + (1 - lambda) q (formed as
    q + lambda (p - q), which is q itself when p == q) gives the frontier point
    (x, y) = (exp(-s KL(q || r)), exp(-s KL(p || r))) with the natural logarithm and 0 log 0 = 0; with the end points (0, 1)
    and (1, 0) the score is the mean of the trapezoid area of y over x and of x over y.  1.0 for equal histograms, towards
    0 as they separate; symmetric in p and q.  return_points=True: (score, float64 [n_points + 2, 2] points sorted by x)."""
    p = np.asarray(p_counts, dtype=np.float64).ravel()
    q = np.asarray(q_counts, dtype=np.float64).ravel()
    if p.shape != q.shape or p.size < 1:
        raise ValueError(f"the histograms must have the same bins (got {p.size} and {q.size})")
    if np.any(p < 0) or np.any(q < 0) or not (np.isfinite(p).all() and np.isfinite(q).all()) or p.sum() <= 0 or q.sum() <= 0:
        raise ValueError("the histograms must hold finite non-negative counts with a positive total")
    n_points = int(n_points)
    if n_points < 1 or not (float(scaling) > 0.0 and np.isfinite(scaling)):
        raise ValueError(f"n_points={n_points} must be at least 1 and scaling={scaling!r} a finite positive number")
    p, q = p / p.sum(), q / q.sum()
    pts = [(0.0, 1.0), (1.0, 0.0)]
    for lam in np.linspace(1e-6, 1.0 - 1e-6, n_points):
        r = q + lam * (p - q)
        pts.append((np.exp(-scaling * _kl(q, r)), np.exp(-scaling * _kl(p, r))))
    pts = np.array(pts, dtype=np.float64)
    by_x = pts[np.lexsort((-pts[:, 1], pts[:, 0]))]
    by_y = pts[np.lexsort((-pts[:, 0], pts[:, 1]))]
    a1 = float(np.sum(np.diff(by_x[:, 0]) * 0.5 * (by_x[1:, 1] + by_x[:-1, 1])))
    a2 = float(np.sum(np.diff(by_y[:, 1]) * 0.5 * (by_y[1:, 0] + by_y[:-1, 0])))
    score = 0.5 * (a1 + a2)
    return (score, by_x) if return_points else score


def mauve_score(cand: AudioMetricsData, ref: AudioMetricsData, n_clusters=None, max_iter=100, n_init=1, seed=0,
                scaling=MAUVE_SCALING, n_points=MAUVE_POINTS, return_details=False):
    """MAUVE of the candidate set against the reference set: the stored rows of both are pooled (candidate first) and
    clustered by kmeans into n_clusters clusters (default max(2, min(n, m) // 10)); the two label histograms go through
    mauve_from_histograms.  Returns {"mauve": the score in (0, 1], "mauve_n_clusters", "mauve_kmeans_iterations",
    "mauve_kmeans_inertia"}; return_details=True adds "mauve_points" (the frontier), "mauve_hist_candidate",
    "mauve_hist_reference" (int64 numpy) and "mauve_labels_candidate", "mauve_labels_reference" (int64 device tensors).
    The rows are clustered as they are - no PCA, no normalisation - and the score is MAUVE itself, without the rescaling
    of the MAD paper."""
    ex = _float32_rows(cand, "mauve_score", "the candidate set")
    ey = _float32_rows(ref, "mauve_score", "the reference set")
    if ex.shape[1] != ey.shape[1]:
        raise ValueError(f"feature widths differ: {ex.shape[1]} and {ey.shape[1]}")
    n, m = int(ex.shape[0]), int(ey.shape[0])
    if n < 1 or m < 1:
        raise ValueError(f"mauve_score needs rows in both sets (got {n} and {m})")
    k = _check_clusters("mauve_score", max(2, min(n, m) // 10) if n_clusters is None else n_clusters, n + m)
    pooled = torch.cat([ex.to(torch.float32), ey.to(torch.float32)], dim=0)
    run = kmeans(pooled, k, max_iter=max_iter, n_init=n_init, seed=seed)
    lc, lr = run["labels"][:n], run["labels"][n:]
    hist = torch.stack([torch.bincount(lc, minlength=k), torch.bincount(lr, minlength=k)]).cpu().numpy()
    score, points = mauve_from_histograms(hist[0], hist[1], scaling, n_points, return_points=True)
    out = {"mauve": score, "mauve_n_clusters": k, "mauve_kmeans_iterations": run["n_iter"], "mauve_kmeans_inertia": run["inertia"]}
    if return_details:
        out.update({"mauve_points": points, "mauve_hist_candidate": hist[0].copy(), "mauve_hist_reference": hist[1].copy(),
                    "mauve_labels_candidate": lc, "mauve_labels_reference": lr})
    return out
