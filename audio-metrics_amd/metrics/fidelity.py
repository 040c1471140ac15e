"""Per-sample fidelity on the k-NN manifold that PRDC builds: which stored rows of `samples` are realistic, which are
off the manifold and which are rare - the per-clip question behind the four scalars of prdc().  The reference has no
such function; its PRDC keeps only counts (prdc.py:34-48).

  realism(x) = max_j r_j / |x - y_j|               Kynkaanniemi et al., NeurIPS 2019 (the paper precision and recall come
                                                   from): >= 1 is roughly "inside some ball", the value ranks the samples
  rarity(x)  = min { r_j : |x - y_j| < r_j }       Han et al., ICLR 2023: the radius of the smallest ball that holds x;
                                                   large = a sparsely populated region of the manifold set

over the stored rows y_j of `manifold` and their k-NN radii r_j = manifold.get_radii(nearest_k), the cached radii prdc()
uses.  One Gram pass on the exact f32 tile engine (ops.sample_scores), no N x M matrix; the distances and the strict
membership test are those of the exact PRDC kernel bit for bit, so ball_count is prdc()'s per-candidate count and the
precision and density computed from it here EQUAL prdc(manifold, samples, nearest_k)'s."""
import numpy as np
import torch

from .. import hip_ops as ops
from ._groups import labelled_rows
from .prdc_groups import grouped_scores


def _check_sets(function_name, samples, manifold, nearest_k, sample_rows=None):
    """The stored float32 rows of both sets after the argument checks; no device call."""
    k = int(nearest_k)
    if k < 1:
        raise ValueError(f"nearest_k={k} must be at least 1")
    rows = []
    for data, name in ((samples, "sample"), (manifold, "manifold")):
        e = sample_rows if (name == "sample" and sample_rows is not None) else getattr(data, "embeddings", None)
        if e is None or e.shape[0] == 0:
            raise ValueError(f"{function_name} needs the stored rows of its {name} set, which keeps none "
                             f"(store_embeddings={getattr(data, 'store_embeddings', None)})")
        rows.append(e)
    for e, name in zip(rows, ("sample", "manifold")):
        if e.dtype == torch.float64:
            raise NotImplementedError(f"{function_name}: the {name} set holds float64 rows; sample_scores takes float32 rows "
                                      "(the float64 matrix-core form is not implemented)")
    if rows[0].shape[1] != rows[1].shape[1]:
        raise ValueError(f"feature widths differ: {rows[0].shape[1]} and {rows[1].shape[1]}")
    return rows[0], rows[1], k


def _scores_on_host(ex, manifold, ey, k, device_labels=None, scores=None):
    """The five per-row vectors as numpy, from ONE read-back: the float32 bit patterns and the int32 counts travel beside
    the indices as int64 [n, 5] (labels that live on the device ride along as a sixth column, "labels").  `scores`: the
    five device tensors where the caller has run the pass already (the leave-group-out forms)."""
    if scores is None:
        scores = ops.sample_scores(ex, ey, manifold.get_radii(k))
    realism, realism_idx, count, rarity, rarity_idx = scores
    columns = [realism.view(torch.int32).to(torch.int64), realism_idx, count.to(torch.int64),
               rarity.view(torch.int32).to(torch.int64), rarity_idx]
    if device_labels is not None:
        columns.append(device_labels.to(device=realism.device, dtype=torch.int64))
    both = torch.stack(columns, dim=1).cpu().numpy()
    extra = {} if device_labels is None else {"labels": both[:, 5].copy()}
    return {**extra,
            "realism": both[:, 0].astype(np.int32).view(np.float32),
            "realism_index": both[:, 1].copy(),
            "ball_count": both[:, 2].astype(np.int32),
            "rarity": both[:, 3].astype(np.int32).view(np.float32),
            "rarity_index": both[:, 4].copy()}


def sample_fidelity(samples, manifold, nearest_k=5, groups=None, manifold_groups=None, match_across_sets=True):
    """Realism, ball count and rarity of every stored row of `samples` on the k-NN manifold of `manifold`.  Returns numpy
    arrays in stored row order of samples, from one read-back:
      realism float32 [n], realism_index int64 [n] (the manifold row that attains it; ties to the smallest index; -1 where
      the realism is 0: a non-finite sample row, or no manifold row with a positive radius),
      ball_count int32 [n] (the balls the row lies in), in_manifold bool [n] (ball_count > 0),
      rarity float32 [n] and rarity_index int64 [n] (0.0 and -1 for a row outside every ball), nearest_k,
      precision = (#in_manifold) / n and density = (1 / k) * (sum(ball_count) / n), equal to prdc(manifold, samples, k)'s.
    float32 rows.  `samples` may be `manifold`: nothing is skipped, so every row then has realism +inf.

    groups / manifold_groups: one integer label per stored row of samples / of manifold (the song a window was cut from; any
    integer dtype, host or device, any order; compared by VALUE across the two sets).  With manifold_groups the radii are
    the leave-group-out radii of the manifold (metrics/prdc_groups.py: leave_group_out_radii; 1 <= nearest_k <= 32); with
    groups as well and match_across_sets=True a manifold row of the sample's own label is no reference row of it
    (ops.sample_scores_groups), and precision and density EQUAL prdc_leave_group_out's.  With `samples is manifold`
    manifold_groups defaults to groups: every row is scored against the OTHER songs, the leave-one-out form.  Without the
    two keywords this is the path above, unchanged."""
    ex, ey, k = _check_sets("sample_fidelity", samples, manifold, nearest_k)
    scores = None
    if groups is not None or manifold_groups is not None:
        scores = grouped_scores("sample_fidelity", samples, ex, manifold, ex if samples is manifold else ey, k, groups,
                                manifold_groups, match_across_sets)
    out = _scores_on_host(ex, manifold, ex if samples is manifold else ey, k, scores=scores)
    n = out["ball_count"].shape[0]
    out["in_manifold"] = out["ball_count"] > 0
    out["nearest_k"] = k
    # the expressions of metrics/prdc.py on the same integers
    out["precision"] = int(out["in_manifold"].sum()) / n
    out["density"] = (1.0 / float(k)) * (int(out["ball_count"].astype(np.int64).sum()) / n)
    return out


def fidelity_by_group(labels, realism, ball_count, rarity, nearest_k):
    """The host aggregation of per-row fidelity into per-group ("per-song") results: numpy float64, no GPU, no torch.
    Returns group_labels (ascending), group_sizes, precision_per_group (rows with ball_count > 0 over the group's rows),
    density_per_group ((1 / k) * mean ball_count), realism_median_per_group and rarity_median_per_group (over the group's
    in-manifold rows; NaN for a group that has none).  Deterministic: a stable sort by label, np.add.reduceat per segment."""
    labels = np.asarray(labels)
    if labels.ndim != 1 or labels.size == 0:
        raise ValueError(f"labels must be 1-D and not empty, got shape {labels.shape}")
    if labels.dtype.kind not in "iu":
        raise ValueError(f"labels must hold integers, got dtype {labels.dtype}")
    k = int(nearest_k)
    if k < 1:
        raise ValueError(f"nearest_k={k} must be at least 1")
    n = labels.shape[0]
    realism = np.asarray(realism, dtype=np.float64)
    rarity = np.asarray(rarity, dtype=np.float64)
    ball_count = np.asarray(ball_count).astype(np.int64)
    for name, v in (("realism", realism), ("ball_count", ball_count), ("rarity", rarity)):
        if v.shape != (n,):
            raise ValueError(f"{name} has shape {v.shape} for {n} labels (one value per row)")
    order = np.argsort(labels, kind="stable")
    sorted_labels = labels[order]
    starts = np.flatnonzero(np.concatenate(([True], sorted_labels[1:] != sorted_labels[:-1])))
    sizes = np.diff(np.concatenate((starts, [n]))).astype(np.int64)
    cnt = ball_count[order]
    inside = cnt > 0
    n_inside = np.add.reduceat(inside.astype(np.int64), starts)
    sum_cnt = np.add.reduceat(cnt, starts)
    real_sorted, rare_sorted = realism[order], rarity[order]
    realism_median = np.empty(len(starts), dtype=np.float64)
    rarity_median = np.full(len(starts), np.nan, dtype=np.float64)
    with np.errstate(invalid="ignore"):                      # the median of two +inf realism values is +inf, not a warning
        for g, (lo, size) in enumerate(zip(starts, sizes)):
            realism_median[g] = np.median(real_sorted[lo:lo + size])
            members = rare_sorted[lo:lo + size][inside[lo:lo + size]]
            if members.size:
                rarity_median[g] = np.median(members)
    return {"group_labels": sorted_labels[starts].astype(np.int64),
            "group_sizes": sizes,
            "precision_per_group": n_inside / sizes,
            "density_per_group": (1.0 / float(k)) * (sum_cnt / sizes),
            "realism_median_per_group": realism_median,
            "rarity_median_per_group": rarity_median}


def sample_fidelity_per_group(samples, manifold, groups, nearest_k=5, return_rows=False, manifold_groups=None,
                              match_across_sets=True):
    """sample_fidelity aggregated over row groups of `samples` (`groups`: one integer label per stored row, e.g. the song a
    clip was cut from): group_labels (ascending), group_sizes, precision_per_group, density_per_group,
    realism_median_per_group, rarity_median_per_group (over the group's in-manifold rows; NaN when it has none) and
    nearest_k; return_rows=True adds the per-row arrays of sample_fidelity.  One read-back; the aggregation runs on the host
    over the vectors already read back (fidelity_by_group).  manifold_groups (one label per stored row of manifold): the
    leave-group-out form of sample_fidelity, with `groups` doubling as the labels of the samples; without it this is the
    plain path, unchanged."""
    rows, n, labels = labelled_rows(samples, groups, "sample_fidelity_per_group", "its sample set")
    ex, ey, k = _check_sets("sample_fidelity_per_group", samples, manifold, nearest_k, sample_rows=rows)
    scores = None
    if manifold_groups is not None:
        scores = grouped_scores("sample_fidelity_per_group", samples, ex, manifold, ex if samples is manifold else ey, k, groups,
                                manifold_groups, match_across_sets)
    on_device = labels.device.type != "cpu"
    per_row = _scores_on_host(ex, manifold, ex if samples is manifold else ey, k, device_labels=labels if on_device else None,
                              scores=scores)
    host_labels = per_row.pop("labels") if on_device else labels.numpy()
    out = fidelity_by_group(host_labels, per_row["realism"], per_row["ball_count"], per_row["rarity"], k)
    out["nearest_k"] = k
    if return_rows:
        per_row["in_manifold"] = per_row["ball_count"] > 0
        out.update(per_row)
    return out
