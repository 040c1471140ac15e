"""Probabilistic precision and recall (P-precision / P-recall; Park & Kim, "Probabilistic Precision and Recall Towards
Reliable Evaluation of Generative Models", ICCV 2023) between the stored rows of two sets.  The reference has no such
function; this is the restatement below, NOT compared with the authors' package.

PRDC's precision and recall count a sample as "in the manifold" as soon as it falls into any one k-NN ball, so one outlying
row with a huge k-NN radius swallows a region of embedding space.  The probabilistic form changes three things: every set
has ONE radius, a pair contributes a probability that falls linearly with distance, and the probabilities of a row's pairs
are combined as 1 - prod(1 - p):

  R_S        = a * mean_i NND_k(s_i)                        NND_k: distance to the k-th nearest other row = get_radii(k)
  PSR_S(z)   = 1 - prod_{i : |z - s_i| < R_S} |z - s_i| / R_S       0: no row of S within R_S;  1: z sits on a row of S
  p_precision = mean_j PSR_ref(y_j)  over the candidate rows,   p_recall = mean_i PSR_cand(x_i)  over the reference rows

with the paper's defaults k = 4, a = 1.2.  Two Gram passes on the exact f32 tile engine (ops.psr_scores), no N x M matrix;
p_precision(cand, ref) and p_recall(ref, cand) are the same pass and agree bit for bit.

Conventions of this build: non-finite k-NN radii (rows with NaN / inf elements) are left out of the mean with one
RuntimeWarning; an in-range fraction above SATURATION_FRACTION on either side gives one RuntimeWarning - the radius covers
most of the other set, the distances have concentrated (isotropic high-dimensional rows) and the values saturate at 1."""
import math
import warnings

import numpy as np
import torch

from .. import hip_ops as ops
from ._groups import labelled_rows

# in-range fraction (mean count / rows of the other set) above which the result is flagged as saturated: a convention of
# this build, not the paper's
SATURATION_FRACTION = 0.5
_F32_MAX = 3.4028234663852886e+38


def psr_radius(radii, a):
    """The set radius from per-row k-NN radii, on the host in numpy float64: (a * mean of the finite radii, number of
    radii left out).  ValueError when no radius is finite."""
    r = np.asarray(radii, dtype=np.float64).reshape(-1)
    a = float(a)
    if not (math.isfinite(a) and a > 0.0):
        raise ValueError(f"a={a} must be finite and > 0")
    finite = np.isfinite(r)
    left_out = int(r.size - int(finite.sum()))
    if left_out == r.size:
        raise ValueError("no finite k-NN radius: the set radius is undefined")
    return a * float(np.mean(r[finite])), left_out


def psr_by_group(labels, psr):
    """The host aggregation of per-row PSR into per-group ("per-song") results: numpy float64, no GPU, no torch.  Returns
    group_labels (ascending), group_sizes and p_precision_per_group (mean PSR of the group's rows).  Deterministic: a stable
    sort by label, np.add.reduceat per segment, as fidelity_by_group does."""
    labels = np.asarray(labels)
    if labels.ndim != 1 or labels.size == 0:
        raise ValueError(f"labels must be 1-D and not empty, got shape {labels.shape}")
    if labels.dtype.kind not in "iu":
        raise ValueError(f"labels must hold integers, got dtype {labels.dtype}")
    n = labels.shape[0]
    psr = np.asarray(psr, dtype=np.float64)
    if psr.shape != (n,):
        raise ValueError(f"psr has shape {psr.shape} for {n} labels (one value per row)")
    order = np.argsort(labels, kind="stable")
    sorted_labels = labels[order]
    starts = np.flatnonzero(np.concatenate(([True], sorted_labels[1:] != sorted_labels[:-1])))
    sizes = np.diff(np.concatenate((starts, [n]))).astype(np.int64)
    return {"group_labels": sorted_labels[starts].astype(np.int64),
            "group_sizes": sizes,
            "p_precision_per_group": np.add.reduceat(psr[order], starts) / sizes}


def _explicit_radius(value, name):
    if value is None:
        return None
    value = float(value)
    if not (math.isfinite(value) and value > 0.0 and value * value <= _F32_MAX):
        raise ValueError(f"{name}={value} must be finite and > 0, with its square a finite float32 number")
    return value


def _check_sets(function_name, cand, ref, nearest_k, a, need_radius, cand_rows=None):
    """The stored float32 rows of both sets, k and a after the argument checks; no device call.  need_radius: per set
    (candidate, reference), whether its radius comes from its k-NN radii (it then needs nearest_k + 1 rows)."""
    k = int(nearest_k)
    if k < 1:
        raise ValueError(f"nearest_k={k} must be at least 1")
    a = float(a)
    if not (math.isfinite(a) and a > 0.0):
        raise ValueError(f"a={a} must be finite and > 0")
    rows = []
    for data, name in ((cand, "candidate"), (ref, "reference")):
        e = cand_rows if (name == "candidate" and cand_rows is not None) else getattr(data, "embeddings", None)
        if e is None or e.shape[0] == 0:
            raise ValueError(f"{function_name} needs the stored rows of its {name} set, which keeps none "
                             f"(store_embeddings={getattr(data, 'store_embeddings', None)})")
        rows.append(e)
    for e, name in zip(rows, ("candidate", "reference")):
        if e.dtype == torch.float64:
            raise NotImplementedError(f"{function_name}: the {name} set holds float64 rows; psr_scores takes float32 rows "
                                      "(the float64 matrix-core form is not implemented)")
    if rows[0].shape[1] != rows[1].shape[1]:
        raise ValueError(f"feature widths differ: {rows[0].shape[1]} and {rows[1].shape[1]}")
    for e, name, need in zip(rows, ("candidate", "reference"), need_radius):
        if need and e.shape[0] < k + 1:
            raise ValueError(f"{function_name}: the {name} set holds {e.shape[0]} rows; the k-NN radius of nearest_k={k} "
                             f"needs at least {k + 1}")
    return rows[0], rows[1], k, a


def _set_radius(data, rows, k, a, name):
    """a * mean of the finite k-NN radii of the stored rows, reduced on the device in f64 and read back once; kept on the
    set under (k, a, stored rows)."""
    n = int(rows.shape[0])
    cache = data.__dict__.setdefault("_psr_radius", {})
    key = (k, a, n, getattr(data, "_content_version", None))
    if key in cache:
        return cache[key]
    radii = data.get_radii(k)
    if radii is None or radii.shape[0] != n:
        # get_radii keeps the reference's rule that an append does not invalidate it: fresh radii for this call, that
        # cache stays as it is
        radii = ops.knn_radii(rows, k)
    r64 = radii.to(torch.float64)
    finite = torch.isfinite(r64)
    both = torch.stack([torch.where(finite, r64, torch.zeros_like(r64)).sum(), finite.sum().to(torch.float64)]).cpu().numpy()
    kept = int(both[1])
    if kept == 0:
        raise ValueError(f"no finite k-NN radius in the {name} set: its radius is undefined")
    if kept != n:
        warnings.warn(f"{n - kept} of the {n} k-NN radii of the {name} set are not finite (rows with NaN / inf elements) "
                      "and are left out of the mean radius", RuntimeWarning, stacklevel=3)
    value = a * (float(both[0]) / kept)
    if not (math.isfinite(value) and value > 0.0 and value * value <= _F32_MAX):
        raise ValueError(f"the radius of the {name} set, {value}, is not a positive number with a finite float32 square")
    for stale in [other for other in cache if other[2:] != key[2:]]:       # radii of rows that are no longer the stored ones
        del cache[stale]
    cache[key] = value
    return value


def _warn_if_saturated(fractions, stacklevel):
    worst = max(fractions)
    if worst > SATURATION_FRACTION:
        warnings.warn(f"the radius covers {100.0 * worst:.0f} % of the other set on average (above "
                      f"{100.0 * SATURATION_FRACTION:.0f} %): the distances have concentrated and probabilistic precision / "
                      "recall saturate at 1", RuntimeWarning, stacklevel=stacklevel)


def probabilistic_precision_recall(cand, ref, nearest_k=4, a=1.2, radius_reference=None, radius_candidate=None,
                                   return_rows=False):
    """P-precision and P-recall of the stored rows of `cand` against those of `ref`.  Returns p_precision, p_recall,
    p_radius_reference, p_radius_candidate, p_in_range_reference (mean over the candidate rows of count / m),
    p_in_range_candidate (mean over the reference rows of count / n), nearest_k and a; return_rows=True adds, in stored row
    order, candidate_psr float64 [n], candidate_in_range int32 [n], reference_psr float64 [m], reference_in_range int32 [m].
    An explicit radius_* skips that side's k-NN radii; otherwise the radius is a * mean(get_radii(nearest_k)) over the
    finite radii.  Without return_rows the only read-back of the two passes is their two pairs of sums, in one transfer.
    float32 rows."""
    r_ref, r_cand = _explicit_radius(radius_reference, "radius_reference"), _explicit_radius(radius_candidate, "radius_candidate")
    ec, er, k, a = _check_sets("probabilistic_precision_recall", cand, ref, nearest_k, a, (r_cand is None, r_ref is None))
    if r_ref is None:
        r_ref = _set_radius(ref, er, k, a, "reference")
    if r_cand is None:
        r_cand = _set_radius(cand, ec, k, a, "candidate")
    n, m = int(ec.shape[0]), int(er.shape[0])
    psr_c, cnt_c, sums_c = ops.psr_scores(ec, er, r_ref)           # X = cand, Y = ref: p_precision
    psr_r, cnt_r, sums_r = ops.psr_scores(er, ec, r_cand)          # X = ref, Y = cand: p_recall
    sums = torch.stack([sums_c, sums_r]).cpu().numpy()
    out = {"p_precision": float(sums[0, 0]) / n,
           "p_recall": float(sums[1, 0]) / m,
           "p_radius_reference": r_ref,
           "p_radius_candidate": r_cand,
           "p_in_range_reference": float(sums[0, 1]) / n / m,
           "p_in_range_candidate": float(sums[1, 1]) / m / n,
           "nearest_k": k,
           "a": a}
    _warn_if_saturated((out["p_in_range_reference"], out["p_in_range_candidate"]), 3)
    if return_rows:
        out["candidate_psr"] = psr_c.cpu().numpy()
        out["candidate_in_range"] = cnt_c.cpu().numpy()
        out["reference_psr"] = psr_r.cpu().numpy()
        out["reference_in_range"] = cnt_r.cpu().numpy()
    return out


def probabilistic_precision_per_group(cand, ref, groups, nearest_k=4, a=1.2, radius_reference=None):
    """P-precision aggregated over row groups of `cand` (`groups`: one integer label per stored row, e.g. the song a clip
    was cut from): group_labels (ascending), group_sizes, p_precision_per_group (mean PSR of the group's rows),
    p_radius_reference, nearest_k and a.  One pass; the aggregation runs on the host over the vector read back
    (psr_by_group)."""
    rows, n, labels = labelled_rows(cand, groups, "probabilistic_precision_per_group", "its candidate set")
    r_ref = _explicit_radius(radius_reference, "radius_reference")
    ec, er, k, a = _check_sets("probabilistic_precision_per_group", cand, ref, nearest_k, a, (False, r_ref is None), cand_rows=rows)
    if r_ref is None:
        r_ref = _set_radius(ref, er, k, a, "reference")
    psr, _, _ = ops.psr_scores(ec, er, r_ref, sums=False)
    host_psr = psr.cpu().numpy()
    host_labels = labels.cpu().numpy()
    out = psr_by_group(host_labels, host_psr)
    out["p_radius_reference"] = r_ref
    out["nearest_k"] = k
    out["a"] = a
    return out
