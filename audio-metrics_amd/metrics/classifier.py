"""Classifier-output metrics: the columns of text-to-audio results tables that are row-wise on a matrix of logits, or on
two matrices paired row by row, rather than distances between two unordered clouds.

  inception_score        IS = exp(H(mean_i p_i) - mean_i H(p_i)), p_i = softmax of row i (Salimans et al. 2016), per split
  kl_divergence_paired   the mean over i of KL(p^ref_i || p^cand_i), the "KL" column (softmax, or one of two sigmoid forms)
  paired_cosine_score    the mean over i of cos(a_i, b_i); with audio and text embeddings of one model this is the mean that
                         papers call "CLAP score" (some report it times 100 or clipped at 0; here it is the mean as it is)

Row quantities of a row l: M = max l_c, e_c = exp(l_c - M), S = sum e_c, U = sum e_c (l_c - M), p_c = e_c / S and
h = sum p_c log p_c = U / S - log S, the negative entropy of the row's posterior.  A logit of -inf is a masked class; a row
with a NaN, a +inf or nothing but -inf is non-finite.  All device arithmetic is f64 in a fixed order (csrc/class_scores.hip):
float32 logits and their float64 copies give the same bits, and so do two calls.  These are restatements of the published
definitions; no evaluation toolkit's numbers are claimed.  The functions are calls, not metric names of AudioMetrics."""
import math
import types
import warnings

import numpy as np
import torch

from .. import hip_ops as ops
from ._groups import _group_labels, labelled_rows, sort_into_groups
from .vendi import _stored_rows

KL_MODES = ("softmax", "sigmoid", "bernoulli")


# ------------------------------------------------------------------ host helpers (numpy, no GPU)
def split_offsets(n, splits):
    """The offsets [k n // splits, k = 0 .. splits] of the list positions of the splits: split k is [offsets[k],
    offsets[k + 1]).  1 <= splits <= n, so no split is empty."""
    n, splits = int(n), int(splits)
    if not 1 <= splits <= n:
        raise ValueError(f"splits={splits} must be >= 1 and <= the number of rows ({n})")
    return [k * n // splits for k in range(splits + 1)]


def inception_summary(log_is, sizes, mean_h, marginal):
    """The result of inception_score from the per-split device records: log_is [B] = log IS_b, sizes [B] the rows per
    split, mean_h [B] = (1 / n_b) sum h, marginal [B] = m_b.  The score is the mean of the per-split IS with its population
    standard deviation (ddof = 0, what the toolkits print); the two entropies are row-weighted over the splits.  A NaN
    split makes every summary NaN."""
    log_is = np.asarray(log_is, dtype=np.float64).ravel()
    sizes = np.asarray(sizes, dtype=np.float64).ravel()
    mean_h = np.asarray(mean_h, dtype=np.float64).ravel()
    marginal = np.asarray(marginal, dtype=np.float64).ravel()
    if not (log_is.size >= 1 and log_is.size == sizes.size == mean_h.size == marginal.size):
        raise ValueError("one log IS, size, mean h and marginal per split, and at least one split")
    per_split = np.exp(log_is)
    n = math.fsum(sizes)
    mean = math.fsum(per_split) / per_split.size
    var = math.fsum((v - mean) ** 2 for v in per_split) / per_split.size
    return {"inception_score": float(mean), "inception_score_std": float(math.sqrt(var)) if var == var else float("nan"),
            "inception_score_per_split": per_split,
            "inception_conditional_entropy": float(-math.fsum(sizes * mean_h) / n),
            "inception_marginal_entropy": float(-math.fsum(sizes * marginal) / n),
            "inception_n_splits": int(per_split.size)}


def paired_summary(sums):
    """(mean, standard error, rows used, rows left out) from the device's { sum v, sum v^2, finite rows, non-finite rows }:
    the mean over the finite rows and s(v) / sqrt(n) with the sample standard deviation (ddof = 1); the standard error is
    NaN for fewer than 2 rows, the mean for none."""
    s1, s2, nf, nn = (float(v) for v in np.asarray(sums, dtype=np.float64).ravel())
    used, left = int(nf), int(nn)
    if used < 1:
        return float("nan"), float("nan"), used, left
    mean = s1 / used
    if used < 2:
        return mean, float("nan"), used, left
    var = max((s2 - s1 * s1 / used) / (used - 1), 0.0)
    return mean, math.sqrt(var / used), used, left


def rows_by_group(labels, values):
    """Host aggregation of per-row values into per-group means: numpy float64, no GPU.  Returns (group_labels ascending,
    group_sizes, mean of the finite values of each group - NaN for a group without one).  A stable sort by label and
    np.add.reduceat per segment, as psr_by_group does."""
    labels = np.asarray(labels)
    if labels.ndim != 1 or labels.size == 0:
        raise ValueError(f"labels must be 1-D and not empty, got shape {labels.shape}")
    if labels.dtype.kind not in "iu":
        raise ValueError(f"labels must hold integers, got dtype {labels.dtype}")
    n = labels.shape[0]
    values = np.asarray(values, dtype=np.float64)
    if values.shape != (n,):
        raise ValueError(f"values has shape {values.shape} for {n} labels (one value per row)")
    order = np.argsort(labels, kind="stable")
    sorted_labels = labels[order]
    starts = np.flatnonzero(np.concatenate(([True], sorted_labels[1:] != sorted_labels[:-1])))
    sizes = np.diff(np.concatenate((starts, [n]))).astype(np.int64)
    v = values[order]
    fin = np.isfinite(v)
    total = np.add.reduceat(np.where(fin, v, 0.0), starts)
    count = np.add.reduceat(fin.astype(np.float64), starts)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(count > 0, total / count, np.nan)
    return sorted_labels[starts].astype(np.int64), sizes, mean


# ------------------------------------------------------------------ Inception Score
def _holder(x):
    """what labelled_rows takes: the set itself, or a stand-in around a 2-D tensor"""
    if torch.is_tensor(x):
        return types.SimpleNamespace(embeddings=x if x.dim() == 2 else None, store_embeddings=True)
    return x


def _warn_nonfinite(function_name, count, what):
    if count:
        warnings.warn(f"{function_name}: {count} {what}", RuntimeWarning, stacklevel=3)


def inception_score(logits, splits=10, seed=None, return_rows=False):
    """The Inception Score of the rows of `logits` (an AudioMetricsData whose stored rows are the classifier's logits, or a
    2-D float32 / float64 device tensor [n, C], C <= 2048).  The rows are cut into `splits` splits: split k is the list
    positions [k n // splits, (k + 1) n // splits) of the stored row order (seed=None) or of
    numpy.random.default_rng(seed).permutation(n).  One library call scores all splits.  Returns {"inception_score": the
    mean of the per-split IS, "inception_score_std": their population standard deviation (ddof = 0),
    "inception_score_per_split": f64 [splits], "inception_conditional_entropy", "inception_marginal_entropy": row-weighted
    over the splits (log IS = marginal - conditional per split), "inception_n_splits"}, plus "row_entropy" (f64 [n], stored
    row order, the entropy of each row's posterior) with return_rows.  A split with a non-finite row (a NaN, a +inf, or
    nothing but -inf) is NaN, and the call issues one RuntimeWarning naming the number of such rows."""
    rows, _ = _stored_rows(logits, "inception_score")
    n = int(rows.shape[0])
    ops.check_score_rows(rows, "logits", ops.CLASS_GROUPS_MAX_COLUMNS)
    offs = split_offsets(n, splits)
    perm = None if seed is None else np.random.default_rng(seed).permutation(n).astype(np.int64)
    rows = ops.as_rows(rows, "logits")
    order = None if perm is None else ops.upload_host_array(perm, rows.device)
    rec, h, check = ops.class_group_scores(rows, order, offs, return_rows=return_rows)
    flat = (torch.cat([rec.reshape(-1), h]) if return_rows else rec.reshape(-1)).cpu().numpy()         # the one read-back
    check()
    nb = len(offs) - 1
    rec_h = flat[:4 * nb].reshape(nb, 4)
    out = inception_summary(rec_h[:, 2], np.diff(offs), rec_h[:, 0], rec_h[:, 1])
    if return_rows:
        ent = np.empty(n)
        ent[perm if perm is not None else np.arange(n)] = -flat[4 * nb:]
        out["row_entropy"] = ent
    _warn_nonfinite("inception_score", int(rec_h[:, 3].sum()),
                    "rows hold a NaN, a +inf or nothing but -inf; the splits that hold them are NaN")
    return out


def inception_score_per_group(logits, groups):
    """The Inception Score of every group of rows on its own ("are the 50 generations of this prompt all one class?").
    `groups`: one integer label per row (numpy or torch, any order, any values, groups of any size); logits as
    inception_score takes them.  One library call for all groups, no gathered copy; a group's bits depend on its rows and
    their order alone, not on where the rows lie.  Returns {"inception_score_per_group": f64 [B], "inception_log_per_group":
    f64 [B], "group_labels": [B] ascending, "group_sizes": int64 [B]}.  A group with a non-finite row gets NaN and the call
    one RuntimeWarning; no other group is affected."""
    rows, n, labels = labelled_rows(_holder(logits), groups, "inception_score_per_group", "its first argument")
    ops.check_score_rows(rows, "logits", ops.CLASS_GROUPS_MAX_COLUMNS)
    rows = ops.as_rows(rows, "logits")
    order, _, group_labels, sizes = sort_into_groups(labels.to(rows.device, torch.int64))
    offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    rec, _, check = ops.class_group_scores(rows, order, offs, return_rows=False)
    rec_h = rec.cpu().numpy()                                                                           # the one read-back
    check()
    bad = rec_h[:, 3] != 0
    if bad.any():
        warnings.warn(f"inception_score_per_group: {int(bad.sum())} of {len(sizes)} groups hold a row with a NaN, a +inf or "
                      "nothing but -inf; their score is NaN", RuntimeWarning, stacklevel=2)
    return {"inception_score_per_group": np.exp(rec_h[:, 2]), "inception_log_per_group": rec_h[:, 2].copy(),
            "group_labels": group_labels, "group_sizes": sizes}


# ------------------------------------------------------------------ paired scores
def _paired(function_name, key, a, b, mode, eps, groups, return_rows):
    rows_a, _ = _stored_rows(a, function_name)
    rows_b, _ = _stored_rows(b, function_name)
    if rows_a.shape[0] != rows_b.shape[0]:
        raise ValueError(f"{function_name}: the sets are paired row by row, but hold {rows_a.shape[0]} and {rows_b.shape[0]} rows")
    eps = ops.check_row_pair(rows_a, rows_b, mode, eps)
    labels = None
    if groups is not None:
        labels = _group_labels(groups)
        if labels.numel() != rows_a.shape[0]:
            raise ValueError(f"groups holds {labels.numel()} labels for {rows_a.shape[0]} row pairs (one label per row)")
        labels = labels.cpu().numpy()
    want_rows = bool(return_rows) or labels is not None
    sums, rows = ops.row_pair_scores(rows_a, rows_b, mode, eps, return_rows=want_rows)
    flat = (torch.cat([sums, rows]) if want_rows else sums).cpu().numpy()                               # the one read-back
    mean, se, used, left = paired_summary(flat[:4])
    out = {key: mean, key + "_std_error": se}
    tail = {"rows_used": used, "rows_nonfinite": left}
    if labels is not None:
        group_labels, sizes, per_group = rows_by_group(labels, flat[4:])
        tail.update(per_group=per_group)
        out.update(group_labels=group_labels, group_sizes=sizes)
    if return_rows:
        tail.update(rows=flat[4:].copy())
    if left:
        warnings.warn(f"{function_name}: {left} of {used + left} row pairs have no finite value and are left out of the mean",
                      RuntimeWarning, stacklevel=3)
    return out, tail


def kl_divergence_paired(cand, ref, mode="softmax", eps=0.0, groups=None, return_rows=False):
    """The "KL" column: the mean over the rows i of the divergence of the candidate clip's class posterior from its paired
    reference clip's, both sets' stored rows being the classifier's logits (AudioMetricsData, or 2-D float32 / float64
    device tensors of one shape and dtype, C <= 8192).  With r the reference row and c the candidate row:
      "softmax"    sum_c p^r_c (log p^r_c - log(p^c_c + eps)), p = softmax; at eps = 0 through the log-sum-exps, finite for
                   finite logits however far they underflow
      "sigmoid"    sum_c s(r_c) (log s(r_c) - log(s(c_c) + eps)), s the logistic function: the one-term form used for
                   multi-label taggers.  It is NOT a divergence between Bernoulli laws and can be negative
      "bernoulli"  sum_c [ s log(s / (t + eps)) + (1 - s) log((1 - s) / (1 - t + eps)) ], s = s(r_c), t = s(c_c): the true
                   per-class divergence, >= 0 at eps = 0
    Returns {"kl": the mean over the rows with a finite value, "kl_std_error": s / sqrt(n) with the sample standard
    deviation (NaN for fewer than 2 rows), "kl_mode", "kl_eps", "kl_rows_used", "kl_rows_nonfinite"}; with groups (one
    integer label per row pair) "kl_per_group", "group_labels", "group_sizes" (host aggregation of the rows read back); with
    return_rows "kl_rows" (f64 [n]).  Without either the only read-back is four sums.  Rows without a finite value are
    counted, left out, and reported by one RuntimeWarning."""
    if mode not in KL_MODES:
        raise ValueError(f"mode={mode!r} must be one of {KL_MODES}")
    out, tail = _paired("kl_divergence_paired", "kl", cand, ref, "kl_" + mode, eps, groups, return_rows)
    out.update(kl_mode=mode, kl_eps=float(eps), kl_rows_used=tail["rows_used"], kl_rows_nonfinite=tail["rows_nonfinite"])
    if "per_group" in tail:
        out["kl_per_group"] = tail["per_group"]
    if "rows" in tail:
        out["kl_rows"] = tail["rows"]
    return out


def paired_cosine_score(a, b, groups=None, return_rows=False):
    """The mean over the rows i of cos(a_i, b_i) = <a_i, b_i> / (|a_i| |b_i|), the two sets' stored rows being paired
    embeddings (AudioMetricsData, or 2-D float32 / float64 device tensors of one shape and dtype, at most 8192 columns).
    With each clip's audio embedding and its prompt's text embedding this mean is what papers call "CLAP score"; some report
    it times 100 or clipped at 0, this is the mean as it is.  Returns {"cosine_score", "cosine_score_std_error",
    "cosine_rows_used", "cosine_rows_nonfinite"}, with groups "cosine_score_per_group", "group_labels", "group_sizes", with
    return_rows "cosine_rows".  A pair with a zero norm or a non-finite element has no value: counted, left out, one
    RuntimeWarning."""
    out, tail = _paired("paired_cosine_score", "cosine_score", a, b, "cosine", 0.0, groups, return_rows)
    out.update(cosine_rows_used=tail["rows_used"], cosine_rows_nonfinite=tail["rows_nonfinite"])
    if "per_group" in tail:
        out["cosine_score_per_group"] = tail["per_group"]
    if "rows" in tail:
        out["cosine_rows"] = tail["rows"]
    return out
