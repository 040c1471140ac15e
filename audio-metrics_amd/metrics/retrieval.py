"""Retrieval ranks of two PAIRED embedding sets: does a clip find ITS OWN prompt among all prompts, and at which rank?

R@1 / R@5 / R@10, median rank, MRR and mAP@10 - the numbers every text-to-audio and audio-captioning table (AudioCaps,
Clotho, the DCASE language-based retrieval task) reports next to the CLAP score.  A mean cosine of 0.31 says nothing
until one knows where the other 99 999 prompts score.

Definitions (csrc/retrieval.hip computes them without an N x M matrix).  Queries Q [N, D], gallery G [M, D], float32; the
positives P_i of query row i: gallery row i (paired sets), or the gallery rows with the query's label (five captions per
clip).  The score of a pair is u_ij = <q_i, g_j> * w_j with the dot product of the exact f32 tile engine and w_j = 1 / |g_j|
(cosine; correctly rounded) or 1 (dot); the query's own norm changes no order inside its row.  A pair whose u is NaN has no
score (a zero-norm gallery row under cosine, a row with a non-finite element): it is never a positive and never counted.

  t_i      = the best scored positive of row i; a row without one is UNRANKED and left out of every mean
  better_i = #{ negatives j : u_ij > t_i },  tied_i = #{ negatives j : u_ij == t_i }       exact float compares
  rank_i   = 1 + better_i           the optimistic convention, `(sims > diag).sum(1)` of the public retrieval code;
                                    ties="pessimistic" is rank + tied, ties="mean" rank + tied / 2

Windows of tracks.  With `groups` / `gallery_groups` (one integer label per row: the song) the columns of the row's own
song are no negatives: a window must not compete with the neighbouring windows of its own track, which share its prompt in
all but name.  A positive inside the row's own song is still the positive.  The standard errors then take the songs as
sampling units (the cluster-robust form of frechet_distance_with_error).

Everything after the sweep (retrieval_summary) is host arithmetic in numpy float64 and works on ranks from anywhere."""
import math
import warnings

import numpy as np
import torch

from .. import hip_ops as ops
from ._groups import _group_labels, joint_group_ids

SIMILARITIES = ("cosine", "dot")
TIE_RULES = ("optimistic", "pessimistic", "mean")
NAN = float("nan")


# ------------------------------------------------------------------------------------------------ host arithmetic
def _check_ks(ks):
    ks = tuple(int(k) for k in ks)
    if not ks or any(k < 1 for k in ks):
        raise ValueError(f"ks={ks!r} must name at least one cut-off, each >= 1")
    return ks


def _std_error(h, inverse, units):
    """Standard error of the mean of h: s / sqrt(n) over rows, or the cluster-robust form
    sqrt(G / (G - 1) * sum_g (sum_{i in g} (h_i - mean))^2) / n over labelled units; NaN below two rows / units."""
    n = len(h)
    if inverse is None:
        return float(math.sqrt(h.var(ddof=1) / n)) if n >= 2 else NAN
    if units < 2:
        return NAN
    per_unit = np.bincount(inverse, weights=h - h.mean(), minlength=units)
    return float(math.sqrt(units / (units - 1.0) * float(np.sum(per_unit * per_unit))) / n)


def retrieval_summary(ranks, tied=None, ks=(1, 5, 10), ties="optimistic", negatives=None, units=None):
    """The retrieval table from per-query ranks - host arithmetic, numpy float64, no GPU.  `ranks`: the optimistic rank of
    every query's best positive, 1 = retrieved first; a value < 1 (the -1 of retrieval_scores) marks an UNRANKED row, which
    is left out of every mean, with ONE RuntimeWarning naming their number.  `tied`: the negatives that score exactly as
    the positive (used by ties="pessimistic": rank + tied, and ties="mean": rank + tied / 2; optimistic ignores it).
    Returns plain floats:
      recall_at_{k}          the share of ranked rows with rank <= k, for every k of `ks`
      median_rank, mean_rank, mrr (the mean of 1 / rank)
      map_at_10              the mean of 1 / rank where rank <= 10, else 0.  It equals DCASE mAP@10 ONLY WITH ONE POSITIVE PER
                             QUERY: with several, average precision counts every positive, this the best one alone
      recall_at_{k}_std_error, mrr_std_error     over the ranked rows: s / sqrt(n), or with `units` (one integer label per
                             row: the song) the cluster-robust form with the units as sampling units
      chance_recall_at_{k}   with `negatives` (the number of negatives of every row): the mean of min(1, k / (negatives + 1)),
                             what a random order of the row's candidates gives
      retrieval_rows_ranked, retrieval_rows_unranked, retrieval_ties (the sum of `tied` over the ranked rows)"""
    if ties not in TIE_RULES:
        raise ValueError(f"ties={ties!r} is not one of {list(TIE_RULES)}")
    ks = _check_ks(ks)
    ranks = np.asarray(ranks)
    if ranks.ndim != 1:
        raise ValueError(f"ranks must be 1-D (one rank per query), got shape {ranks.shape}")
    n_all = ranks.shape[0]

    def per_row(v, name):
        if v is None:
            return None
        v = np.asarray(v)
        if v.shape != (n_all,):
            raise ValueError(f"{name} must hold one value per query ({n_all}), got shape {v.shape}")
        return v
    tied, negatives, units = per_row(tied, "tied"), per_row(negatives, "negatives"), per_row(units, "units")
    if ties != "optimistic" and tied is None:
        raise ValueError(f"ties={ties!r} needs the tied counts")
    keep = ranks >= 1
    n = int(keep.sum())
    if n < n_all:
        warnings.warn(f"retrieval_summary: {n_all - n} of {n_all} queries are unranked (no scored positive) and left out of "
                      "every mean", RuntimeWarning, stacklevel=2)
    out = {}
    r = ranks[keep].astype(np.float64)
    t = tied[keep].astype(np.float64) if tied is not None else np.zeros(n)
    if ties == "pessimistic":
        r = r + t
    elif ties == "mean":
        r = r + t / 2.0
    inverse, n_units = None, 0
    if units is not None and n:
        uniq, inverse = np.unique(units[keep], return_inverse=True)
        inverse, n_units = inverse.reshape(-1), len(uniq)
    for k in ks:
        hit = (r <= k).astype(np.float64)
        out[f"recall_at_{k}"] = float(hit.mean()) if n else NAN
        out[f"recall_at_{k}_std_error"] = _std_error(hit, inverse, n_units) if n else NAN
    rr = 1.0 / r
    out["median_rank"] = float(np.median(r)) if n else NAN
    out["mean_rank"] = float(r.mean()) if n else NAN
    out["mrr"] = float(rr.mean()) if n else NAN
    out["mrr_std_error"] = _std_error(rr, inverse, n_units) if n else NAN
    out["map_at_10"] = float(np.where(r <= 10, rr, 0.0).mean()) if n else NAN
    if negatives is not None:
        cand = negatives[keep].astype(np.float64) + 1.0
        for k in ks:
            out[f"chance_recall_at_{k}"] = float(np.minimum(1.0, k / cand).mean()) if n else NAN
    out["retrieval_rows_ranked"] = float(n)
    out["retrieval_rows_unranked"] = float(n_all - n)
    out["retrieval_ties"] = float(t.sum())
    return out


# ------------------------------------------------------------------------------------------------ front end
def _rows(data, name, what):
    rows = data if torch.is_tensor(data) else getattr(data, "embeddings", None)
    if rows is None or rows.dim() != 2 or rows.shape[0] == 0:
        if rows is not None and rows.dim() != 2:
            raise ValueError(f"{name} must hold 2-D rows, got shape {tuple(rows.shape)}")
        raise ValueError(f"{what} needs the stored rows of {name}, which keeps none "
                         f"(store_embeddings={getattr(data, 'store_embeddings', None)})")
    if rows.dtype == torch.float64:
        raise NotImplementedError(f"{what} takes float32 rows ({name} holds float64 rows; the float64 matrix-core form is not "
                                  "implemented)")
    return rows


def _row_labels(values, name, n):
    try:
        labels = _group_labels(values)
    except ValueError as e:
        raise ValueError(str(e).replace("groups", name, 1)) from None
    if labels.numel() != n:
        raise ValueError(f"{name} holds {labels.numel()} labels for {n} rows (one label per row)")
    return labels


def _both_or_neither(a, b, name_a, name_b, what):
    if (a is None) != (b is None):
        given, missing = (name_a, name_b) if b is None else (name_b, name_a)
        raise ValueError(f"{what}: {given} without {missing}: both sides need them, or neither")


def retrieval_scores(queries, gallery, query_labels=None, gallery_labels=None, groups=None, gallery_groups=None,
                     similarity="cosine", ks=(1, 5, 10), ties="optimistic", return_rows=False):
    """Retrieval of `gallery` rows by `queries` rows (AudioMetricsData with stored rows, or 2-D float32 device tensors, of
    one width).  Without labels the sets are paired row by row (equal length; the positive of row i is row i).  With
    query_labels / gallery_labels (one integer label per row, any integer dtype, host or device, compared by value across
    the two sets) the positives of a query are the gallery rows with an equal label - five captions per clip; the best of
    them ranks the query, a query whose label no gallery row carries is unranked.  groups / gallery_groups (the song of
    every row, as the labels of nearest_neighbors): the columns of the row's own song are no negatives - PASS THEM WHENEVER
    THE ROWS ARE WINDOWS OF TRACKS; both or neither.  similarity: "cosine" or "dot".

    Returns the floats of retrieval_summary - recall_at_{k}, median_rank, mean_rank, mrr, map_at_10 (the mean of 1 / rank
    where rank <= 10, else 0: DCASE mAP@10 only with ONE positive per query), recall_at_{k}_std_error and mrr_std_error
    (cluster-robust over the songs with `groups`), chance_recall_at_{k} (negatives_i = M - positives - the gallery rows of
    the row's own song that are no positives), retrieval_rows_ranked / _unranked, retrieval_ties - and
    "retrieval_similarity".  ties: "optimistic" (rank = 1 + better, the `(sims > diag).sum(1)` of the public code),
    "pessimistic" (rank + tied) or "mean" (rank + tied / 2); retrieval_ties says how much the choice can matter.  Unranked
    rows (no scored positive: a zero-norm or non-finite row) are left out of every mean with one RuntimeWarning.
    return_rows adds, in stored row order of the queries: "ranks" (int64, -1 unranked), "tied", "positive_score" (the
    cosine, or the dot product), "positive_index" (the gallery row that ranked the query; the smallest among equals) and
    "negatives".  Text -> audio and audio -> text are two calls with the arguments exchanged.  One sweep over N x M pairs
    on the exact f32 tile engine, the segments built on the device, one read-back."""
    what = "retrieval_scores"
    if similarity not in SIMILARITIES:
        raise ValueError(f"similarity={similarity!r} is not one of {list(SIMILARITIES)}")
    if ties not in TIE_RULES:
        raise ValueError(f"ties={ties!r} is not one of {list(TIE_RULES)}")
    ks = _check_ks(ks)
    _both_or_neither(query_labels, gallery_labels, "query_labels", "gallery_labels", what)
    _both_or_neither(groups, gallery_groups, "groups", "gallery_groups", what)
    eq, eg = _rows(queries, "queries", what), _rows(gallery, "gallery", what)
    n, m = int(eq.shape[0]), int(eg.shape[0])
    if eq.shape[1] != eg.shape[1]:
        raise ValueError(f"{what}: feature widths differ: {eq.shape[1]} and {eg.shape[1]}")
    if query_labels is None:
        if n != m:
            raise ValueError(f"{what}: without labels the sets are paired row by row, but queries holds {n} rows and gallery {m}")
    else:
        query_labels = _row_labels(query_labels, "query_labels", n)
        gallery_labels = _row_labels(gallery_labels, "gallery_labels", m)
    if groups is not None:
        groups = _row_labels(groups, "groups", n)
        gallery_groups = _row_labels(gallery_groups, "gallery_groups", m)
    if eq.device != eg.device:
        raise ValueError(f"{what}: queries and gallery are on different devices ({eq.device} and {eg.device})")
    dev = eq.device

    # the segments, on the device, nothing read back: paired - row i names column i; labelled - the gallery sorted by
    # label once, a query's segment is the run of its label
    if query_labels is None:
        pos_start = torch.arange(n, dtype=torch.int64, device=dev)
        pos_count = torch.ones(n, dtype=torch.int64, device=dev)
        pos_columns = pos_start
    else:
        lq, lg = joint_group_ids(query_labels, gallery_labels, dev)
        sorted_lg, pos_columns = torch.sort(lg.to(torch.int64), stable=True)
        lq = lq.to(torch.int64)
        pos_start = torch.searchsorted(sorted_lg, lq, right=False)
        pos_count = torch.searchsorted(sorted_lg, lq, right=True) - pos_start
    ids = None
    if groups is not None:
        ids = joint_group_ids(groups, gallery_groups, dev)
    better, tied, score, positive, n_pos, n_own = ops.retrieval_ranks(eq, eg, pos_start, pos_count, pos_columns,
                                                                      cosine=similarity == "cosine", groups=ids)
    # negatives_i = M - positives - (gallery rows of the row's own song) + (positives of the row's own song)
    negatives = m - n_pos.to(torch.int64)
    if ids is not None:
        song_rows = torch.zeros(n + m, dtype=torch.int64, device=dev)                   # (joint ids are dense: < n + m)
        song_rows.scatter_add_(0, ids[1].to(torch.int64), torch.ones(m, dtype=torch.int64, device=dev))
        negatives = negatives - song_rows[ids[0].to(torch.int64)] + n_own.to(torch.int64)
    # the one read-back: the float32 bit patterns of the scores travel beside the integers
    host = torch.stack([better.to(torch.int64), tied.to(torch.int64), positive, negatives,
                        score.view(torch.int32).to(torch.int64)]).cpu().numpy()
    better_h, tied_h, positive_h, negatives_h = host[0], host[1], host[2], host[3]
    ranks = np.where(better_h >= 0, better_h + 1, -1).astype(np.int64)
    units = groups.cpu().numpy() if groups is not None else None
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = retrieval_summary(ranks, tied_h, ks=ks, ties=ties, negatives=negatives_h, units=units)
    for w in caught:                                        # the summary's one warning, in this function's name
        warnings.warn(str(w.message).replace("retrieval_summary", what, 1), w.category, stacklevel=2)
    out["retrieval_similarity"] = similarity
    if return_rows:
        out["ranks"] = ranks
        out["tied"] = tied_h.copy()
        out["positive_score"] = host[4].astype(np.int32).view(np.float32)
        out["positive_index"] = positive_h.copy()
        out["negatives"] = negatives_h.copy()
    return out
