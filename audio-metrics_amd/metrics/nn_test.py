"""The nearest-neighbour two-sample test (Schilling 1986; Henze 1988; as a sample-quality measure: the leave-one-out 1-NN
accuracy of Lopez-Paz & Oquab 2017 and Xu et al. 2018): pool the candidate and the reference rows, give every row its k
nearest pooled rows, and count how often a neighbour comes from the row's own set.  Two samples of one law mix - the share
is what the set sizes give, 1/2 after balancing - and two different laws keep to themselves.  No kernel, bandwidth, model
or optimiser is involved.  The definitions below are THIS BUILD'S (the reference has no such test).

Units and the pooled order.  Units are the labels of `groups` / `ref_groups` (the song a window comes from); without labels
every row of that side is its own unit.  Candidate units and reference units are distinct even where their integers
coincide.  Pooled row order: the candidate rows, then the reference rows (reference row j is pooled row n + j).

Graph.  Every pooled row gets its k nearest pooled rows THAT ARE NOT IN ITS OWN UNIT - windows of one track are
near-duplicates, and a graph that lets a window choose its siblings measures the windowing, not the model.  It comes
from four searches and no pooled copy of the rows: cand in cand and ref in ref leave the row's group out
(ops.knn_search_groups; without labels ops.knn_search with self_offset = 0), cand in ref and ref in cand are plain
searches.  A row's two lists of k are merged on the device by a stable sort on the squared distance, the candidate-side
list first: a tie goes to the smaller pooled index.  The graph depends on no set label.

Statistic.  With S_x the number of (row, neighbour) edges from a candidate-labelled row to a candidate-labelled row, E_x the
number of edges from candidate-labelled rows, S_y and E_y the same for the reference,
    nn_accuracy = 1/2 (S_x / E_x + S_y / E_y);   nn_accuracy_candidate and nn_accuracy_reference are the two terms.
A missing neighbour (index -1: fewer than k admissible rows) is not an edge.  A row with a NaN or inf element is in nothing.

Null.  The edges are aggregated to (unit a, unit b, count) triples - at most (n + m) k of them, never a dense U x U matrix,
because units may be single rows.  A relabelling calls the first n_x_units entries of one rng.permutation(U) "candidate"
(rng = numpy.random.default_rng(seed): the draw of mmd_permutation_null, on the host) and the same formula is evaluated
on the same graph; the observed value is the identity labelling through the same code.
    nn_p_value = (1 + #{T_p >= T_obs}) / (1 + P);   a draw that leaves a side without edges is NaN and counts as exceeding.
The relabelling is over UNITS, so the test keeps its level on windowed data with or without the exclusion - but without it
the accuracy is near 1 under the null as well and the test has little power left (README)."""
import warnings

import numpy as np
import torch

from .. import hip_ops as ops
from ..data import AudioMetricsData
from ._groups import labelled_rows

NAN = float("nan")
PAIR_BLOCK = 1 << 23                     # (relabellings x triples) looked at in one numpy pass of the null


# ------------------------------------------------------------------ host: the null on (unit, unit, count) triples
def _unit_triples(unit_of_row, neighbor_unit, U):
    """(a, b, count): the edges (row, neighbour) aggregated by (unit of the row, unit of the neighbour)"""
    present = neighbor_unit >= 0
    a = np.broadcast_to(unit_of_row[:, None], neighbor_unit.shape)[present].astype(np.int64)
    b = neighbor_unit[present].astype(np.int64)
    pair, count = np.unique(a * U + b, return_counts=True)
    return pair // U, pair % U, count.astype(np.float64)


def _labelling_terms(unit_of_row, neighbor_unit, n_x_units, n_permutations, seed):
    """(candidate term, reference term) of the statistic as float64 [1 + P]: entry 0 the identity labelling (the first
    n_x_units units are the candidate), entry p the p-th relabelling.  Every sum is an integer below 2^53: exact."""
    unit_of_row = np.asarray(unit_of_row)
    neighbor_unit = np.asarray(neighbor_unit)
    if unit_of_row.ndim != 1 or unit_of_row.dtype.kind not in "iu" or (unit_of_row.size and unit_of_row.min() < 0):
        raise ValueError(f"unit_of_row must hold one non-negative integer per row, got {unit_of_row.dtype} {unit_of_row.shape}")
    if neighbor_unit.ndim != 2 or neighbor_unit.shape[0] != unit_of_row.shape[0] or neighbor_unit.dtype.kind not in "iu":
        raise ValueError(f"neighbor_unit must be an integer array [rows, k] (-1: no neighbour), got {neighbor_unit.dtype} "
                         f"{neighbor_unit.shape} for {unit_of_row.shape[0]} rows")
    U = int(unit_of_row.max()) + 1 if unit_of_row.size else 0
    if neighbor_unit.size and int(neighbor_unit.max()) >= U:
        raise ValueError("neighbor_unit names a unit that no row belongs to")
    n_x_units, P = int(n_x_units), int(n_permutations)
    if not 1 <= n_x_units < U:
        raise ValueError(f"n_x_units={n_x_units} must leave both sides at least one of the {U} units")
    if P < 1:
        raise ValueError(f"n_permutations={n_permutations} must be at least 1")
    a, b, count = _unit_triples(unit_of_row, neighbor_unit.astype(np.int64), U)
    total = float(count.sum())
    out_deg = np.bincount(a, weights=count, minlength=U)         # edges that leave a unit / that arrive at it
    in_deg = np.bincount(b, weights=count, minlength=U)
    rng = np.random.default_rng(seed)
    L = np.zeros((P + 1, U), dtype=bool)
    L[0, :n_x_units] = True
    for p in range(1, P + 1):
        L[p, rng.permutation(U)[:n_x_units]] = True
    e_x = L @ out_deg                                            # edges from candidate-labelled rows
    to_x = L @ in_deg
    s_x = np.empty(P + 1, dtype=np.float64)
    step = max(1, PAIR_BLOCK // max(1, len(a)))
    for lo in range(0, P + 1, step):
        blk = L[lo:lo + step]
        s_x[lo:lo + step] = (blk[:, a] & blk[:, b]) @ count
    e_y = total - e_x
    s_y = total - e_x - to_x + s_x                               # neither end candidate-labelled
    with np.errstate(invalid="ignore", divide="ignore"):
        acc_x = np.where(e_x > 0, s_x / e_x, NAN)
        acc_y = np.where(e_y > 0, s_y / e_y, NAN)
    return acc_x, acc_y


def nn_permutation_null(unit_of_row, neighbor_unit, n_x_units, n_permutations=999, seed=0):
    """(T_obs, null, p) of the balanced nearest-neighbour accuracy under relabellings of units - host numpy, no GPU.
    unit_of_row: the unit of every row of the graph (integers 0 .. U - 1, the candidate's units first: units 0 ..
    n_x_units - 1 are the candidate under the identity labelling).  neighbor_unit: integer [rows, k], the unit of each of
    the row's neighbours, -1 where there is none.  The edges are aggregated to (unit, unit, count) triples; the labellings
    come from rng = numpy.random.default_rng(seed): for each relabelling the first n_x_units entries of one
    rng.permutation(U) are the candidate.  T = 1/2 (S_x / E_x + S_y / E_y) (module text); T_obs is the same code at the
    identity labelling.  null: float64 numpy [P]; p = (1 + #{T_p >= T_obs}) / (1 + P).  A draw that leaves a side without
    edges has no statistic: its null entry is NaN and it counts as exceeding."""
    acc_x, acc_y = _labelling_terms(unit_of_row, neighbor_unit, n_x_units, n_permutations, seed)
    T = 0.5 * (acc_x + acc_y)
    t_obs, null = float(T[0]), T[1:].copy()
    exceed = int(np.count_nonzero(~(null < t_obs)))               # NaN (no statistic) counts as exceeding
    return t_obs, null, (1.0 + exceed) / (1.0 + len(null))


def _null_summary(null):
    """(mean, population standard deviation, 95 % quantile) of the draws that have a statistic"""
    have = null[~np.isnan(null)]
    if have.size == 0:
        return NAN, NAN, NAN
    return float(have.mean()), float(have.std()), float(np.quantile(have, 0.95))


# ------------------------------------------------------------------ the device side
def _side(data, groups, what, name):
    """(stored rows, their number, dense unit id per row as int64 numpy or None, number of units) - no device call"""
    if groups is not None:
        rows, n, labels = labelled_rows(data, groups, what, f"its {name} set")
        _, inverse = np.unique(np.asarray(labels.cpu()), return_inverse=True)
        inverse = inverse.reshape(-1).astype(np.int64)
        units = int(inverse.max()) + 1
    else:
        rows, inverse = getattr(data, "embeddings", None), None
        n = int(rows.shape[0]) if rows is not None else 0
        if rows is None or n == 0:
            raise ValueError(f"{what} scores the stored rows of its {name} set, which keeps none "
                             f"(store_embeddings={getattr(data, 'store_embeddings', None)})")
        units = n
    if rows.dtype != torch.float32:
        raise NotImplementedError(f"{what}: the {name} set holds {rows.dtype} rows; the search takes float32 rows (the float64 "
                                  "matrix-core form is not implemented)")
    if units < 2:
        raise ValueError(f"{what}: the {name} set has {units} unit(s); a relabelling needs at least 2 on each side")
    return rows, n, inverse, units


def pooled_neighbor_graph(rows_x, rows_y, k, unit_x=None, unit_y=None):
    """int64 device tensor [n + m, k]: for every pooled row (the rows of rows_x, then those of rows_y) the pooled indices of
    its k nearest pooled rows outside its own unit, ascending by distance, ties to the smaller pooled index, -1 where there
    are fewer.  unit_x / unit_y: int32 device vectors (one unit id per row; the two sides' ids are never compared with
    each other) or None: every row of that side its own unit.  Four searches, one stable sort per side; stream-ordered."""
    n = int(rows_x.shape[0])

    def own(rows, unit):
        if unit is None:
            return ops.knn_search(rows, rows, k, self_offset=0, squared=True)
        return ops.knn_search_groups(rows, rows, k, unit, unit, squared=True)

    def merged(in_cand, in_ref):
        dist = torch.cat([in_cand[0], in_ref[0]], dim=1)
        idx = torch.cat([in_cand[1], torch.where(in_ref[1] >= 0, in_ref[1] + n, in_ref[1])], dim=1)
        order = torch.sort(dist, dim=1, stable=True)[1][:, :k]      # the candidate-side list first: ties to the smaller index
        return torch.gather(idx, 1, order)

    top = merged(own(rows_x, unit_x), ops.knn_search(rows_x, rows_y, k, squared=True))
    bottom = merged(ops.knn_search(rows_y, rows_x, k, squared=True), own(rows_y, unit_y))
    return torch.cat([top, bottom], dim=0)


def nearest_neighbor_two_sample_test(cand: AudioMetricsData, ref: AudioMetricsData, groups=None, ref_groups=None, k=1,
                                     n_permutations=999, seed=0, return_rows=False):
    """Do the stored rows of candidate set `cand` and of reference set `ref` come from one law?  The balanced
    leave-unit-out k-NN accuracy on the pooled rows and its permutation test over units (see the module text for every
    definition; they are this build's).

    groups / ref_groups: one integer label per stored row (the song a window comes from; any order, any values).  A row's
    neighbours are then taken outside its own song, and songs - not windows - are relabelled.  PASS THEM WHENEVER THE ROWS
    ARE WINDOWS OF TRACKS: without them nn_accuracy is near 1 for two samples of one law.  Fewer than 2 units on a side
    raise ValueError.  float32 rows on one GPU; 1 <= k <= 32.

    Returns {"nn_accuracy": 1/2 for indistinguishable sets, 1 for separated ones; "nn_accuracy_candidate",
    "nn_accuracy_reference": its two terms; "nn_p_value": small says the sets are distinguishable; "nn_null_mean",
    "nn_null_std", "nn_null_q95": of the relabellings that have a statistic; "nn_units": (candidate, reference) units that
    take part; "nn_n_permutations", "nn_k", "nn_rows_nonfinite"}.  return_rows=True adds "candidate_same_share" float64 [n]:
    the share of a clip's neighbours that are candidate rows ("this clip sits among fakes"; NaN without neighbours),
    "reference_same_share" [m]: the share that are reference rows, and "candidate_neighbors" [n, k], "reference_neighbors"
    [m, k]: int64 pooled indices (candidate rows first), -1 for none.  A row with a NaN or inf element is in nothing: it
    has no neighbours, is nobody's neighbour, is counted in nn_rows_nonfinite and ONE RuntimeWarning names the count.
    This is not a metric name of AudioMetrics.evaluate()."""
    what = "nearest_neighbor_two_sample_test"
    k, P = int(k), int(n_permutations)
    if not 1 <= k <= ops.KNN_SEARCH_MAX_K:
        raise ValueError(f"k={k} must be in 1 .. {ops.KNN_SEARCH_MAX_K}")
    if P < 1:
        raise ValueError(f"n_permutations={n_permutations} must be at least 1")
    rows_x, n, unit_x, units_x = _side(cand, groups, what, "candidate")
    rows_y, m, unit_y, units_y = _side(ref, ref_groups, what, "reference")
    if rows_x.shape[1] != rows_y.shape[1]:
        raise ValueError(f"{what}: feature widths differ: {rows_x.shape[1]} and {rows_y.shape[1]}")
    if rows_x.device != rows_y.device:
        raise ValueError(f"{what}: the sets live on {rows_x.device} and {rows_y.device}; a single GPU only")

    device = rows_x.device
    ids = [None if u is None else ops.upload_host_array(u.astype(np.int32), device) for u in (unit_x, unit_y)]
    graph = pooled_neighbor_graph(rows_x, rows_y, k, ids[0], ids[1])
    bad = torch.cat([~torch.isfinite(rows_x).all(dim=1), ~torch.isfinite(rows_y).all(dim=1)])
    host = torch.cat([graph, bad.to(torch.int64)[:, None]], dim=1).cpu().numpy()       # the one read-back
    graph, bad = host[:, :k].copy(), host[:, k] != 0
    nonfinite = int(bad.sum())

    # units of the rows that take part, the candidate's first, numbered densely
    unit = np.concatenate([np.arange(n) if unit_x is None else unit_x, units_x + (np.arange(m) if unit_y is None else unit_y)])
    used = np.unique(unit[~bad])
    n_x_units = int(np.searchsorted(used, units_x))
    if n_x_units < 2 or len(used) - n_x_units < 2:
        raise ValueError(f"{what}: {n_x_units} candidate and {len(used) - n_x_units} reference unit(s) are left once the rows with "
                         "a non-finite element are set aside; a relabelling needs at least 2 on each side")
    dense = np.full(units_x + units_y, -1, dtype=np.int64)
    dense[used] = np.arange(len(used))
    unit = dense[unit]
    neighbor_unit = np.where(graph >= 0, unit[np.maximum(graph, 0)], -1)
    acc_x, acc_y = _labelling_terms(unit[~bad], neighbor_unit[~bad], n_x_units, P, seed)
    T = 0.5 * (acc_x + acc_y)
    null = T[1:]
    exceed = int(np.count_nonzero(~(null < T[0])))
    mean, std, q95 = _null_summary(null)
    out = {"nn_accuracy": float(T[0]), "nn_accuracy_candidate": float(acc_x[0]), "nn_accuracy_reference": float(acc_y[0]),
           "nn_p_value": (1.0 + exceed) / (1.0 + P), "nn_null_mean": mean, "nn_null_std": std, "nn_null_q95": q95,
           "nn_units": (n_x_units, len(used) - n_x_units), "nn_n_permutations": P, "nn_k": k, "nn_rows_nonfinite": nonfinite}
    if return_rows:
        present = (graph >= 0).sum(axis=1).astype(np.float64)
        in_cand = ((graph >= 0) & (graph < n)).sum(axis=1).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            same = np.where(present > 0, np.where(np.arange(n + m) < n, in_cand, present - in_cand) / present, NAN)
        out.update(candidate_same_share=same[:n].copy(), reference_same_share=same[n:].copy(),
                   candidate_neighbors=graph[:n].copy(), reference_neighbors=graph[n:].copy())
    if nonfinite:
        warnings.warn(f"{what}: {nonfinite} row(s) hold a NaN or inf element and take part in nothing", RuntimeWarning, stacklevel=2)
    return out
