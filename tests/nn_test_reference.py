"""Float64 brute-force reference of the nearest-neighbour two-sample test (metrics/nn_test.py), written from its
definitions and sharing no code with it: the pooled graph with own-unit exclusion and ties to the smaller pooled index, the
statistic, and the null on a DENSE unit x unit matrix of edge counts."""
import numpy as np


def pooled_units(n, m, groups=None, ref_groups=None):
    """(unit of every pooled row, candidate units): candidate rows first; the two sides' units are distinct"""
    ux = np.arange(n) if groups is None else np.unique(np.asarray(groups), return_inverse=True)[1].reshape(-1)
    uy = np.arange(m) if ref_groups is None else np.unique(np.asarray(ref_groups), return_inverse=True)[1].reshape(-1)
    n_x_units = int(ux.max()) + 1
    return np.concatenate([ux, n_x_units + uy]), n_x_units


def pooled_graph(x, y, k, exclusion_unit):
    """int64 [n + m, k]: the k nearest pooled rows outside the row's exclusion unit, ascending by (d2, pooled index), -1 where
    there are fewer; a row with a non-finite element has no neighbours and is nobody's neighbour.  d2 in float64 (exact on
    integer-valued rows)."""
    z = np.concatenate([np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)])
    bad = ~np.isfinite(z).all(axis=1)
    z = np.where(bad[:, None], 0.0, z)
    sq = (z * z).sum(axis=1)
    d2 = np.maximum(sq[:, None] + sq[None, :] - 2.0 * z @ z.T, 0.0)
    d2[exclusion_unit[:, None] == exclusion_unit[None, :]] = np.inf
    d2[bad, :] = np.inf
    d2[:, bad] = np.inf
    if k == 1:
        order = np.argmin(d2, axis=1)[:, None]                     # the first of equal minima
    else:
        order = np.argsort(d2, axis=1, kind="stable")[:, :k]      # stable: equal distances stay in index order
    graph = np.where(np.isfinite(np.take_along_axis(d2, order, axis=1)), order, -1).astype(np.int64)
    if graph.shape[1] < k:                                         # fewer pooled rows than k
        graph = np.concatenate([graph, np.full((len(z), k - graph.shape[1]), -1, dtype=np.int64)], axis=1)
    return graph, bad


def accuracy_terms(graph, is_cand):
    """(S_x / E_x, S_y / E_y) of one labelling of the ROWS (bool per pooled row); NaN for a side without edges"""
    present = graph >= 0
    to_cand = present & is_cand[np.maximum(graph, 0)]
    e_x, e_y = int(present[is_cand].sum()), int(present[~is_cand].sum())
    s_x, s_y = int(to_cand[is_cand].sum()), int((present & ~to_cand)[~is_cand].sum())
    return (s_x / e_x if e_x else float("nan")), (s_y / e_y if e_y else float("nan"))


def dense_null(unit_of_row, neighbor_unit, n_x_units, n_permutations, seed):
    """(T_obs, null [P], p) from the dense U x U matrix of edge counts; the labellings of numpy.random.default_rng(seed):
    the first n_x_units entries of one rng.permutation(U) per relabelling"""
    U = int(unit_of_row.max()) + 1
    C = np.zeros((U, U), dtype=np.int64)
    for a, row in zip(unit_of_row, neighbor_unit):
        for b in row:
            if b >= 0:
                C[a, b] += 1

    def statistic(lab):
        s_x, e_x = int(lab @ C @ lab), int(lab @ C.sum(axis=1))
        s_y, e_y = int((1 - lab) @ C @ (1 - lab)), int((1 - lab) @ C.sum(axis=1))
        if e_x == 0 or e_y == 0:
            return float("nan")
        return 0.5 * (s_x / e_x + s_y / e_y)

    lab = np.zeros(U, dtype=np.int64)
    lab[:n_x_units] = 1
    t_obs = statistic(lab)
    rng = np.random.default_rng(seed)
    null = np.empty(n_permutations)
    for p in range(n_permutations):
        lab = np.zeros(U, dtype=np.int64)
        lab[rng.permutation(U)[:n_x_units]] = 1
        null[p] = statistic(lab)
    exceed = sum(1 for t in null if not t < t_obs)
    return t_obs, null, (1 + exceed) / (1 + n_permutations)


def two_sample_test(x, y, groups=None, ref_groups=None, k=1, n_permutations=999, seed=0, exclusion_by_row=False):
    """Every value nearest_neighbor_two_sample_test returns (return_rows=True), from the definitions.  exclusion_by_row:
    a row leaves out only itself when its neighbours are taken, while the relabelling still moves whole units."""
    n, m = len(x), len(y)
    unit, n_x_units = pooled_units(n, m, groups, ref_groups)
    graph, bad = pooled_graph(x, y, k, np.arange(n + m) if exclusion_by_row else unit)
    used = np.unique(unit[~bad])
    dense = np.full(int(unit.max()) + 1, -1, dtype=np.int64)
    dense[used] = np.arange(len(used))
    n_x_used = int((used < n_x_units).sum())
    unit = dense[unit]
    neighbor_unit = np.where(graph >= 0, unit[np.maximum(graph, 0)], -1)
    is_cand = np.arange(n + m) < n
    acc_x, acc_y = accuracy_terms(graph, is_cand)
    t_obs, null, p = dense_null(unit[~bad], neighbor_unit[~bad], n_x_used, n_permutations, seed)
    assert t_obs == 0.5 * (acc_x + acc_y) or (np.isnan(t_obs) and np.isnan(acc_x + acc_y))
    have = null[~np.isnan(null)]
    present = (graph >= 0).sum(axis=1)
    same = np.array([np.nan if present[i] == 0 else ((graph[i] >= 0) & ((graph[i] < n) == is_cand[i])).sum() / present[i]
                     for i in range(n + m)])
    return {"nn_accuracy": t_obs, "nn_accuracy_candidate": acc_x, "nn_accuracy_reference": acc_y, "nn_p_value": p,
            "nn_null_mean": float(have.mean()) if have.size else float("nan"),
            "nn_null_std": float(have.std()) if have.size else float("nan"),
            "nn_null_q95": float(np.quantile(have, 0.95)) if have.size else float("nan"),
            "nn_units": (n_x_used, len(used) - n_x_used), "nn_n_permutations": n_permutations, "nn_k": k,
            "nn_rows_nonfinite": int(bad.sum()), "candidate_same_share": same[:n], "reference_same_share": same[n:],
            "candidate_neighbors": graph[:n], "reference_neighbors": graph[n:]}
