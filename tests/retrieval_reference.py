"""The definition of the retrieval ranks (csrc/retrieval.hip, metrics/retrieval.py) in numpy: a plain module, imported by name.

  * ranks_from_scores: thresholds, positives and counts from ANY score matrix u [N, M] (NaN = no score) - the definition
    itself, shared by the f64 reference and the f32 bits oracle;
  * scores_f64 / sandwich: the f64 scores and the lo / hi counts that bracket what f32 arithmetic may return;
  * lattice rows and lattice_scores: integer-valued rows, small enough that every dot product and norm is exact in f32 in
    any order, so that w = float32(1) / sqrt(float32(norm)) and u = acc * w are single correctly rounded numpy float32
    operations - the bits the device must return;
  * summary: the table arithmetic, written directly."""
import math

import numpy as np

SHAPES = [(130, 300, 40), (130, 300, 64), (257, 130, 40), (130, 1, 40), (130, 4000, 40)]


# ---------------------------------------------------------------------------------------------------- positives
def paired_positives(n):
    return [np.array([i], dtype=np.int64) for i in range(n)]


def label_positives(q_labels, g_labels):
    """P_i = the gallery rows with the query's label, ascending."""
    g_labels = np.asarray(g_labels)
    return [np.flatnonzero(g_labels == l).astype(np.int64) for l in np.asarray(q_labels)]


def segments(positives):
    """(pos_start, pos_count, pos_columns) int64: one segment per row, nothing shared."""
    counts = np.array([len(p) for p in positives], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    cols = np.concatenate(positives).astype(np.int64) if counts.sum() else np.zeros(0, dtype=np.int64)
    return starts, counts, cols


# ---------------------------------------------------------------------------------------------------- the definition
def ranks_from_scores(u, positives, q_group=None, g_group=None):
    """{better, tied int32 [N]; t (dtype of u), positive int64, n_pos, n_pos_own_group int32, negatives int64} from the score
    matrix u [N, M], NaN = the pair has no score.  Unranked rows: better = tied = positive = -1, t = NaN."""
    n, m = u.shape
    better, tied = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    positive = np.full(n, -1, np.int64)
    t = np.full(n, np.nan, u.dtype)
    n_pos, n_own, negatives = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64)
    for i in range(n):
        p = np.asarray(positives[i], dtype=np.int64)
        is_pos = np.zeros(m, bool)
        is_pos[p] = True
        neg = ~is_pos
        if q_group is not None:
            neg &= g_group != q_group[i]
            n_own[i] = int(np.count_nonzero(g_group[p] == q_group[i]))
        n_pos[i] = len(p)
        negatives[i] = int(np.count_nonzero(neg))
        row = u[i]
        scored = p[~np.isnan(row[p])]
        if len(scored) == 0:
            continue
        t[i] = row[scored].max()
        positive[i] = scored[row[scored] == t[i]].min()
        with np.errstate(invalid="ignore"):
            better[i] = int(np.count_nonzero(neg & (row > t[i])))
            tied[i] = int(np.count_nonzero(neg & (row == t[i])))
    return {"better": better, "tied": tied, "t": t, "positive": positive, "n_pos": n_pos, "n_pos_own_group": n_own,
            "negatives": negatives}


# ---------------------------------------------------------------------------------------------------- f64 and its sandwich
def scores_f64(q, g, cosine):
    """(s [N, M] f64, eps [N, M]): s_ij = <q_i, g_j> omega_j with omega_j = 1 / |g_j| (cosine) or 1, and the generous
    first-order bound eps_ij = (2 D + 16) 2^-24 |q_i| |g_j| omega_j on what the f32 fmaf chain, norm, root, division and
    product may be off by."""
    q64, g64 = q.astype(np.float64), g.astype(np.float64)
    qn, gn = np.sqrt((q64 * q64).sum(1)), np.sqrt((g64 * g64).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        omega = 1.0 / gn if cosine else np.ones_like(gn)
        s = (q64 @ g64.T) * omega[None, :]
        eps = (2 * q.shape[1] + 16) * 2.0 ** -24 * qn[:, None] * (gn * omega)[None, :]
    return s, eps


def sandwich(q, g, positives, cosine, q_group=None, g_group=None):
    """(lo, hi, ranked): lo_i = #{neg j : s_ij - eps_ij > t_i + e_i}, hi_i = #{neg j : s_ij + eps_ij > t_i - e_i}, e_i the
    largest eps among the row's positives; ranked_i = the row has a positive."""
    s, eps = scores_f64(q, g, cosine)
    n, m = s.shape
    lo, hi, ranked = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, bool)
    for i in range(n):
        p = np.asarray(positives[i], dtype=np.int64)
        if len(p) == 0:
            continue
        ranked[i] = True
        neg = np.ones(m, bool)
        neg[p] = False
        if q_group is not None:
            neg &= g_group != q_group[i]
        t, e = s[i, p].max(), eps[i, p].max()
        lo[i] = int(np.count_nonzero(neg & (s[i] - eps[i] > t + e)))
        hi[i] = int(np.count_nonzero(neg & (s[i] + eps[i] > t - e)))
    return lo, hi, ranked


def sandwich_rows(n, m, d):
    """The rows of the sandwich test: seed = N + M + D, q then g standard normal float32, the first p = min(N, M) gallery
    rows pulled towards their query by a = linspace(0, 0.5, p); positives by label: row i <-> column i for i < p, every
    other row a label of its own."""
    rng = np.random.default_rng(n + m + d)
    q = rng.standard_normal((n, d)).astype(np.float32)
    g = rng.standard_normal((m, d)).astype(np.float32)
    p = min(n, m)
    a = np.linspace(0.0, 0.5, p)[:, None]
    g[:p] = (a * q[:p] + (1.0 - a) * g[:p]).astype(np.float32)
    q_labels = np.arange(n, dtype=np.int64)
    g_labels = np.arange(m, dtype=np.int64)
    q_labels[p:] += m                                   # a label no gallery row carries
    g_labels[p:] += n + m                               # ... and labels no query carries
    return q, g, q_labels, g_labels


# ---------------------------------------------------------------------------------------------------- lattice rows, f32 bits
def lattice_rows(seed, n, d, lo=-2, hi=2):
    """Integer-valued float32 rows in [lo, hi]: with d <= 64 every dot product and norm is an integer below 2^24."""
    return np.random.default_rng(seed).integers(lo, hi + 1, size=(n, d)).astype(np.float32)


def lattice_scores(q, g, cosine):
    """(u float32 [N, M], wq float32 [N]): the bits of the device for lattice rows.  acc is exact whatever the order; w and
    u are one correctly rounded float32 operation each.  A zero row has w = inf and u = 0 * inf = NaN: no score."""
    acc = (q.astype(np.float64) @ g.astype(np.float64).T)
    assert np.all(np.abs(acc[np.isfinite(acc)]) < 2 ** 24)
    acc = (acc + 0.0).astype(np.float32)                # (-0 -> +0: the chain starts from +0)

    def weights(x):
        norm = (x.astype(np.float64) ** 2).sum(1).astype(np.float32)
        if not cosine:
            return np.ones(len(x), np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.float32(1.0) / np.sqrt(norm)
    wq, wg = weights(q), weights(g)
    with np.errstate(invalid="ignore"):
        u = acc * wg[None, :]
    assert u.dtype == np.float32 and wq.dtype == np.float32
    return u, wq


def lattice_oracle(q, g, positives, cosine, q_group=None, g_group=None):
    """ranks_from_scores on the f32 bits, plus "score": t (dot) or fmul_rn(t, w^Q) (cosine)."""
    u, wq = lattice_scores(q, g, cosine)
    out = ranks_from_scores(u, positives, q_group, g_group)
    with np.errstate(invalid="ignore"):
        out["score"] = (out["t"] * wq).astype(np.float32) if cosine else out["t"].copy()
    return out


def unit_lattice_rows(seed, n, d):
    """Unit-norm rows that are exact in f32: four entries of +-0.5, the rest 0 (|row|^2 = 4 * 0.25 = 1; every dot product
    is a multiple of 0.25)."""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, d), np.float32)
    for i in range(n):
        x[i, rng.choice(d, 4, replace=False)] = rng.choice([-0.5, 0.5], 4)
    return x


# ---------------------------------------------------------------------------------------------------- the table, directly
def summary(ranks, tied, ks=(1, 5, 10), ties="optimistic", negatives=None, units=None):
    """The figures of retrieval_summary with plain loops."""
    rows = [i for i, r in enumerate(ranks) if r >= 1]
    eff = []
    for i in rows:
        r = float(ranks[i])
        if ties == "pessimistic":
            r += float(tied[i])
        elif ties == "mean":
            r += float(tied[i]) / 2.0
        eff.append(r)
    n = len(eff)

    def std_error(h):
        mean = sum(h) / n
        if units is None:
            return math.sqrt(sum((v - mean) ** 2 for v in h) / (n - 1) / n) if n >= 2 else float("nan")
        per = {}
        for i, v in zip(rows, h):
            per[units[i]] = per.get(units[i], 0.0) + (v - mean)
        G = len(per)
        return math.sqrt(G / (G - 1.0) * sum(v * v for v in per.values())) / n if G >= 2 else float("nan")
    out = {}
    for k in ks:
        hit = [1.0 if r <= k else 0.0 for r in eff]
        out[f"recall_at_{k}"] = sum(hit) / n
        out[f"recall_at_{k}_std_error"] = std_error(hit)
        if negatives is not None:
            out[f"chance_recall_at_{k}"] = sum(min(1.0, k / (negatives[i] + 1.0)) for i in rows) / n
    rr = [1.0 / r for r in eff]
    s = sorted(eff)
    out["median_rank"] = s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2.0
    out["mean_rank"] = sum(eff) / n
    out["mrr"] = sum(rr) / n
    out["mrr_std_error"] = std_error(rr)
    out["map_at_10"] = sum(v if r <= 10 else 0.0 for v, r in zip(rr, eff)) / n
    out["retrieval_rows_ranked"] = float(n)
    out["retrieval_rows_unranked"] = float(len(ranks) - n)
    out["retrieval_ties"] = float(sum(tied[i] for i in rows)) if tied is not None else 0.0
    return out
