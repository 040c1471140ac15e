"""Numpy-float32 restatement of the per-sample realism / ball count / rarity of csrc/sample_scores.hip: the oracle of
tests/test_gpu_sample_scores.py and tests/test_fidelity_cpu.py.  Nothing here imports the package.

On LATTICE inputs (small-integer rows) every norm, inner product and squared distance is an exact f32 integer whatever
the order of the additions, and everything behind it - sqrt, r * r, the division, the threshold search - is one correctly
rounded IEEE operation in numpy float32 as on the device.  The oracle is therefore bit-exact and owes nothing to any
library call."""
import numpy as np

F32 = np.float32


def int_rows(seed, n, d):
    """Small-integer rows in -3 .. 3 (kmeans_reference.int_rows)."""
    return np.random.default_rng(seed).integers(-3, 4, size=(n, d)).astype(F32)


def lattice_case(n, m, d, seed, duplicates=False):
    """(samples x [n, d], manifold rows y [m, d]) of the tie-heavy lattice recipe, in this order:
    1 (duplicates) rows 3000 .. 3099 of y := rows 100 .. 199 - equal rows, the copies in a later column chunk;
    2 the first n / 3 samples are rows 100, 101, .. of y (wrapping at m) with +1 on three coordinates: near the manifold;
    3 +2 on every second coordinate of the last n / 3 samples: off the manifold."""
    y, x = int_rows(seed, m, d), int_rows(seed + 1, n, d)
    if duplicates:
        y[3000:3100] = y[100:200]
    third = n // 3
    x[:third] = y[(100 + np.arange(third)) % m]
    x[:third, :3] += 1
    x[n - third:, ::2] += 2
    return x, y


def exact_d2(x, y):
    """Squared distances of integer rows: exact in int64, and exact as f32 while below 2^24 (asserted)."""
    xi, yi = x.astype(np.int64), y.astype(np.int64)
    d2 = (xi * xi).sum(1)[:, None] + (yi * yi).sum(1)[None, :] - 2 * xi @ yi.T
    assert d2.min() >= 0 and d2.max() < 2 ** 24
    return d2.astype(F32)


def radii_of_d2(d2_self, k):
    """k-NN radii from a self-distance matrix: sqrt of the (k+1)-th smallest entry of every row (the row itself is one of
    them); +inf where the set has no k-th neighbour."""
    m = d2_self.shape[0]
    if m <= k:
        return np.full(m, np.inf, dtype=F32)
    return np.sqrt(np.sort(d2_self, axis=1)[:, k].astype(F32))


def threshold_of_radius(r):
    """T(r) = min { t : sqrt_rn(t) >= r } in f32, so that  sqrt_rn(d2) < r  <=>  d2 < T(r): start at r * r, walk down while
    the predecessor still reaches r, walk up until the value reaches it (at most 8 steps each way)."""
    r = F32(r)
    if not r > 0:
        return F32(0)
    if np.isinf(r):
        return r
    c = F32(r * r)
    for _ in range(8):
        p = np.nextafter(c, F32(-np.inf))
        if c > 0 and np.sqrt(p) >= r:
            c = p
        else:
            break
    for _ in range(8):
        if np.sqrt(c) < r:
            c = np.nextafter(c, F32(np.inf))
        else:
            break
    return F32(c)


def scores_from_d2(d2, r):
    """The five outputs from an f32 [n, m] matrix of squared distances (NaN counts as +inf) and f32 radii [m]:
    (realism f32, realism_index i64, ball_count i32, rarity f32, rarity_index i64), the definition without any gate."""
    d2 = np.asarray(d2, dtype=F32).copy()
    d2[np.isnan(d2)] = np.inf
    r = np.asarray(r, dtype=F32)
    rs = np.where(r > 0, r, F32(0)).astype(F32)                       # not > 0 (zero, negative, NaN): nobody's ball
    thr = np.array([threshold_of_radius(v) for v in rs], dtype=F32)
    member = d2 < thr[None, :]
    with np.errstate(all="ignore"):
        r2 = (rs * rs).astype(F32)
        q = (r2[None, :] / d2).astype(F32)
    q[np.isnan(q)] = 0                                                # 0 / 0, inf / inf
    qmax = q.max(axis=1)
    realism = np.sqrt(qmax).astype(F32)
    realism_index = np.where(qmax > 0, q.argmax(axis=1), -1).astype(np.int64)     # argmax: the first maximum
    count = member.sum(axis=1).astype(np.int32)
    n = d2.shape[0]
    rarity, rarity_index = np.zeros(n, dtype=F32), np.full(n, -1, dtype=np.int64)
    for i in range(n):
        cols = np.flatnonzero(member[i])
        if cols.size:
            best = rs[cols].min()
            rarity[i] = best
            rarity_index[i] = cols[rs[cols] == best][0]
    return realism, realism_index, count, rarity, rarity_index


def tie_counts(d2, r):
    """(samples whose best ratio is attained by more than one column, in-manifold samples whose smallest ball radius is
    attained by more than one member column): how hard a case exercises the tie rule."""
    r = np.asarray(r, dtype=F32)
    rs = np.where(r > 0, r, F32(0)).astype(F32)
    thr = np.array([threshold_of_radius(v) for v in rs], dtype=F32)
    member = d2 < thr[None, :]
    with np.errstate(all="ignore"):
        q = ((rs * rs).astype(F32)[None, :] / d2).astype(F32)
    q[np.isnan(q)] = 0
    realism_ties = int(((q == q.max(axis=1)[:, None]).sum(axis=1) > 1).sum())
    rarity_ties = 0
    for i in range(d2.shape[0]):
        cols = np.flatnonzero(member[i])
        if cols.size and (rs[cols] == rs[cols].min()).sum() > 1:
            rarity_ties += 1
    return realism_ties, rarity_ties


# (n, m, d, k, duplicates): the lattice cases both test files run
LATTICE_CASES = [(130, 300, 40, 5, False), (130, 300, 64, 3, False), (257, 130, 40, 5, False), (130, 4000, 40, 5, True)]


def lattice_oracle(n, m, d, k, duplicates, seed=7):
    """Everything a test needs of one lattice case: rows, radii and the five expected outputs."""
    x, y = lattice_case(n, m, d, seed, duplicates)
    r = radii_of_d2(exact_d2(y, y), k)
    d2 = exact_d2(x, y)
    return {"x": x, "y": y, "r": r, "d2": d2, "want": scores_from_d2(d2, r), "tie_heavy": duplicates}


def check_lattice_is_not_degenerate(case, tie_heavy):
    """The conditions that keep a lattice case meaningful: rows inside and outside the manifold, no zero radius, and - for
    the case with duplicated manifold rows, which is there for the tie rule - enough exact ties in both reductions."""
    _, _, count, _, _ = case["want"]
    inside = float((count > 0).mean())
    realism_ties, rarity_ties = tie_counts(case["d2"], case["r"])
    assert 0 < (count > 0).sum() < len(count), inside
    assert (case["r"] > 0).all()
    if tie_heavy:
        assert realism_ties >= 10 and rarity_ties >= 10, (realism_ties, rarity_ties)
    return inside, realism_ties, rarity_ties
