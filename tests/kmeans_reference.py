"""Float64 numpy restatement of the k-means kernels and of the MAUVE frontier: the oracle of tests/test_gpu_kmeans.py and
tests/test_kmeans_cpu.py.  Nothing here imports the package."""
import numpy as np


def int_rows(seed, n, d):
    """Small-integer rows: every product, norm and squared distance is exact in f32 (and far below 2^24)."""
    return np.random.default_rng(seed).integers(-3, 4, size=(n, d)).astype(np.float32)


def sq_distances(x, c):
    """float64 [N, K]: max(|x|^2 + |c|^2 - 2 x.c, 0)."""
    x64, c64 = np.asarray(x, dtype=np.float64), np.asarray(c, dtype=np.float64)
    return np.maximum((x64 * x64).sum(1)[:, None] + (c64 * c64).sum(1)[None, :] - 2.0 * x64 @ c64.T, 0.0)


def assign(x, c):
    """(labels: the FIRST argmin, d2 of it, gap to the second smallest distance (+inf for K = 1), inertia) in float64."""
    d2 = sq_distances(x, c)
    labels = np.argmin(d2, axis=1)
    best = d2[np.arange(len(d2)), labels]
    if d2.shape[1] > 1:
        rest = d2.copy()
        rest[np.arange(len(d2)), labels] = np.inf
        gap = rest.min(axis=1) - best
    else:
        gap = np.full(len(d2), np.inf)
    return labels, best, gap, float(best.sum())


def rounding_bound(x, c, d):
    """float64 [N, K]: the worst case of an f32 fmaf chain of D terms under the factor 2 plus the two f32 norm sums,
    b = (2 D + 4) 2^-24 (|x|^2 + |c|^2) - the bound tests/test_gpu_knn_search.py uses for the same arithmetic."""
    x64, c64 = np.asarray(x, dtype=np.float64), np.asarray(c, dtype=np.float64)
    return (2 * d + 4) * 2.0 ** -24 * ((x64 * x64).sum(1)[:, None] + (c64 * c64).sum(1)[None, :])


def update(x, labels, c_old):
    """(float64 [K, D] means - the old centroid where a cluster has no rows -, int64 [K] counts); labels < 0 are ignored."""
    x64 = np.asarray(x, dtype=np.float64)
    out = np.asarray(c_old, dtype=np.float64).copy()
    counts = np.zeros(len(out), dtype=np.int64)
    for k in range(len(out)):
        rows = x64[labels == k]
        counts[k] = len(rows)
        if len(rows):
            out[k] = rows.sum(axis=0) / len(rows)
    return out, counts


def ulp32(v):
    """Spacing of float32 at |v| (float64 array in, float64 array out)."""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def disjoint_mauve(scaling, n_points):
    """MAUVE of two histograms with disjoint supports, computed from the closed form of its frontier: the points are
    ((1 - lambda)^s, lambda^s), whatever the histograms are."""
    lam = np.linspace(1e-6, 1.0 - 1e-6, n_points)
    pts = np.concatenate([[(0.0, 1.0)], np.stack([(1.0 - lam) ** scaling, lam ** scaling], axis=1), [(1.0, 0.0)]])
    area = 0.0
    for a, b in ((0, 1), (1, 0)):
        s = pts[np.argsort(pts[:, a], kind="stable")]
        area += float(np.sum(np.diff(s[:, a]) * 0.5 * (s[1:, b] + s[:-1, b])))
    return 0.5 * area
