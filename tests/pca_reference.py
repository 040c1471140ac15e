"""Float64 oracles for the PCA path (csrc/eigh.hip, projection.IncrementalPCA): plain numpy, no device, no scikit-learn.

  eigh_check          the four error measures of a computed eigendecomposition against np.linalg.eigh
  matrix families     gram / graded / clustered / near_pair / rank_r / diagonal, all seeded, all built in float64
  pca_gram_route      scikit-learn's IncrementalPCA.partial_fit restated through the Gram matrix of its stacked matrix
  component_bound     Davis-Kahan: how far a perturbation of norm delta can turn an eigenvector
  PCA_CASES           (D, n_components, row splits, note) of the incremental fits the device is checked on

Everything here is deterministic: the same call gives the same bytes."""
import functools

import numpy as np

import inputs

E1_LIMIT, E2_LIMIT, E3_LIMIT = 1e-10, 1e-10, 1e-9        # the limits test_own_eigensolver_and_projection asserts
SHAPE_SWEEP = (1, 2, 3, 15, 16, 17, 31, 32, 33, 48, 49, 100, 130, 257, 513, 528, 768, 1030, 1040)
SCALE_EXPONENTS = (-600, -300, -260, 260, 300, 600)


# ------------------------------------------------------------------ eigensolver
def eigh_check(a, evals, evecs):
    """Errors of (evals[D] descending, evecs[D, D] with row i = vector i) as an eigendecomposition of the symmetric `a`,
    all relative to lam0 = max |lambda| of np.linalg.eigh(a) (lam0 = 0, the zero matrix: absolute):
      e1       max |evals - lambda|
      sorted   evals is non-increasing
      e2       max |V V^T - I|   (absolute)
      e3       max |V A V^T - diag(evals)|
    A itself is divided by lam0 before V A V^T is formed, so that a matrix near the end of the f64 range is measured
    without overflow."""
    a = np.asarray(a, np.float64)
    evals, evecs = np.asarray(evals, np.float64), np.asarray(evecs, np.float64)
    lam = np.linalg.eigvalsh(a)[::-1]
    lam0 = float(np.max(np.abs(lam)))
    unit = lam0 if lam0 > 0 else 1.0
    d = a.shape[0]
    with np.errstate(all="ignore"):
        e1 = float(np.max(np.abs(evals / unit - lam / unit)))
        e2 = float(np.max(np.abs(evecs @ evecs.T - np.eye(d))))
        e3 = float(np.max(np.abs(evecs @ (a / unit) @ evecs.T - np.diag(evals / unit))))
    bad = float("inf")
    return dict(lam=lam, lam0=lam0, e1=e1 if np.isfinite(e1) else bad, sorted=bool(np.all(np.diff(evals) <= 0)),
                e2=e2 if np.isfinite(e2) else bad, e3=e3 if np.isfinite(e3) else bad)


def _orthogonal(rng, d):
    q, r = np.linalg.qr(rng.standard_normal((d, d)))
    return q * np.where(np.diagonal(r) < 0, -1.0, 1.0)            # the QR with a positive diagonal: unique


def _from_spectrum(seed, lam):
    q = _orthogonal(np.random.default_rng(seed), len(lam))
    a = (q * np.asarray(lam, np.float64)) @ q.T
    return 0.5 * (a + a.T)


def gram(d, rows, seed=9):
    x = np.random.default_rng(seed + 1000 * d).standard_normal((rows, d)) * np.logspace(0, -2, d)
    return x.T @ x


def graded(d, decades, seed=11):
    return _from_spectrum(seed + 1000 * d, np.logspace(0, -decades, d))


CLUSTER_VALUES = (1.0, 0.5, 0.1)


def clustered_spectrum(d):
    sizes = [d - 2 * (d // 3), d // 3, d // 3]
    return np.concatenate([np.full(n, v) for n, v in zip(sizes, CLUSTER_VALUES)])


def clustered(d, seed=13):
    return _from_spectrum(seed + 1000 * d, clustered_spectrum(d))


def near_pair(d, seed=17):
    lam = np.logspace(0, -2, d)
    lam[1] = lam[0] * (1.0 - 1e-13)
    return _from_spectrum(seed + 1000 * d, lam)


def rank_r(d, r, seed=19):
    lam = np.zeros(d)
    lam[:r] = np.logspace(0, -1, r) if r > 1 else 1.0
    return _from_spectrum(seed + 1000 * d + r, lam)


DIAGONAL_KINDS = ("identity", "distinct", "ties")


def diagonal(d, kind, seed=23):
    rng = np.random.default_rng(seed + 1000 * d)
    if kind == "identity":
        v = np.full(d, 2.5)
    elif kind == "distinct":
        v = rng.permutation(np.arange(1, d + 1) * 0.375)
    elif kind == "ties":
        v = rng.permutation(np.repeat(np.arange(1, d // 4 + 2) * 0.75, 4)[:d])
    else:
        raise ValueError(kind)
    return np.diag(v)


def spectra_cases():
    """(name, matrix builder) of every spectrum case of the device test; the CPU test walks the same list."""
    out = []
    for d in (33, 130):
        out.append((f"graded12-{d}", lambda d=d: graded(d, 12)))
        out.append((f"near_pair-{d}", lambda d=d: near_pair(d)))
    for d in (48, 130):
        out.append((f"clustered-{d}", lambda d=d: clustered(d)))
    for d in (17, 130):
        for r in (0, 1, d // 3):
            out.append((f"rank{r}-{d}", lambda d=d, r=r: rank_r(d, r)))
    for d in (16, 40, 130):
        for kind in DIAGONAL_KINDS:
            out.append((f"diagonal-{kind}-{d}", lambda d=d, kind=kind: diagonal(d, kind)))
    return out


def scale_bases():
    return (("gram64", lambda: gram(64, 192)), ("graded130", lambda: graded(130, 6)))


def scaled(a, e):
    return np.ldexp(a, e)                                         # exact: no entry of the bases leaves the normal range


def cluster_projectors(evals, evecs, values, lam0):
    """Projector onto the rows of evecs whose eigenvalue is nearest to each of `values` (times lam0)."""
    evals = np.asarray(evals)
    nearest = np.argmin(np.abs(evals[:, None] / lam0 - np.asarray(values)[None, :]), axis=1)
    return [evecs[nearest == k].T @ evecs[nearest == k] for k in range(len(values))]


def component_bound(lams, i, delta):
    """4 delta / min_{j != i} |lam_i - lam_j|: Davis-Kahan's sin(theta) bound (2 delta / gap) for a symmetric perturbation
    of norm delta, doubled once more because the 2-norm of the difference of two aligned unit vectors is
    2 sin(theta / 2) <= sqrt(2) sin(theta)."""
    lams = np.asarray(lams, np.float64)
    gap = np.min(np.abs(np.delete(lams, i) - lams[i])) if len(lams) > 1 else np.inf
    return 4.0 * delta / gap if gap > 0 else np.inf


# ------------------------------------------------------------------ incremental PCA through the Gram matrix
PCA_CASES = (
    # D, n_components, row splits, note
    (5, 1, (7, 3), ""),
    (40, 6, (60, 1, 25), ""),
    (40, 40, (60, 1, 25), ""),
    (40, None, (12,), "first batch has fewer rows than columns"),
    (40, 6, (60, 25), "column 7 constant"),
    (130, 17, (50, 200, 1, 64), ""),
    (768, 64, (900, 300), ""),
)
PCA_SEED = 13100        # the seventh draw (7100, 8100, ...): the first whose (40, 40) fit keeps every gap wide enough for STAT_CAP
HELD_OUT_ROWS = 40


def case_id(case):
    d, p, splits, note = case
    return f"D{d}-p{p}-" + "_".join(str(s) for s in splits) + ("-const7" if "constant" in note else "")


def case_batches(case, index):
    """The float32 row batches of a case (inputs.decaying, the family the issue names) and a held-out batch."""
    d, _, splits, note = case
    seed = PCA_SEED + 100 * index
    out = [inputs.decaying(seed + i, n, d, decades=1.5, shift=0.3 * i) for i, n in enumerate(splits)]
    held = inputs.decaying(seed + 50, HELD_OUT_ROWS, d, decades=1.5, shift=0.2)
    if "constant" in note:
        for x in out + [held]:
            x[:, 7] = 0.625
    return out, held


def batch_stats(x):
    """(n, mean, unbiased covariance) of a batch in float64; one row has covariance 0, as the device statistics have."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    mean = x.mean(axis=0)
    xc = x - mean
    cov = xc.T @ xc / (n - 1) if n > 1 else np.zeros((x.shape[1], x.shape[1]))
    return n, mean, cov


def svd_flip_rows(vt):
    """svd_flip(u_based_decision=False): the entry of largest magnitude of every row becomes positive."""
    idx = np.argmax(np.abs(vt), axis=1)
    signs = np.sign(vt[np.arange(vt.shape[0]), idx])
    signs[signs == 0] = 1.0
    return vt * signs[:, None]


def pca_gram_route(state, x, n_components=None):
    """One IncrementalPCA.partial_fit of scikit-learn, through the Gram matrix of its stacked matrix
    [diag(s) C ; X - batch mean ; correction row] and np.linalg.eigh instead of the SVD.  `state` is None (first batch) or
    the dict an earlier call returned; the result carries the fitted attributes under scikit-learn's names plus
    "gram" (the matrix that was decomposed), "lams" (all of its D eigenvalues, descending) and "vt" (all D eigenvectors as
    rows, in that order)."""
    x = np.asarray(x, np.float64)
    n, d = x.shape
    mean_b = x.mean(axis=0)
    xc = x - mean_b
    scatter = xc.T @ xc
    var_b = np.diagonal(scatter) / n
    if state is None:
        p = min(n, d) if n_components is None else n_components
        n_total, mean, var = n, mean_b, var_b
        g = scatter
        rows = n
    else:
        p = state["components_"].shape[0]
        n_seen = state["n_samples_seen_"]
        n_total = n_seen + n
        mean = (n_seen * state["mean_"] + n * mean_b) / n_total
        delta = state["mean_"] - mean_b
        var = (state["var_"] * n_seen + var_b * n + delta * delta * (n_seen * n / n_total)) / n_total
        corr = np.sqrt((n_seen / n_total) * n) * delta
        c = state["components_"]
        g = (c.T * state["singular_values_"] ** 2) @ c + scatter + np.outer(corr, corr)
        rows = p + n + 1
    g = 0.5 * (g + g.T)
    lam, vec = np.linalg.eigh(g)
    lam, vt = np.maximum(lam[::-1], 0.0), svd_flip_rows(vec[:, ::-1].T)
    n_sv = min(rows, d)
    s2 = lam[:n_sv]
    ev = s2 / (n_total - 1)
    evr = s2 / np.sum(var * n_total)
    noise = float(ev[p:].mean()) if (p not in (n, d) and p < n_sv) else 0.0
    return dict(n_samples_seen_=n_total, n_components_=p, mean_=mean, var_=var, components_=vt[:p].copy(),
                singular_values_=np.sqrt(s2[:p]), explained_variance_=ev[:p].copy(), explained_variance_ratio_=evr[:p].copy(),
                noise_variance_=noise, gram=g, lams=lam, vt=vt)


class GramPCA:
    """The small class around pca_gram_route: partial_fit / transform with scikit-learn's attribute names."""

    def __init__(self, n_components=None):
        self.n_components = n_components
        self.state = None

    def partial_fit(self, x):
        self.state = pca_gram_route(self.state, x, self.n_components)
        for k, v in self.state.items():
            if k.endswith("_"):
                setattr(self, k, v)
        return self

    def transform(self, x):
        return (np.asarray(x, np.float64) - self.mean_) @ self.components_.T


_TRAJECTORIES = {}


def trajectory(index):
    """The oracle's state after every update of PCA_CASES[index] (computed once, shared by the tests, never modified)."""
    if index not in _TRAJECTORIES:
        case = PCA_CASES[index]
        batches, _ = case_batches(case, index)
        fit, states = GramPCA(case[1]), []
        for x in batches:
            states.append(fit.partial_fit(x).state)
        _TRAJECTORIES[index] = states
    return _TRAJECTORIES[index]


def null_threshold(delta):
    """Eigenvalues of a positive semi-definite matrix below 2 delta cannot be told from zero under a perturbation of norm
    delta; together they span the (numerical) null space, and only that SPACE is determined - the rows mode of the case
    whose first batch has fewer rows than columns keeps one component from it."""
    return 2.0 * delta


def component_bounds(state, delta):
    """(bound per kept component, mask of the kept components that lie in the numerical null space).  A null-space
    component is bounded as a member of its space: lams of the space are merged into one eigenvalue 0 before the gap is
    taken, and the test compares the part of the device's vector outside the oracle's space against the bound."""
    lams = state["lams"]
    null = lams <= null_threshold(delta)
    p = state["components_"].shape[0]
    merged = np.concatenate([lams[~null], [0.0]]) if null.any() else lams
    bounds = np.empty(p)
    for i in range(p):
        j = len(merged) - 1 if null[i] else i
        bounds[i] = component_bound(merged, j, delta)
    return bounds, null[:p]


def outside_null_space(state, delta, v):
    """Coordinates of v along the oracle's eigenvectors that are NOT in the numerical null space (zero for a null-space vector)."""
    return state["vt"][state["lams"] > null_threshold(delta)] @ v


def delta_statistics(state):
    return E3_LIMIT * state["lams"][0]


def delta_rows(state, dtype):
    """Norm of the Gram matrix's error when the batch statistics come from the device: the covariance limits the suite
    asserts (test_stats_full_size_vs_f64: 2e-7 |G|_F for float32 rows; test_float64_rows_keep_float64_statistics:
    1e-12 max|G| D for float64 rows) times (n - 1), on top of the statistics-mode limit."""
    g = state["gram"]
    if dtype == np.float32:
        return 2e-7 * float(np.linalg.norm(g)) + delta_statistics(state)
    return 1e-12 * float(np.max(np.abs(g))) * g.shape[0] + delta_statistics(state)


STAT_CAP, ROWS_CAP, SIGN_MARGIN = 1e-4, 1e-2, 1e-6


def sign_margins(state, null_mask):
    """Difference of the two largest |entries| of every kept component that is not a null-space component."""
    a = np.sort(np.abs(state["components_"]), axis=1)
    m = a[:, -1] - a[:, -2] if a.shape[1] > 1 else a[:, -1]
    return m[~null_mask]


@functools.lru_cache(maxsize=None)
def rows_mode_cases(dtype):
    """Indices of PCA_CASES checked in rows mode: every case but (40, 40, ...) when that one's bound misses ROWS_CAP."""
    keep = []
    for index, case in enumerate(PCA_CASES):
        worst = max(float(component_bounds(st, delta_rows(st, dtype))[0].max()) for st in trajectory(index))
        if worst <= ROWS_CAP or not (case[0] == 40 and case[1] == 40):
            keep.append(index)
    return keep


# ------------------------------------------------------------------ projection
PROJECT_SHAPES = (
    # N, D, p: every value of every axis, the corners, the 64-row / 16-component edges crossed together
    (1, 1, 1), (1000, 513, 33), (1, 513, 17), (1, 4, 16), (63, 3, 15), (63, 70, 33), (64, 4, 16), (64, 5, 1),
    (65, 5, 17), (65, 1, 33), (65, 513, 15), (1000, 1, 1), (1000, 3, 17), (1000, 70, 16), (64, 513, 33), (63, 4, 17),
    (65, 70, 15), (1, 5, 33), (64, 3, 1), (1000, 4, 15), (65, 3, 16),
)


def project_inputs(n, d, p, exact, seed=31):
    """(rows f64, mean, components): small integers (every product and partial sum exact in f64) or real values.  The rows
    are representable in float32 either way, so both row types see the same numbers."""
    rng = np.random.default_rng(seed + 7 * n + 1000 * d + p)
    if exact:
        return (rng.integers(-3, 4, (n, d)).astype(np.float64), rng.integers(-3, 4, d).astype(np.float64),
                rng.integers(-3, 4, (p, d)).astype(np.float64))
    return (rng.standard_normal((n, d)).astype(np.float32).astype(np.float64), rng.standard_normal(d),
            rng.standard_normal((p, d)))


def project_reference(x, mean, comp):
    """((x - mean) @ comp^T, the entry-wise error scale sum_d |x_d - mean_d| |c_d|)."""
    xc = np.asarray(x, np.float64) - mean
    return xc @ comp.T, np.abs(xc) @ np.abs(comp).T
