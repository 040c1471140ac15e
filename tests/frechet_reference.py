"""float64 oracles and arithmetic models for the Frechet solver (frechet.hip, frechet_batch.hip, ns_engine.h) and the f32
statistics (stats.hip).  numpy only; nothing here runs on a device or reads a kernel's output.

Three kinds of thing live here:
  * oracles      closed forms and LAPACK evaluations of the definition (fd_closed, fd_psd, merge_f64, scatter_f64),
  * models       plain transcriptions of the arithmetic the kernels document (ns_model, stats_f32_model): they bound what
                 the documented method can deliver, so the device tests take their tolerances from them,
  * inputs       the seeded builders both the CPU validation and the device tests use, so a bound measured on the CPU is a
                 bound on the very matrices the device sees.
"""
import numpy as np

# ------------------------------------------------------------------ shared case tables
D_EDGES = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 97, 100, 130, 132]
COND = [1, 1e4, 1e8]
GENERAL_D = [5, 33, 65, 130]
RANK_DEFICIENT = [(33, 10, 200), (65, 20, 300), (5, 3, 40), (130, 40, 600), (17, 2, 100)]     # (D, rows_x, rows_y)
BUDGET_PAIR = (33, 1e4, 0)                                                                    # (D, cond, seed)
BUDGETS = [1, 2, 15, 16, 17, 31, 32, 64]
DEGENERATE_D = [1, 3, 33]
EQUAL_PAIR_COND = 1e2                                                                          # Cx = Cy: the product has its square

STATS_N = [2, 3, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1025, 2049]
STATS_D = [1, 3, 4, 5, 8, 24, 31, 32, 33, 34, 64, 96, 127, 128, 129, 131, 257]
SCATTER_N = [33, 257, 513]
SCATTER_D = [5, 33, 129]


def _sym(a):
    return 0.5 * (a + a.T)


# ------------------------------------------------------------------ inputs of the solver
def commuting_pair(d, cond, seed):
    """(mu_x, cx, mu_y, cy, tr_sqrt): Cx = Q diag(a) Q^T and Cy = Q diag(b) Q^T share their eigenvectors, so
    tr sqrt(Cx Cy) = sum sqrt(a_i b_i) in closed form - no eigensolver between the inputs and the expected value."""
    rng = np.random.default_rng([int(seed), int(d), int(round(np.log10(cond)))])
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    a = np.geomspace(1.0, 1.0 / cond, d)
    b = rng.permutation(np.geomspace(2.0, 2.0 / np.sqrt(cond), d))
    cx, cy = _sym((q * a) @ q.T), _sym((q * b) @ q.T)
    mu_x, mu_y = rng.standard_normal(d), rng.standard_normal(d)
    return mu_x, cx, mu_y, cy, float(np.sqrt(a * b).sum())


def sample_pair(d, rows_x, rows_y, seed):
    """(mu_x, cx, mu_y, cy): two independent sample covariances (decaying column scales, the two sets differ in scale and
    offset); rows < d + 1 gives a rank-deficient one."""
    rng = np.random.default_rng([int(seed), int(d), int(rows_x), int(rows_y)])
    scale = 1.0 / np.sqrt(1.0 + np.arange(d))
    x = rng.standard_normal((rows_x, d)) * scale * 1.1 + 0.05
    y = rng.standard_normal((rows_y, d)) * scale
    return (x.mean(0), _sym(np.cov(x, rowvar=False).reshape(d, d)), y.mean(0), _sym(np.cov(y, rowvar=False).reshape(d, d)))


def dyadic_pair(d, seed):
    """(mu_x, mu_y, cy) whose entries are multiples of 2^-10 below 8 in size: every sum the distance takes of them and of
    their squares is exact in f64 in any order, so `exactly` can be asserted of a result that sums them."""
    rng = np.random.default_rng([int(seed), int(d)])
    grid = lambda v: np.round(v * 1024.0) / 1024.0
    mu_x, mu_y = grid(rng.standard_normal(d)), grid(rng.standard_normal(d))
    g = rng.standard_normal((d, 2 * d + 2))
    cy = grid(_sym(g @ g.T / (2 * d + 2)))
    return mu_x, mu_y, cy


# ------------------------------------------------------------------ oracles of the distance
def fd_of(mu_x, cx, mu_y, cy, tr_sqrt):
    return float(((mu_x - mu_y) ** 2).sum() + np.trace(cx) + np.trace(cy) - 2.0 * tr_sqrt)


def fd_closed(mu_x, cx, mu_y, cy, tr_sqrt):
    """The Frechet distance of a commuting_pair from its closed-form trace."""
    return fd_of(mu_x, cx, mu_y, cy, tr_sqrt)


def fd_psd(mx, cx, my, cy):
    """(fd, tr_sqrt) of any pair: tr sqrt(Cx Cy) = sum sqrt(eig(sqrt(Cx) Cy sqrt(Cx))), both steps symmetric
    eigenproblems, negative rounding dust clamped."""
    w, v = np.linalg.eigh(_sym(cx))
    root = (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T
    lam = np.linalg.eigvalsh(_sym(root @ cy @ root))
    tr_sqrt = float(np.sqrt(np.clip(lam, 0.0, None)).sum())
    return fd_of(mx, cx, my, cy, tr_sqrt), tr_sqrt


def solver_scale(cx, cy):
    """tr Cx + tr Cy: the terms the distance is a difference of; every solver bound is relative to it."""
    return float(np.trace(cx) + np.trace(cy))


BATCH_D = [33, 5]
BATCH_RANK_ROWS = {33: 10, 5: 3}


def batch_sets(d, shared):
    """Five sets of one batched call, as (kind, mu_x, cx, mu_y, cy, fd, tr_sqrt) with the oracle's fd and tr_sqrt:
    well-conditioned, rank-deficient, zero, cond 1e8 (closed form) and Cx = Cy (tr sqrt = tr Cy).  shared: every set is scored
    against the reference of the cond-1e8 pair, so one (mu_y, cy) serves all five; otherwise each set brings its own."""
    mu_c, cx_c, my_c, cy_c, tr_c = commuting_pair(d, 1e8, 3)
    sets = []
    for kind in ("well", "rank", "zero", "cond", "same"):
        if kind == "well":
            mu_x, cx, mu_y, cy = sample_pair(d, 4 * d, 4 * d, 11)
        elif kind == "rank":
            mu_x, cx, mu_y, cy = sample_pair(d, BATCH_RANK_ROWS[d], 6 * d, 12)
        elif kind == "zero":
            mu_x, _, mu_y, cy = sample_pair(d, 4 * d, 4 * d, 13)
            cx = np.zeros((d, d))
        elif kind == "cond":
            mu_x, cx, mu_y, cy = mu_c, cx_c, my_c, cy_c
        else:
            mu_x, _, mu_y, cy = sample_pair(d, 4 * d, 5 * d, 14)
            cx = cy
        if shared:
            mu_y, cy = my_c, cy_c
            if kind == "same":
                cx = cy
        if kind == "zero":
            fd, tr = fd_of(mu_x, cx, mu_y, cy, 0.0), 0.0
        elif kind == "cond":
            fd, tr = fd_of(mu_x, cx, mu_y, cy, tr_c), tr_c
        elif kind == "same":
            tr = float(np.trace(cy))
            fd = fd_of(mu_x, cx, mu_y, cy, tr)
        else:
            fd, tr = fd_psd(mu_x, cx, mu_y, cy)
        sets.append((kind, mu_x, cx, mu_y, cy, fd, tr))
    return sets


# ------------------------------------------------------------------ model of the Newton-Schulz solve
def ns_model(cx, cy, max_iter=64, tol=1e-13):
    """(tr_sqrt, iters, stop, resid) of the coupled Newton-Schulz iteration with the stopping rule of frechet.hip's header:
        A = Cx Cy;  Y0 = A / |A|_F,  Z0 = I;   T = (3 I - Z Y) / 2;  Y <- Y T;  Z <- T Z;   tr sqrt(A) = sqrt(|A|_F) tr(Y)
    Every evaluation of the rule looks at r = |I - Z Y|_F and t = tr(Y): a trace that fell (below prev (1 - 1e-14)) or is not
    finite stops with code 2 and keeps the previous trace; otherwise the trace is accepted (iters += 1) and r < tol sqrt(D)
    stops with code 1.  The budget is max_iter updates; one more evaluation follows the last update.  Code 0: budget spent,
    3: zero product, 4: non-finite product (or a first trace that is not finite).  The header gives the rule; the slack
    (1 - 1e-14), the - 1e-300 term and code 4 for a first trace that is not finite follow ns_next_state in ns_engine.h.
    No expected value of a device test comes from here alone: those come from the closed form and from LAPACK."""
    with np.errstate(all="ignore"):
        a = np.asarray(cx, dtype=np.float64) @ np.asarray(cy, dtype=np.float64)
        d = a.shape[0]
        norm = float(np.sqrt((a * a).sum()))
    if not np.isfinite(norm):
        return float("nan"), 0, 4, 0.0
    if norm == 0.0:
        return 0.0, 0, 3, 0.0
    y, z, eye = a / norm, np.eye(d), np.eye(d)
    prev, resid, iters, stop = -np.inf, 0.0, 0, 0
    for it in range(max_iter + 1):
        with np.errstate(all="ignore"):
            zy = z @ y
            r = float(np.sqrt(((eye - zy) ** 2).sum()))
            t = float(np.trace(y))
        if not (np.isfinite(t) and not np.isnan(r)) or t < prev * (1.0 - 1e-14) - 1e-300:
            stop = 4 if np.isinf(prev) else 2
            break
        prev, resid, iters = t, r, iters + 1
        if r < tol * np.sqrt(float(d)):
            stop = 1
            break
        if it == max_iter:
            break
        with np.errstate(all="ignore"):
            tm = 1.5 * eye - 0.5 * zy
            y, z = y @ tm, tm @ z
    return float(prev * np.sqrt(norm)), iters, stop, resid


# ------------------------------------------------------------------ statistics: inputs, oracle, model
def stats_input(n, d, seed=0):
    """f32 rows with a scale in [0.5, 1.5) and an offset N(0, 1) per column."""
    rng = np.random.default_rng([int(seed), int(n), int(d)])
    return (rng.standard_normal((n, d)) * (0.5 + rng.random(d)) + rng.standard_normal(d)).astype(np.float32)


def scatter_f64(x, mean):
    xc = np.asarray(x, dtype=np.float64) - np.asarray(mean, dtype=np.float64)
    return xc.T @ xc


def cov_f64(x):
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    return scatter_f64(x, x.mean(0)) / (n - 1) if n > 1 else np.zeros((d, d))


STATS_CHAIN = 256
STATS_TILE = 128


def stats_f32_model(x, mean=None):
    """The arithmetic stats.hip documents, on f32 rows: column mean in f64 (or the mean given); rows centred in f32 against
    the f32-rounded mean; f32 products summed in f32 over chains of 256 rows; the chains added in f64.  Below one 128-column
    tile the products (exact in f64) are summed in f64 from the first row on.  Returns the unbiased
    covariance (mean=None: the sample's own mean; one row gives zeros) or, for a given mean, the undivided scatter."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    n, d = x.shape
    own = mean is None
    m = x.astype(np.float64).mean(0) if own else np.asarray(mean, dtype=np.float64)
    if own and n == 1:
        return np.zeros((d, d))
    xc = x - m.astype(np.float32)
    assert xc.dtype == np.float32
    if d < STATS_TILE:
        s = xc.astype(np.float64).T @ xc.astype(np.float64)
    else:
        s = np.zeros((d, d))
        for r0 in range(0, n, STATS_CHAIN):
            c = xc[r0:r0 + STATS_CHAIN]
            s += (c.T @ c).astype(np.float64)
    return s / (n - 1) if own else s


def elem_rel(got, want, diag=None):
    """max |got - want|_ij / sqrt(d_i d_j), d the diagonal of `want` (or the one given): an elementwise measure, so one wrong
    strip or mirrored element cannot hide in a norm.  Zero diagonal entries (a constant column) count with their own size."""
    diag = np.diagonal(want) if diag is None else diag
    den = np.sqrt(np.outer(diag, diag))
    err = np.abs(np.asarray(got) - np.asarray(want))
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(den > 0, err / den, np.where(err > 0, np.inf, 0.0))
    return float(rel.max())


def merge_f64(n1, m1, c1, n2, m2, c2):
    """(mean, cov, bound) of the Chan merge in the association order merge_cov_kernel's comment states,
    (w1 c1 + w2 c2) + wd (delta_i delta_j), and the elementwise size of its three terms."""
    n = float(n1 + n2)
    w1, w2, wd = (n1 - 1) / (n - 1), (n2 - 1) / (n - 1), (float(n1) * float(n2) / n) / (n - 1)
    delta = m1 - m2
    outer = np.outer(delta, delta)
    mean = (float(n1) * m1 + float(n2) * m2) / n
    cov = (w1 * c1 + w2 * c2) + wd * outer
    return mean, cov, np.abs(w1 * c1) + np.abs(w2 * c2) + np.abs(wd * outer)
