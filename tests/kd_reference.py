"""Kernel-distance test support, host only: a float64 oracle of the per-subset unbiased MMD^2, data on which every
device dot product is exact, and a CPU emulation of the device arithmetic that prices the rounding tests.

Used by tests/test_gpu_kd.py (the kernels against the oracle) and tests/test_kd_numerics_cpu.py (that the data is exact
and that the rounding tolerances still tell a correct split-f16 form from a plain f16 one)."""
import numpy as np

from oracle.kd import mmd2_unbiased

# ---------------------------------------------------------------------------------------------------- exact data


def exact_rows(rng, n, d, emin=-8, emax=8):
    """float32 rows of integers in [-3, 3] times a per-row power of two 2^e, e in [emin, emax].  A dot product of two rows
    is 2^(e1 + e2) times an integer of magnitude <= 9 d < 2^24 (d <= 9000): exact in float32 whatever the order of the
    additions, exact in the hi plane of the split-f16 form (the lo plane is 0), and the RBF norms and squared distances
    are exact in float64."""
    ints = rng.integers(-3, 4, size=(n, d)).astype(np.float64)
    e = rng.integers(emin, emax + 1, size=(n, 1)).astype(np.float64)
    return (ints * np.exp2(e)).astype(np.float32)


def rbf_rows(rng, n, d, sigma):
    """exact_rows scaled (by powers of two) so that squared distances are of the order of 2 sigma^2: RBF values spread
    over (0, 1) instead of all underflowing to 0 or all rounding to 1."""
    c = int(np.round(np.log2(sigma / (2.0 * np.sqrt(d)))))
    return exact_rows(rng, n, d, c - 1, c + 1)


def index_tables(rng, n1, n2, S, m):
    """int64 [S, m] tables (idx1 into set 1, idx2 into set 2), no repeats inside a subset.  Every subset holds the first and
    the last row of each set at random positions (m == 1: the first and last rows alternate between subsets)."""
    def one(n):
        t = np.empty((S, m), dtype=np.int64)
        for s in range(S):
            if m == 1:
                t[s, 0] = 0 if s % 2 == 0 else n - 1
                continue
            rest = rng.choice(n - 2, m - 2, replace=False) + 1 if m > 2 else np.empty(0, np.int64)
            row = np.concatenate([[0, n - 1], rest]).astype(np.int64)
            t[s] = row[rng.permutation(m)]
        return t
    return one(n1), one(n2)


# ---------------------------------------------------------------------------------------------------- float64 oracle


class Kernel:
    """Polynomial (x y^T gamma + coef0)^degree (reference kd.py:112-116) or RBF exp(-|x - y|^2 / (2 sigma^2))
    (kd.py:86-109) in float64, fed with float64 rows (oracle) or with emulated dot products (rounding tests)."""

    def __init__(self, kind, gamma=None, coef0=1.0, degree=3, sigma=10.0):
        self.kind, self.gamma, self.coef0, self.degree, self.sigma = kind, gamma, coef0, degree, sigma

    def __call__(self, a, b):
        return self.from_dots(a @ b.T, a, b)

    def from_dots(self, d, a, b):
        if self.kind == "rbf":
            d2 = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * d
            return np.exp(-np.maximum(d2, 0.0) * (1.0 / (2.0 * self.sigma * self.sigma)))
        gamma = 1.0 / a.shape[1] if self.gamma is None else self.gamma
        return (d * gamma + self.coef0) ** self.degree


def subset_values(x, y, idx1, idx2, kernel, dots=None):
    """Per subset: (unbiased MMD^2, mean |K| over the three m x m blocks), every step in float64 on float64 copies of the
    gathered rows.  `dots(a, b)`: an emulated f32 dot-product matrix to feed the kernel instead (rounding tests); the
    kernel then gets the float64 rows only for the RBF norms."""
    vals, scale = [], []
    for s in range(idx1.shape[0]):
        a = np.asarray(x[idx1[s]], dtype=np.float64)
        b = np.asarray(y[idx2[s]], dtype=np.float64)
        with np.errstate(over="ignore", invalid="ignore"):                  # non-finite rows: non-finite values
            blocks = [kernel(p, q) if dots is None else kernel.from_dots(dots(p, q), p, q) for p, q in ((a, a), (a, b), (b, b))]
        with np.errstate(divide="ignore", invalid="ignore"):                # m == 1: the reference's 0 / 0
            vals.append(float(mmd2_unbiased(blocks[0], blocks[1], blocks[2])))
        scale.append(float(np.mean([np.abs(k).mean() for k in blocks])))
    return np.array(vals), np.array(scale)


# ---------------------------------------------------------------------------------------------------- device emulation


def half_scale_exp(maxabs):
    """pairwise_common.h half_scale_exp: 13 - floor(log2(max |x|)), clamped to [-60, 60]; 0 for an all-zero row."""
    _, e = np.frexp(maxabs.astype(np.float32))
    ex = 13 - (e.astype(np.int64) - 1)
    return np.where(maxabs == 0, 0, np.clip(ex, -60, 60))


def split_planes(a):
    """kd_split_gather_kernel: each row scaled by its own power of two (largest |element| in [2^13, 2^14)), hi = rn16(t),
    lo = rn16(t - hi); returns (hi, lo, unscale) as float64."""
    a = np.asarray(a, dtype=np.float32)
    ex = half_scale_exp(np.abs(a).max(axis=1))
    t = (a * np.exp2(ex)[:, None].astype(np.float32)).astype(np.float32)
    hi = t.astype(np.float16)
    lo = (t - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64), np.exp2(-ex).astype(np.float64)


def _accumulate(pairs, d, width):
    """f32 accumulator; per `width`-element slab and per (p, q) stage one exact partial dot product and one f32 rounding."""
    acc = None
    for k0 in range(0, d, width):
        sl = slice(k0, k0 + width)
        for p, q in pairs:
            part = p[:, sl] @ q[:, sl].T
            acc = part.astype(np.float32) if acc is None else (acc.astype(np.float64) + part).astype(np.float32)
    return acc


def emulated_dots(form):
    """dots(a, b) of a device form, from float32 rows:
       "split"    split-f16 form: <hi, hi'> + <lo, hi'> + <hi, lo'> per 64-element slab into an f32 accumulator
       "hi_only"  the same with the lo plane dropped, i.e. plain f16 operands (what the tolerances must exclude)
       "f32"      f32 tile form: f32 accumulation per 32-element slab"""
    def dots(a, b):
        d = a.shape[1]
        if form == "f32":
            return _accumulate([(a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64))], d, 32
                               ).astype(np.float64)
        ha, la, ua = split_planes(a)
        hb, lb, ub = split_planes(b)
        stages = [(ha, hb)] if form == "hi_only" else [(ha, hb), (la, hb), (ha, lb)]
        acc = _accumulate(stages, d, 64)
        scale = (ua[:, None] * ub[None, :]).astype(np.float32)               # exact powers of two
        return (acc * scale).astype(np.float64)
    return dots


# Rounding tests (real-valued data, m = 1000): (name, inputs.pair kind, seed, D, form the shape takes, kernel).
ROUNDING_M, ROUNDING_S, ROUNDING_ROWS = 1000, 4, 2000
ROUNDING_CASES = [
    ("unit_128", "unit", 601, 128, "split", Kernel("poly", 1.0 / 128)),
    ("randn_200", "randn", 602, 200, "split", Kernel("poly", 1.0 / 200)),
    ("unit_512", "unit", 603, 512, "split", Kernel("poly", 1.0 / 512)),
    ("shifted_512_c0", "shifted", 604, 512, "split", Kernel("poly", 2.0 / 512, coef0=0.25)),
    ("shifted_1024", "shifted", 605, 1024, "split", Kernel("poly", 1.0 / 1024)),
    ("randn_64", "randn", 606, 64, "f32", Kernel("poly", 1.0 / 64)),
    ("shifted_100", "shifted", 607, 100, "f32", Kernel("poly", 1.0 / 100)),
    ("unit_512_rbf", "unit", 608, 512, "f32", Kernel("rbf", sigma=0.5)),
]
# the limit is MARGIN times the largest emulated error over the subsets of a case: room for the matrix cores' own
# accumulation order, which the emulation does not model (one rounding per slab and stage instead of one per instruction)
MARGIN = 16.0


def rounding_case(name):
    """(x, y, idx1, idx2, form, kernel) of a committed rounding case."""
    import inputs
    _, kind, seed, d, form, kernel = next(c for c in ROUNDING_CASES if c[0] == name)
    x, y = inputs.pair(kind, seed, ROUNDING_ROWS, ROUNDING_ROWS, d)
    i1, i2 = index_tables(np.random.default_rng(seed), ROUNDING_ROWS, ROUNDING_ROWS, ROUNDING_S, ROUNDING_M)
    return x, y, i1, i2, form, kernel


def emulated_errors(x, y, idx1, idx2, form, kernel, want=None):
    """|emulated - float64| per subset (want: the float64 values, if already computed)."""
    if want is None:
        want, _ = subset_values(x, y, idx1, idx2, kernel)
    got, _ = subset_values(x, y, idx1, idx2, kernel, dots=emulated_dots(form))
    return np.abs(got - want)


def rounding_tolerance(errors):
    return MARGIN * float(np.max(errors))
