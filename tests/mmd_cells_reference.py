"""Unit-pair kernel sums and the permutation statistic, host only: the float64 oracle of am_mmd_rbf_cells_f32 in the arithmetic
the library documents (include/audio_metrics_hip.h),

  d2(a, b) = max((|a|^2 + |b|^2) - 2 a.b, 0),  K = exp(-d2 gamma),
  a set is a list of positions (an index outside [0, N) is an empty position: it contributes to no sum),
  cell a = positions [32 a, 32 a + 32),  value of (a, b) = sum of K over the position pairs, p != q inside one set,
  unit = a run of cells,

and the permutation statistic of metrics/kad_perm.py by direct relabel-and-recompute from the full Gram matrix.

Used by tests/test_gpu_mmd_cells.py and tests/test_gpu_kad_perm.py (the kernels and the front end against the oracle) and
tests/test_mmd_perm_cpu.py (the host logic, and the oracle itself)."""
import numpy as np

import kad_reference as ka

CELL = 32
BLOCK = 2048          # rows of a block per step of the Gram


def position_gram(x, idx_x, y, idx_y, gamma, dots=None):
    """K over the POSITIONS of the two lists, float64 [n_pos_x, n_pos_y]: 0 wherever a position is empty (idx None: the rows
    in stored order).  `dots(a, b)`: an emulated f32 dot-product matrix."""
    x, y = np.asarray(x), np.asarray(y)

    def side(a, idx):
        idx = np.arange(len(a)) if idx is None else np.asarray(idx, dtype=np.int64)
        live = (idx >= 0) & (idx < len(a))
        return idx, live
    ix, lx = side(x, idx_x)
    iy, ly = side(y, idx_y)
    rx, ry = x[ix[lx]], y[iy[ly]]
    k = np.zeros((len(rx), len(ry)))
    with np.errstate(over="ignore", invalid="ignore"):
        for lo in range(0, len(rx), BLOCK):
            k[lo:lo + BLOCK] = np.exp(-ka.d2_matrix(rx[lo:lo + BLOCK], ry, dots) * gamma)
    out = np.zeros((len(ix), len(iy)))
    out[np.ix_(np.flatnonzero(lx), np.flatnonzero(ly))] = k
    return out


def _live(a, idx):
    """the number of positions of a list that name a row"""
    if idx is None:
        return len(a)
    idx = np.asarray(idx, dtype=np.int64)
    return int(((idx >= 0) & (idx < len(a))).sum())


def fold(k, rows, cols):
    """sums of k over the blocks cut at the offsets `rows` x `cols`"""
    return np.add.reduceat(np.add.reduceat(k, rows[:-1], axis=0), cols[:-1], axis=1)


def cell_offsets(n_pos):
    c = -(-n_pos // CELL)
    return np.minimum(np.arange(c + 1) * CELL, n_pos)


def unit_offsets(n_pos, units):
    """position offsets of the units (cell offsets `units`, or None: unit = cell)"""
    cells = cell_offsets(n_pos)
    return cells if units is None else cells[np.asarray(units, dtype=np.int64)]


def unit_sums(x, y, gamma, idx_x=None, idx_y=None, units_x=None, units_y=None, dots=None, same=False):
    """dict "xx" [U1, U1], "yy" [U2, U2], "xy" [U1, U2] and "scale" = mean |K| over the three blocks' live pairs (the unit of
    the exact-data tolerance).  The diagonal of the within blocks is dropped by POSITION, whatever its value.  same=True: y
    (and its list) IS x."""
    def within(a, idx, units):
        k = position_gram(a, idx, a, idx, gamma, dots)
        total = np.nansum(np.abs(k))
        np.fill_diagonal(k, 0.0)
        offs = unit_offsets(k.shape[0], units)
        live = _live(a, idx)
        return fold(k, offs, offs), total / max(float(live) * live, 1.0)
    xx, abs_xx = within(x, idx_x, units_x)
    yy, abs_yy = (xx.copy(), abs_xx) if same else within(y, idx_y, units_y)
    k = position_gram(x, idx_x, y, idx_y, gamma, dots)
    xy = fold(k, unit_offsets(k.shape[0], units_x), unit_offsets(k.shape[1], units_y))
    live = float(_live(x, idx_x)) * _live(y, idx_y)
    return dict(xx=xx, yy=yy, xy=xy, scale=float(np.mean([abs_xx, abs_yy, np.nansum(np.abs(k)) / max(live, 1.0)])))


def pooled(s):
    """the pooled [U, U] matrix of a dict of unit sums, X's units first"""
    return np.block([[s["xx"], s["xy"]], [s["xy"].T, s["yy"]]])


# ---------------------------------------------------------------------------------------------------- the permutation statistic
def relabelled_mmd2(K, unit_of_row, x_units):
    """The unbiased MMD^2 when the rows of the units `x_units` are X and all others Y, straight from the pooled Gram matrix K
    (its diagonal is never read); NaN when a side has fewer than 2 rows."""
    in_x = np.isin(unit_of_row, x_units)
    ix, iy = np.flatnonzero(in_x), np.flatnonzero(~in_x)
    n, m = len(ix), len(iy)
    if n < 2 or m < 2:
        return float("nan")
    kxx, kyy, kxy = K[np.ix_(ix, ix)], K[np.ix_(iy, iy)], K[np.ix_(ix, iy)]
    return float((kxx.sum() - np.trace(kxx)) / (n * (n - 1.0)) + (kyy.sum() - np.trace(kyy)) / (m * (m - 1.0))
                 - 2.0 * kxy.sum() / (float(n) * m))


def labellings(U, n_x_units, n_permutations, seed):
    """the unit sets metrics/kad_perm.py draws: per permutation the first n_x_units entries of one rng.permutation(U)"""
    rng = np.random.default_rng(seed)
    return [rng.permutation(U)[:n_x_units] for _ in range(n_permutations)]


def permutation_null(K, unit_of_row, n_x_units, n_permutations, seed):
    """(T_obs, null [P], p) by relabel-and-recompute"""
    U = int(np.max(unit_of_row)) + 1
    t_obs = relabelled_mmd2(K, unit_of_row, np.arange(n_x_units))
    null = np.array([relabelled_mmd2(K, unit_of_row, s) for s in labellings(U, n_x_units, n_permutations, seed)])
    return t_obs, null, (1.0 + np.count_nonzero(~(null < t_obs))) / (1.0 + n_permutations)


def pooled_gram(x, y, gamma):
    z = np.concatenate([np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)])
    return np.exp(-ka.d2_matrix(z, z) * gamma)


def run_units(n, unit_rows, first=0):
    """unit of every row when a set of n rows is cut into runs of unit_rows (numbered from `first`)"""
    return first + np.arange(n) // unit_rows
