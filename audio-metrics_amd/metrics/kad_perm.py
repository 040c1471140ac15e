"""A permutation test for the Kernel Audio Distance: can the candidate set still be told apart from the reference set?

The closed-form standard error of metrics/kad_stats.py is NOT a test of kad = 0 (its first-order term vanishes under
equality).  The standard answer is a permutation test of the unbiased MMD^2: pool the two sets, relabel, recompute, and see
where the observed value falls.  Recomputing costs a Gram pass per relabelling; regrouping does not:

  cut the pooled rows [X; Y] into exchangeable UNITS;  G[a][b] = sum_{i in a, j in b, i != j} k(z_i, z_j)
  for a 0/1 labelling l of the units (1 = X), n = l.sizes, m = N - n:
    XX = l'Gl,   XY = l'G1 - XX,   YY = 1'G1 - 2 l'G1 + XX,   T = XX / (n (n - 1)) + YY / (m (m - 1)) - 2 XY / (n m)

ops.mmd_rbf_cell_sums yields G in ONE Gram sweep (the work of kernel_audio_distance itself), and P relabellings are one
[P, U] x [U, U] float64 matmul.

The unit must be what is exchangeable under the null hypothesis.  Embedding pipelines slice every file into windows, so
stored rows come in runs of near-duplicates per track, and a test that permutes ROWS is invalid on such data: on two sets
of 16 and 14 songs of 16 windows drawn from ONE distribution it rejected at the 5 % level in 100 % of 300 draws, where
permuting songs rejected in 6.3 %.  Pass one label per row (x_groups / y_groups: the song) whenever rows are not independent.

The bandwidth.  A number makes the test exact.  bandwidth=None takes the median pairwise distance of the reference set, as
kernel_audio_distance does; that choice looks at the labels (it is not invariant under relabelling), so the test is then
exact only up to the choice of the kernel width."""
import math
import warnings

import numpy as np
import torch

from .. import hip_ops as ops
from ..data import AudioMetricsData
from ._groups import labelled_rows, sort_into_groups
from .kad import KAD_SCALE, _finish_bandwidth, _gamma_bits, _resolve_bandwidth, _rows_of

CELL = ops.MMD_CELL
MAX_DEFAULT_UNITS = 8192          # the pooled unit count unit_rows=None keeps to: G is at most 8192 x 8192 doubles


def mmd_permutation_null(G, sizes, n_x_units, n_permutations=999, seed=0):
    """(T_obs, null, p) of the unbiased MMD^2 under relabellings of units - host logic and one matmul, no library call.
    G: the pooled [U, U] matrix of unit-pair kernel sums (self pairs excluded), X's units first - a torch tensor on any
    device or a numpy array, worked on in float64 where it lives.  sizes: the number of real rows of every unit.  The
    labellings come from rng = numpy.random.default_rng(seed): for each permutation the first n_x_units entries of one
    rng.permutation(U) are X - drawn on the host, so every device sees the same labellings.  The observed statistic is the
    same formula at the identity labelling (the first n_x_units units), in the same matmul.  null: float64 numpy [P];
    p = (1 + #{T_p >= T_obs}) / (1 + P).  A draw that leaves a side fewer than 2 rows has no statistic: its null entry is NaN
    and it counts as exceeding."""
    on_device = isinstance(G, torch.Tensor)
    if not on_device:
        G = torch.as_tensor(np.asarray(G, dtype=np.float64))
    G = G.to(torch.float64)
    if G.dim() != 2 or G.shape[0] != G.shape[1]:
        raise ValueError(f"G must be a square matrix of unit-pair sums, got shape {tuple(G.shape)}")
    U = int(G.shape[0])
    sizes = np.asarray(sizes, dtype=np.float64)
    if sizes.shape != (U,) or not (sizes >= 1).all():
        raise ValueError(f"sizes must hold one positive row count per unit ({U}), got shape {sizes.shape}")
    n_x_units, P = int(n_x_units), int(n_permutations)
    if not 1 <= n_x_units < U:
        raise ValueError(f"n_x_units={n_x_units} must leave both sides at least one of the {U} units")
    if P < 1:
        raise ValueError(f"n_permutations={n_permutations} must be at least 1")
    rng = np.random.default_rng(seed)
    L = np.zeros((P + 1, U), dtype=np.float64)
    L[0, :n_x_units] = 1.0
    for p in range(1, P + 1):
        L[p, rng.permutation(U)[:n_x_units]] = 1.0
    Lt = torch.as_tensor(L).to(G.device)
    LG = Lt @ G                                              # every statistic of the call comes from this one product
    xx = (LG * Lt).sum(1)
    lg1 = LG.sum(1)
    xy = lg1 - xx
    yy = G.sum() - 2.0 * lg1 + xx
    n = Lt @ torch.as_tensor(sizes).to(G.device)
    m = float(sizes.sum()) - n
    ok = (n >= 2) & (m >= 2)
    one = torch.ones_like(n)
    nn, mm = torch.where(ok, n, 2.0 * one), torch.where(ok, m, 2.0 * one)
    T = xx / (nn * (nn - 1.0)) + yy / (mm * (mm - 1.0)) - 2.0 * xy / (nn * mm)
    T = torch.where(ok, T, float("nan") * one).cpu().numpy()
    t_obs, null = float(T[0]), T[1:].copy()
    exceed = int(np.count_nonzero(~(null < t_obs)))        # NaN (no statistic) counts as exceeding
    return t_obs, null, (1.0 + exceed) / (1.0 + P)


def _default_unit_rows(n, m):
    k = 1
    while -(-n // (CELL * k)) - (-m // (CELL * k)) > MAX_DEFAULT_UNITS:
        k += 1
    return CELL * k


def _run_units(n, unit_rows):
    """Consecutive runs of unit_rows stored rows: (index list None, cell offsets or None, rows per unit)"""
    u = -(-n // unit_rows)
    sizes = np.full(u, unit_rows, dtype=np.int64)
    sizes[-1] = n - (u - 1) * unit_rows
    if unit_rows == CELL:
        return None, None, sizes
    cells, per = -(-n // CELL), unit_rows // CELL
    return None, [min(i * per, cells) for i in range(u + 1)], sizes


def _label_units(labels, device):
    """One unit per label: (positions - the stored rows unit by unit, every unit padded to whole cells with -1 -, cell
    offsets, rows per unit)"""
    order, counts, _, sizes = sort_into_groups(labels.to(device, torch.int64))
    cells = -(-sizes // CELL)
    offs = np.concatenate([[0], np.cumsum(cells)])
    starts = torch.as_tensor(np.concatenate([[0], np.cumsum(sizes)[:-1]])).to(device)
    padded = torch.as_tensor(offs[:-1] * CELL).to(device)
    unit = torch.repeat_interleave(torch.arange(len(sizes), device=device), counts)
    dest = torch.arange(order.numel(), device=device) - starts[unit] + padded[unit]
    idx = torch.full((int(offs[-1]) * CELL,), -1, dtype=torch.int64, device=device)
    idx[dest] = order
    return idx, offs.tolist(), sizes


def kernel_audio_distance_permutation_test(x: AudioMetricsData, y: AudioMetricsData, x_groups=None, y_groups=None, unit_rows=None,
                                           n_permutations=999, seed=0, bandwidth=None, scale=KAD_SCALE, return_null=False):
    """Permutation test of KAD(x, y) = 0: the p-value of the observed unbiased MMD^2 among `n_permutations` relabellings of
    exchangeable units of the pooled rows, for the Gram work of kernel_audio_distance itself (one library call; a small p
    says the candidate set can still be told apart from the reference).

    Units.  x_groups / y_groups: one integer label per stored row (the song a window comes from) - one unit per label; the
    two sides are independent.  Without labels a side is cut into consecutive runs of `unit_rows` stored rows (a multiple of
    32; None: the smallest multiple of 32 that keeps the pooled unit count <= 8192, i.e. 32 up to 262 144 pooled rows; the
    last unit of a set may be short).  Rows of one track are near-duplicates and are NOT exchangeable: permuting rows of
    windowed audio rejects equal distributions every time, so give labels whenever rows are not independent.

    Bandwidth: as kernel_audio_distance (the reference-side cache is shared).  bandwidth=None takes the reference's median
    distance, which is not invariant under relabelling: the test is then exact only up to that choice.  A number makes it
    exact.

    Returns {"kad", "kad_mmd2", "kad_bandwidth", "kad_p_value" = (1 + #{T_p >= T_obs}) / (1 + P), "kad_null_mean",
    "kad_null_std", "kad_null_q95" (scaled like kad), "kad_units": (U_x, U_y), "kad_n_permutations"} and, with return_null,
    "kad_null": the P unscaled MMD^2 values.  kad_mmd2 agrees with kernel_audio_distance up to the summation order.  With
    default units on the reference side its unit-pair matrix is cached on the reference set: a second candidate set costs
    the XX and XY blocks only.  float32 rows only."""
    what = "kernel_audio_distance_permutation_test"
    sides = []
    for data, groups, name in ((x, x_groups, "candidate"), (y, y_groups, "reference")):
        if groups is None:
            rows, labels = _rows_of(data, name), None
        else:
            rows, _, labels = labelled_rows(data, groups, what, f"its {name} set")
        if rows.dtype == torch.float64:
            raise NotImplementedError(f"{what} takes float32 rows (the {name} set holds float64 rows; the float64 matrix-core form "
                                      "of the unit-pair sums is not implemented)")
        sides.append((rows, labels, name))
    (ex, lx, _), (ey, ly, _) = sides
    if ex.shape[1] != ey.shape[1]:
        raise ValueError(f"feature widths differ: {ex.shape[1]} and {ey.shape[1]}")
    n, m = int(ex.shape[0]), int(ey.shape[0])
    P = int(n_permutations)
    if P < 1:
        raise ValueError(f"n_permutations={n_permutations!r} must be at least 1")
    if unit_rows is None:
        unit_rows = _default_unit_rows(n if lx is None else 0, m if ly is None else 0)
    else:
        if int(unit_rows) != unit_rows or unit_rows < CELL or unit_rows % CELL:
            raise ValueError(f"unit_rows={unit_rows!r} must be a positive multiple of {CELL} (the kernel sums are kept per cell of "
                             f"{CELL} rows)")
        unit_rows = int(unit_rows)
    for rows, labels, name in sides:
        if labels is None and -(-int(rows.shape[0]) // unit_rows) < 2:
            raise ValueError(f"{what}: the {name} set has fewer than 2 units ({rows.shape[0]} rows in runs of {unit_rows}); a "
                             "relabelling needs at least 2 units on every side")
    units = []
    for rows, labels, name in sides:
        idx, offs, sizes = _run_units(int(rows.shape[0]), unit_rows) if labels is None else _label_units(labels, rows.device)
        if len(sizes) < 2:
            raise ValueError(f"{what}: the {name} set has fewer than 2 units (its labels name {len(sizes)}); a relabelling needs "
                             "at least 2 units on every side")
        units.append((idx, offs, sizes))
    (idx_x, offs_x, sizes_x), (idx_y, offs_y, sizes_y) = units
    ux, uy = len(sizes_x), len(sizes_y)
    if math.comb(ux + uy, ux) < P:
        warnings.warn(f"{what}: {ux} + {uy} units have only {math.comb(ux + uy, ux)} distinct relabellings, fewer than the {P} "
                      "permutations asked for: the resolution of the p-value is limited by the units, not by n_permutations",
                      RuntimeWarning, stacklevel=2)
    cache, bw, gamma, bw2_dev = _resolve_bandwidth(bandwidth, y, ey)
    width = {"bw2": bw2_dev} if bw2_dev is not None else {"gamma": gamma}
    cacheable = ly is None                                   # default units: the YY matrix depends on (gamma, unit_rows) alone
    yy = cache.cells.get((_gamma_bits(gamma), unit_rows)) if cacheable and gamma is not None else None
    fresh = yy is None
    blocks = ops.MMD_XX | ops.MMD_XY | (ops.MMD_YY if fresh else 0)
    xx, new_yy, xy = ops.mmd_rbf_cell_sums(ex, ey, idx_x=idx_x, idx_y=idx_y, units_x=offs_x, units_y=offs_y, blocks=blocks, **width)
    if fresh:
        yy = new_yy
    G = torch.cat([torch.cat([xx, xy], 1), torch.cat([xy.t(), yy], 1)], 0)
    t_obs, null, p = mmd_permutation_null(G, np.concatenate([sizes_x, sizes_y]), ux, P, seed)
    bw2_v = float(bw2_dev.to(torch.float64).item()) if bw2_dev is not None else 0.0
    bw = _finish_bandwidth(cache, bw, gamma, bw2_dev, bw2_v, None)      # cache.syy and cache.vrow are left alone
    if fresh and cacheable:
        cache.cells[(_gamma_bits(0.5 / bw2_v if bw2_dev is not None else gamma), unit_rows)] = yy
    scale = float(scale)
    have = null[~np.isnan(null)]
    stats = (have.mean(), have.std(ddof=1) if len(have) > 1 else float("nan"), np.quantile(have, 0.95)) if len(have) else (float("nan"),) * 3
    out = {"kad": scale * t_obs, "kad_mmd2": t_obs, "kad_bandwidth": bw, "kad_p_value": p, "kad_null_mean": scale * float(stats[0]),
           "kad_null_std": scale * float(stats[1]), "kad_null_q95": scale * float(stats[2]), "kad_units": (ux, uy),
           "kad_n_permutations": P}
    if return_null:
        out["kad_null"] = null
    return out
