"""Statistical dependence between two PAIRED embedding sets: does row i of one set depend on row i of the other?

Distance covariance / correlation (Szekely, Rizzo, Bakirov 2007; the unbiased form and its t-test: Szekely & Rizzo 2013,
2014) and its kernel twin HSIC (Gretton et al. 2005; unbiased: Song et al. 2012) with the normalised form CKA (Kornblith et
al. 2019, here debiased).  Both are one formula on two pair matrices a_ij (from the x rows) and b_ij (from the y rows), i != j:

  A_i = sum_j a_ij,  B_i = sum_j b_ij,  H_i = sum_j a_ij b_ij,  AA_i = sum_j a_ij^2,  BB_i = sum_j b_ij^2      (ops.pair_dependence)
  T_a = sum A_i,  T_b = sum B_i,  S_ab = sum H_i,  C_ab = sum A_i B_i
  U(a, b) = [S_ab - 2 C_ab / (n - 2) + T_a T_b / ((n - 1)(n - 2))] / (n (n - 3))

with a = |x_i - x_j| this is the unbiased dCov^2, with a = k(x_i, x_j) the unbiased HSIC; U(a, a) uses sum AA_i and sum A_i^2.
The row sums come from ONE sweep that forms both Gram tiles of a pair block in one workgroup (csrc/pair_dependence.hip); no
N x N matrix exists.  Everything after the sweep is host arithmetic in numpy float64.

A model that ignores its context scores 0 (up to the estimator's noise, which may be negative); a reference set of real
(context, stem) pairs gives the ceiling to compare with.  These are dependence measures, not distances between sets.

The t-test of the distance correlation assumes INDEPENDENT pairs.  Windows of one track are not independent: on such data
quote the permutation null with `groups` (one label per pair: the song), which re-pairs whole songs."""
import math
import warnings

import numpy as np
import torch

from .. import hip_ops as ops
from ._groups import _group_labels
from .kad import reference_cache
from .kad_stats import _phi

MIN_ROWS = ops.PAIR_DEPENDENCE_MIN_ROWS
NORMAL_TAIL_DOF = 1e6              # above this many degrees of freedom Student's t is the normal distribution to double precision


# ------------------------------------------------------------------------------------------------ host arithmetic
def _u(s, c, ta, tb, n):
    return (s - 2.0 * c / (n - 2.0) + ta * tb / ((n - 1.0) * (n - 2.0))) / (n * (n - 3.0))


def _v(s, c, ta, tb, n):
    return s / n ** 2 - 2.0 * c / n ** 3 + ta * tb / n ** 4


def dependence_from_sums(rows_or_sums, n):
    """The U- and V-statistics from the row sums - host arithmetic, float64, no GPU.  `rows_or_sums`: the [n, 5] row sums
    {A_i, B_i, H_i, AA_i, BB_i} of ops.pair_dependence, or a vector {T_a, T_b, S_ab, S_aa, S_bb, C_ab[, C_aa, C_bb]} of their
    totals (C_ab = sum A_i B_i, C_aa = sum A_i^2, C_bb = sum B_i^2; without the last two the variances are NaN).  Returns
    {"u_ab", "u_aa", "u_bb"}: U(a, b) = [S_ab - 2 C_ab / (n - 2) + T_a T_b / ((n - 1)(n - 2))] / (n (n - 3)), the unbiased
    dCov^2 / HSIC and the two variances, and {"v_ab", "v_aa", "v_bb"}: the V-statistics S / n^2 - 2 C / n^3 + T_a T_b / n^4."""
    n = int(n)
    if n < MIN_ROWS:
        raise ValueError(f"n={n}: the unbiased statistics need at least {MIN_ROWS} paired rows (they divide by n - 3)")
    a = np.asarray(rows_or_sums, dtype=np.float64)
    if a.ndim == 2:
        if a.shape != (n, 5):
            raise ValueError(f"row sums must have shape ({n}, 5), got {a.shape}")
        A, B = a[:, 0], a[:, 1]
        ta, tb, sab, saa, sbb = (float(a[:, j].sum()) for j in range(5))
        cab, caa, cbb = float(A @ B), float(A @ A), float(B @ B)
    elif a.ndim == 1 and a.shape[0] in (6, 8):
        ta, tb, sab, saa, sbb, cab = (float(v) for v in a[:6])
        caa, cbb = (float(a[6]), float(a[7])) if a.shape[0] == 8 else (float("nan"), float("nan"))
    else:
        raise ValueError(f"expected the [n, 5] row sums or a vector of 6 or 8 totals, got shape {a.shape}")
    n = float(n)
    return {"u_ab": _u(sab, cab, ta, tb, n), "u_aa": _u(saa, caa, ta, ta, n), "u_bb": _u(sbb, cbb, tb, tb, n),
            "v_ab": _v(sab, cab, ta, tb, n), "v_aa": _v(saa, caa, ta, ta, n), "v_bb": _v(sbb, cbb, tb, tb, n)}


def row_dependence(rows):
    """Each pair's share of U(a, b) from the [n, 5] row sums, in stored order:
    [H_i - 2 A_i B_i / (n - 2) + (A_i T_b + B_i T_a) / (2 (n - 1)(n - 2))] / (n - 3).  Its mean is the statistic."""
    a = np.asarray(rows, dtype=np.float64)
    n = float(a.shape[0])
    A, B, H = a[:, 0], a[:, 1], a[:, 2]
    return (H - 2.0 * A * B / (n - 2.0) + (A * B.sum() + B * A.sum()) / (2.0 * (n - 1.0) * (n - 2.0))) / (n - 3.0)


def _ratio(u_ab, u_aa, u_bb):
    """u_ab / sqrt(u_aa u_bb), or None where a variance is not positive"""
    if not (u_aa > 0.0 and u_bb > 0.0):
        return None
    return u_ab / math.sqrt(u_aa * u_bb)


def dcor_t_test(dcor, n):
    """(t, degrees of freedom, one-sided p) of the bias-corrected distance correlation under independence of n INDEPENDENT
    pairs (Szekely & Rizzo 2013): t = sqrt(v - 1) dcor / sqrt(1 - dcor^2), v = n (n - 3) / 2, Student's t with v - 1 degrees
    of freedom; a small p says dependent.  Above 1e6 degrees of freedom the normal tail."""
    v = n * (n - 3.0) / 2.0
    dof = v - 1.0
    if not (abs(dcor) < 1.0) or dof <= 0.0:
        t = math.copysign(float("inf"), dcor) if abs(dcor) >= 1.0 and dof > 0.0 else float("nan")
        p = float("nan") if math.isnan(t) else (0.0 if t > 0 else 1.0)
        return t, dof, p
    t = math.sqrt(dof) * dcor / math.sqrt(1.0 - dcor * dcor)
    if dof > NORMAL_TAIL_DOF:
        return t, dof, _phi(-t)
    from scipy import stats                                  # only this branch needs it
    return t, dof, float(stats.t.sf(t, dof))


def dependence_permutations(n, groups=None, n_permutations=0, seed=0):
    """The re-pairings of the permutation null: (perms int64 [P, n], units_movable, units_fixed); pair i keeps its x row and
    takes the y row perms[p, i].  Labellings come from numpy.random.default_rng(seed) on the host.  Without `groups` rows are
    permuted freely (one rng.permutation(n) per labelling; every row is a movable unit).  With `groups` (one integer label
    per pair: the song) whole songs exchange their y blocks inside classes of equal row count, the window order kept: per
    labelling, for the classes of at least two songs in ascending row count, one rng.permutation(number of songs); song j of
    the class (ascending label) takes the block of song sigma[j].  A song alone in its class stays fixed."""
    n, P = int(n), int(n_permutations)
    rng = np.random.default_rng(seed)
    if groups is None:
        perms = np.stack([rng.permutation(n) for _ in range(P)]).astype(np.int64) if P else np.zeros((0, n), dtype=np.int64)
        return perms, n, 0
    labels = np.asarray(groups).astype(np.int64)
    order = np.argsort(labels, kind="stable")
    uniq, starts, counts = np.unique(labels[order], return_index=True, return_counts=True)
    classes, fixed = [], 0
    for size in np.unique(counts):
        songs = np.nonzero(counts == size)[0]
        if len(songs) < 2:
            fixed += 1
            continue
        classes.append(np.stack([order[starts[s]:starts[s] + size] for s in songs]))       # [songs, windows] stored rows
    movable = int(sum(len(c) for c in classes))
    perms = np.tile(np.arange(n, dtype=np.int64), (P, 1))
    for p in range(P):
        for block in classes:
            sigma = rng.permutation(len(block))
            perms[p, block.reshape(-1)] = block[sigma].reshape(-1)
    return perms, movable, fixed


# ------------------------------------------------------------------------------------------------ front ends
def _rows(data, name, what):
    rows = data if torch.is_tensor(data) else getattr(data, "embeddings", None)
    if rows is None:
        raise ValueError(f"{what} needs the stored rows of {name}, which keeps none "
                         f"(store_embeddings={getattr(data, 'store_embeddings', None)})")
    if rows.dim() != 2:
        raise ValueError(f"{name} must hold 2-D rows, got shape {tuple(rows.shape)}")
    if rows.dtype == torch.float64:
        raise NotImplementedError(f"{what} takes float32 rows ({name} holds float64 rows; the float64 matrix-core form is not "
                                  "implemented)")
    return rows


def _open(x, y, groups, n_permutations, what):
    """The checks both front ends open with; no device call."""
    ex, ey = _rows(x, "x", what), _rows(y, "y", what)
    n = int(ex.shape[0])
    if int(ey.shape[0]) != n:
        raise ValueError(f"{what}: the sets are paired row by row, but x holds {n} rows and y {int(ey.shape[0])}")
    if n < MIN_ROWS:
        raise ValueError(f"{what}: {n} paired rows; the unbiased statistics need at least {MIN_ROWS} (they divide by n - 3)")
    if ex.device != ey.device:
        raise ValueError(f"{what}: x and y are on different devices ({ex.device} and {ey.device})")
    P = int(n_permutations)
    if P < 0:
        raise ValueError(f"n_permutations={n_permutations!r} must be at least 0")
    labels = None
    if groups is not None:
        labels = _group_labels(groups)
        if labels.numel() != n:
            raise ValueError(f"groups holds {labels.numel()} labels for {n} pairs (one label per pair)")
        labels = labels.cpu().numpy()
    return ex, ey, n, P, labels


def _permutation_null(ex, ey, kind, widths, host_rows, labels, P, seed, u_obs, prefix, what):
    """{prefix_p_value_permutation, prefix_null_mean / _std / _q95, prefix_n_permutations, units_movable, units_fixed}: a
    re-pairing changes S_ab alone on the device (one sweep with `perm` each) and C_ab by a host dot product of the observed
    row sums; T_a, T_b and both variances stay."""
    n = host_rows.shape[0]
    perms, movable, fixed = dependence_permutations(n, labels, P, seed)
    out = {prefix + "_n_permutations": P, "units_movable": movable, "units_fixed": fixed}
    nan = float("nan")
    if movable < 2:
        warnings.warn(f"{what}: fewer than two movable units ({movable}; {fixed} songs are alone in their row-count class): no "
                      "re-pairing exists, the permutation p-value is NaN", RuntimeWarning, stacklevel=3)
        out.update({prefix + "_p_value_permutation": nan, prefix + "_null_mean": nan, prefix + "_null_std": nan,
                    prefix + "_null_q95": nan})
        return out, None
    s_ab = torch.empty(P, dtype=torch.float64, device=ex.device)
    for p in range(P):
        perm = ops.upload_host_array(perms[p], ex.device)
        s_ab[p] = ops.pair_dependence(ex, ey, kind, perm=perm, **widths)[1][2]
    s_ab = s_ab.cpu().numpy()                                # the one read-back of the null
    A, B = host_rows[:, 0], host_rows[:, 1]
    c_ab = B[perms] @ A                                      # C_ab(pi) = sum_i A_i B_pi(i)
    null = _u(s_ab, c_ab, float(A.sum()), float(B.sum()), float(n))
    exceed = int(np.count_nonzero(~(null < u_obs)))          # NaN counts as exceeding
    out.update({prefix + "_p_value_permutation": (1.0 + exceed) / (1.0 + P), prefix + "_null_mean": float(null.mean()),
                prefix + "_null_std": float(null.std(ddof=1)) if P > 1 else nan, prefix + "_null_q95": float(np.quantile(null, 0.95))})
    return out, null


def _nonfinite_warning(what, count, n):
    warnings.warn(f"{what}: {count} of {n} pairs hold a row with non-finite elements (NaN / inf embeddings); every figure is NaN",
                  RuntimeWarning, stacklevel=3)


def distance_correlation(x, y, groups=None, n_permutations=0, seed=0, return_rows=False):
    """Distance covariance and correlation of two paired sets (AudioMetricsData with stored rows, or 2-D float32 device
    tensors): row i of x belongs to row i of y; the widths may differ.  Returns
      dcov2, dvar_x, dvar_y   the unbiased U(a, b), U(a, a), U(b, b) with a_ij = |x_i - x_j|, b_ij = |y_i - y_j|
      dcor                    dcov2 / sqrt(dvar_x dvar_y): bias-corrected, on the scale of the SQUARED correlation; about 0
                              under independence and then slightly negative half of the time
      dcor_v                  the classical V-statistic V(a, b) / sqrt(V(a, a) V(b, b)) in [0, 1] on the same scale
      dcor_t, dcor_dof, dcor_p_value    the t-test of independence (dcor_t_test; one-sided, small: dependent).  It assumes
                              INDEPENDENT pairs: windows of one track are not, and then the permutation null below with
                              `groups` is the test to quote
      dcor_rows, dcor_rows_nonfinite    the number of pairs, and of pairs with a non-finite row (then every figure is NaN and
                              one RuntimeWarning names the count)
    return_rows adds "row_dependence" (row_dependence(): each pair's share, its mean is dcov2) and "row_sums" [n, 5].
    n_permutations > 0 adds the permutation null of dcov2 (dcor_p_value_permutation = (1 + #{U_p >= U_obs}) / (1 + P),
    dcor_null_mean / _std / _q95, units_movable, units_fixed; one sweep per labelling): with `groups` (one integer label per
    pair: the song) whole songs exchange their y blocks inside classes of equal row count, else rows are permuted freely
    (dependence_permutations).  A variance <= 0 or the same object passed twice gives NaN for dcor and its test, and one
    RuntimeWarning."""
    what = "distance_correlation"
    ex, ey, n, P, labels = _open(x, y, groups, n_permutations, what)
    rows_dev, sums_dev = ops.pair_dependence(ex, ey, "energy")
    host = torch.cat([rows_dev.reshape(-1), sums_dev]).cpu().numpy()          # the one read-back of the observed sums
    host_rows, sums = host[:5 * n].reshape(n, 5), host[5 * n:]
    bad = int(sums[7])
    nan = float("nan")
    out = {}
    if bad:
        _nonfinite_warning(what, bad, n)
        out = {k: nan for k in ("dcov2", "dvar_x", "dvar_y", "dcor", "dcor_v", "dcor_t")}
        out.update({"dcor_dof": n * (n - 3.0) / 2.0 - 1.0, "dcor_p_value": nan})
    else:
        st = dependence_from_sums(host_rows, n)
        same = x is y
        dcor = None if same else _ratio(st["u_ab"], st["u_aa"], st["u_bb"])
        if dcor is None:
            warnings.warn(f"{what}: " + ("the same object was passed twice" if same else
                                         f"a distance variance is not positive (dvar_x={st['u_aa']!r}, dvar_y={st['u_bb']!r})") +
                          "; dcor and its test are NaN", RuntimeWarning, stacklevel=2)
            dcor_v, (t, dof, pv) = nan, (nan, n * (n - 3.0) / 2.0 - 1.0, nan)
            dcor = nan
        else:
            vr = _ratio(st["v_ab"], st["v_aa"], st["v_bb"])
            dcor_v = nan if vr is None else vr
            t, dof, pv = dcor_t_test(dcor, n)
        out = {"dcov2": st["u_ab"], "dvar_x": st["u_aa"], "dvar_y": st["u_bb"], "dcor": dcor, "dcor_v": dcor_v, "dcor_t": t,
               "dcor_dof": dof, "dcor_p_value": pv}
    out.update({"dcor_rows": n, "dcor_rows_nonfinite": bad})
    if P > 0:
        if bad:
            out.update({"dcor_p_value_permutation": nan, "dcor_null_mean": nan, "dcor_null_std": nan, "dcor_null_q95": nan,
                        "dcor_n_permutations": P})
        else:
            null_out, _ = _permutation_null(ex, ey, "energy", {}, host_rows, labels, P, seed, out["dcov2"], "dcor", what)
            out.update(null_out)
    if return_rows:
        out["row_dependence"] = np.full(n, nan) if bad else row_dependence(host_rows)
        out["row_sums"] = host_rows.copy()
    return out


def _bandwidth(bandwidth, data, rows, name):
    """(the bw2 argument of ops.pair_dependence, the device scalar or None): a number fixes the width; None takes the
    set's own median pairwise distance as a device scalar, through the select and - on an AudioMetricsData - the cache
    kernel_audio_distance uses; no host round trip."""
    if bandwidth is not None:
        bw = float(bandwidth)
        if not math.isfinite(bw) or bw <= 0.0:
            raise ValueError(f"{name}={bandwidth!r} must be a finite positive number")
        return bw * bw, None
    if torch.is_tensor(data):
        dev = ops.pairwise_select_sq(rows)
    else:
        cache = reference_cache(data)
        if cache.bw2 is None:
            cache.bw2 = ops.pairwise_select_sq(rows)
        dev = cache.bw2
    return dev, dev


def kernel_alignment(x, y, kernel="gaussian", bandwidth_x=None, bandwidth_y=None, groups=None, n_permutations=0, seed=0,
                     return_rows=False):
    """HSIC and the debiased centred kernel alignment of two paired sets, with the keywords of distance_correlation.
    `kernel`: "gaussian" exp(-d2 / (2 bw^2)) or "laplacian" exp(-d / bw), one bandwidth per side: a number, or None for the
    set's own median pairwise distance (a device scalar from the select kernel_audio_distance uses; never read back before
    the sweep).  Returns hsic, hsic_xx, hsic_yy (the unbiased U(a, b), U(a, a), U(b, b) of Song et al. 2012),
    cka = hsic / sqrt(hsic_xx hsic_yy), hsic_bandwidth_x, hsic_bandwidth_y, hsic_kernel, hsic_rows, hsic_rows_nonfinite; the
    permutation null under the prefix hsic_ and the rows as distance_correlation does."""
    what = "kernel_alignment"
    if kernel not in ("gaussian", "laplacian"):
        raise ValueError(f"kernel={kernel!r} is not one of ['gaussian', 'laplacian']")
    ex, ey, n, P, labels = _open(x, y, groups, n_permutations, what)
    (bwx, devx), (bwy, devy) = _bandwidth(bandwidth_x, x, ex, "bandwidth_x"), _bandwidth(bandwidth_y, y, ey, "bandwidth_y")
    widths = {"bw2x": bwx, "bw2y": bwy}
    rows_dev, sums_dev = ops.pair_dependence(ex, ey, kernel, **widths)
    tail = [d.to(torch.float64).reshape(1) if d is not None else torch.zeros(1, dtype=torch.float64, device=ex.device) for d in (devx, devy)]
    host = torch.cat([rows_dev.reshape(-1), sums_dev, *tail]).cpu().numpy()       # the one read-back of the observed sums
    host_rows, sums = host[:5 * n].reshape(n, 5), host[5 * n:5 * n + 8]
    bw2 = [float(host[5 * n + 8 + j]) if d is not None else float(w) for j, (d, w) in enumerate(((devx, bwx), (devy, bwy)))]
    bad = int(sums[7])
    nan = float("nan")
    for v, name in zip(bw2, ("x", "y")):
        if not bad and not (math.isfinite(v) and v > 0.0):
            raise ValueError(f"{what}: the median pairwise distance of {name} is {v!r} - more than half of its row pairs coincide "
                             f"(duplicate rows); pass bandwidth_{name}= to fix the kernel width")
    if bad:
        _nonfinite_warning(what, bad, n)
        out = {"hsic": nan, "hsic_xx": nan, "hsic_yy": nan, "cka": nan}
    else:
        st = dependence_from_sums(host_rows, n)
        same = x is y
        cka = None if same else _ratio(st["u_ab"], st["u_aa"], st["u_bb"])
        if cka is None:
            warnings.warn(f"{what}: " + ("the same object was passed twice" if same else
                                         f"a kernel variance is not positive (hsic_xx={st['u_aa']!r}, hsic_yy={st['u_bb']!r})") +
                          "; cka is NaN", RuntimeWarning, stacklevel=2)
            cka = nan
        out = {"hsic": st["u_ab"], "hsic_xx": st["u_aa"], "hsic_yy": st["u_bb"], "cka": cka}
    out.update({"hsic_bandwidth_x": math.sqrt(bw2[0]) if bw2[0] > 0 else nan, "hsic_bandwidth_y": math.sqrt(bw2[1]) if bw2[1] > 0 else nan,
                "hsic_kernel": kernel, "hsic_rows": n, "hsic_rows_nonfinite": bad})
    if P > 0:
        if bad:
            out.update({"hsic_p_value_permutation": nan, "hsic_null_mean": nan, "hsic_null_std": nan, "hsic_null_q95": nan,
                        "hsic_n_permutations": P})
        else:
            null_out, _ = _permutation_null(ex, ey, kernel, widths, host_rows, labels, P, seed, out["hsic"], "hsic", what)
            out.update(null_out)
    if return_rows:
        out["row_dependence"] = np.full(n, nan) if bad else row_dependence(host_rows)
        out["row_sums"] = host_rows.copy()
    return out
