"""Gaussian-kernel diversity at any number of rows: the random-feature Vendi spectrum (FKEA: Ospanov, Zhang, Jalali, Cao,
Bogdanov, Farnia, NeurIPS 2024), the exact order-2 score (RKE: Jalali, Li, Farnia, NeurIPS 2023) and a two-set novelty
spectrum after the construction of KEN (Zhang, Li, Farnia, ICML 2024).

  W        = rff_frequencies(D, R, seed): numpy.random.default_rng(seed).standard_normal((R, D)) rounded to float32 once - a
             unit-bandwidth draw, independent of the bandwidth, the same on every machine
  z_il     = <w_l, x_i> in f32 on the exact tile engine;  a_il = (double) z_il * inv_bw,  inv_bw = 1 / bw in f64 (from a number,
             or on the device from the float32 device scalar bw^2 of ops.pairwise_select_sq - no host round trip)
  phi_i    = R^(-1/2) [cos a_i1 .. cos a_iR, sin a_i1 .. sin a_iR], cos and sin in f64: <phi_i, phi_j> is an unbiased estimate
             of exp(-|x_i - x_j|^2 / (2 bw^2)) and |phi_i|^2 = 1                                     (ops.rff_features)
  S        = (1 / n) sum_i phi_i phi_i^T, [2R][2R] f64, trace 1; its non-zero eigenvalues are those of Phi Phi^T / n, which
             approximates K / n with a Monte-Carlo error of order 1 / sqrt(R)                         (ops.rff_moment)
  scores     from the eigenvalues as vendi_from_eigenvalues forms them, zero rule WHOLE_SET_ZERO_TOL.  ONLY ORDERS q >= 1: the
             small eigenvalues of the random-feature proxy are Monte-Carlo noise, and below order 1 they dominate
  rke      = n^2 / (n + sum_{i != j} exp(-|x_i - x_j|^2 / bw^2)) = 1 / |K / n|_F^2: order 2 exactly, no features - the square
             of a Gaussian kernel is the Gaussian kernel at twice gamma                               (ops.mmd_rbf_sums)
  novelty    Lambda = S_cand - eta S_ref, the same W and the same bandwidth for both sets.  The solver takes PSD input, so it
             gets Lambda + eta I (PSD because S_ref <= trace(S_ref) I = I) and eta is subtracted from its eigenvalues.
             Eigenvalues > 1e-9 (1 + eta) are the positive ones lam+, s their sum:
             novel_mass = s,  ken = sum lam+ ln(s / lam+),  novel_modes = exp(ken / s);  no positive eigenvalue: all three 0.0.
             This restates the paper's construction as this build defines it; no package was available to compare with.
  modes      for eigenvector v_j (descending eigenvalue) the score of row i is phi_i^T v_j; the sign of v_j is fixed so that
             the scores sum to >= 0; mode_rows[j] holds the stored-row indices of the rows_per_mode largest scores, ties to
             the smallest index.

Rounding.  z carries the float32 dot product's error, (D + 16) 2^-24 |x_i| |w_l|, and a multiplies it by inv_bw: unit-norm
rows at a median bandwidth are harmless, rows far from the origin are not.  The Gaussian kernel is shift-invariant, so
centring such rows first is the caller's remedy."""
import math
import struct
import warnings

import numpy as np
import torch

from .. import hip_ops as ops
from .kad import reference_cache
from .vendi import (WHOLE_SET_ZERO_TOL, _bandwidth_tail, _check_kernel, _check_median_rows, _check_orders, _report_bandwidth,
                    _stored_rows, _width, vendi_from_eigenvalues)

NOVELTY_ZERO_TOL = 1e-9            # times (1 + eta): am_eigh_sym_f64's pinned accuracy is 1e-10 of the largest eigenvalue of Lambda + eta I
MODE_CHUNK_ROWS = 4096             # rows per rff_features call of the mode scores: [2R][4096] doubles = 64 MiB at R = 1024


def rff_frequencies(dim, n_features=1024, seed=0):
    """float32 numpy [n_features, dim]: numpy.random.default_rng(seed).standard_normal((n_features, dim)) rounded to float32
    once.  A unit-bandwidth draw: the bandwidth scales the projections, not the frequencies.  Host only."""
    dim, n_features = int(dim), int(n_features)
    if dim < 1 or n_features < 1:
        raise ValueError(f"rff_frequencies: dim={dim} and n_features={n_features} must be at least 1")
    return np.random.default_rng(seed).standard_normal((n_features, dim)).astype(np.float32)


def novelty_from_eigenvalues(lam, eta):
    """The novelty numbers from the eigenvalues of Lambda = S_cand - eta S_ref - numpy float64, no GPU.  Eigenvalues >
    1e-9 (1 + eta) are the positive ones lam+ (summed in descending order), s their sum: {"novel_mass": s, "ken": sum lam+
    ln(s / lam+), "novel_modes": exp(ken / s), "novel_eigenvalues": lam+ descending}; no positive eigenvalue gives 0.0, 0.0,
    0.0 and an empty array, a non-finite eigenvalue NaN."""
    eta = float(eta)
    if not (eta > 0.0 and math.isfinite(eta)):
        raise ValueError(f"eta={eta!r} must be a finite positive number")
    lam = np.sort(np.asarray(lam, dtype=np.float64).ravel())[::-1]
    if lam.size == 0:
        raise ValueError("no eigenvalues")
    if not np.isfinite(lam).all():
        return {"novel_mass": math.nan, "ken": math.nan, "novel_modes": math.nan, "novel_eigenvalues": np.full(0, np.nan)}
    pos = lam[lam > NOVELTY_ZERO_TOL * (1.0 + eta)].copy()
    if pos.size == 0:
        return {"novel_mass": 0.0, "ken": 0.0, "novel_modes": 0.0, "novel_eigenvalues": pos}
    s = float(np.cumsum(pos)[-1])
    ken = float(np.cumsum(pos * np.log(s / pos))[-1])
    return {"novel_mass": s, "ken": ken, "novel_modes": math.exp(ken / s), "novel_eigenvalues": pos}


# ---------------------------------------------------------------- validation, all of it before any device call
def _whole_number(value, lo, hi):
    """value as an int when it is a whole number in lo .. hi, else None"""
    try:
        ok = not isinstance(value, bool) and int(value) == value and lo <= int(value) <= hi
    except (TypeError, ValueError, OverflowError):
        ok = False
    return int(value) if ok else None


def _check_features(n_features, modes, rows_per_mode):
    cap = ops.rff_max_features()
    r = _whole_number(n_features, 1, cap)
    if r is None:
        raise ValueError(f"n_features={n_features!r} must be an integer in 1 .. {cap} (rff_max_features())")
    j = _whole_number(modes, 0, 2 * r)
    if j is None:
        raise ValueError(f"modes={modes!r} must be an integer in 0 .. 2 n_features = {2 * r}")
    k = _whole_number(rows_per_mode, 1, 1 << 31)
    if k is None:
        raise ValueError(f"rows_per_mode={rows_per_mode!r} must be a positive integer")
    return r, j, k


def _check_rff_orders(orders):
    orders = _check_orders(orders)
    if any(q < 1.0 for q in orders):
        raise ValueError(f"orders={orders!r}: the random-feature spectrum supports orders q >= 1 only (its small eigenvalues are "
                         "Monte-Carlo noise, which dominates below order 1); vendi_score has every order up to 2048 rows")
    return orders


def _float32_rows(x, what, name="its first argument"):
    rows, owner = _stored_rows(x, what)
    if rows.dtype == torch.float64:
        raise NotImplementedError(f"{what}: {name} holds float64 rows; rff_moment takes float32 rows (the float64 matrix-core "
                                  "form is not implemented)")
    return rows, owner


def _rff_width(bw, rows, owner):
    """(the width keywords of ops.rff_features / ops.rff_moment, the state _report_bandwidth needs, the key of the width's
    source for a cache)"""
    _, state = _width("gaussian", bw, rows, owner)
    if bw is not None:
        return {"inv_bw": 1.0 / bw}, state, ("fixed", struct.pack("<d", bw))
    return {"bw2": state[3]}, state, ("median",)


# ---------------------------------------------------------------- mode scores: plumbing on ops.rff_features
def _mode_rows(rows, w, width, vecs, k):
    """(mode_rows int64 [J, k], mode_scores f64 [J, k]) as device tensors: the k rows with the largest phi_i^T v_j for every
    row v_j of vecs [J, 2R], the sign of v_j chosen so that the scores sum to >= 0, ties to the smallest index.  The scores
    are V @ F per row chunk; both signs keep a running list (a stable descending sort of [list so far, chunk] keeps equal
    scores in index order), the sum decides which one is returned."""
    n, dev, j = int(rows.shape[0]), rows.device, int(vecs.shape[0])
    k = min(k, n)
    best = [(torch.empty((j, 0), dtype=torch.float64, device=dev), torch.empty((j, 0), dtype=torch.int64, device=dev)) for _ in range(2)]
    total = torch.zeros(j, dtype=torch.float64, device=dev)
    buf = torch.empty((vecs.shape[1], min(n, MODE_CHUNK_ROWS)), dtype=torch.float64, device=dev)
    for r0 in range(0, n, MODE_CHUNK_ROWS):
        c = min(MODE_CHUNK_ROWS, n - r0)
        f = ops.rff_features(rows, w, row0=r0, nrows=c, out=buf, **width)[:, :c]
        scores = torch.matmul(vecs, f)
        total += scores.sum(dim=1)
        index = torch.arange(r0, r0 + c, dtype=torch.int64, device=dev).expand(j, c)
        for side, sign in ((0, 1.0), (1, -1.0)):
            vals = torch.cat([best[side][0], sign * scores], dim=1)
            idx = torch.cat([best[side][1], index], dim=1)
            vals, order = torch.sort(vals, dim=1, descending=True, stable=True)
            best[side] = (vals[:, :k].contiguous(), torch.gather(idx, 1, order[:, :k]))
    flip = (total < 0.0)[:, None]
    return torch.where(flip, best[1][1], best[0][1]), torch.where(flip, best[1][0], best[0][0])


def _mode_fields(out, lam, modes, mode_rows, mode_scores):
    out["mode_eigenvalues"] = lam[:modes].copy()
    out["mode_rows"] = mode_rows
    out["mode_scores"] = mode_scores


def _nan_modes(modes, k):
    return np.full((modes, k), -1, dtype=np.int64), np.full((modes, k), np.nan)


# ---------------------------------------------------------------- the three scores
def vendi_score_rff(x, orders=(1.0, 2.0, float("inf")), bandwidth=None, n_features=1024, seed=0, return_eigenvalues=False,
                    modes=0, rows_per_mode=8):
    """The Gaussian-kernel Vendi scores of the rows of x (an AudioMetricsData with stored rows, or a float32 device tensor
    [n, D]) at ANY number of rows, from the spectrum of the [2 n_features]^2 random-feature moment matrix S (module
    docstring).  orders: q >= 1 only (float('inf') allowed), q < 1 raises ValueError.  bandwidth=None: the median pairwise
    distance of x's own rows, through the reference-side cache of KAD when x is a set; a number fixes it.  Returns
    {"vendi_rff": the order-1 score, "vendi_rff_per_order": f64 [len(orders)], "vendi_rff_orders", "vendi_rff_rank",
    "vendi_rff_bandwidth", "vendi_rff_features": n_features, "vendi_rff_seed"}, plus "vendi_rff_eigenvalues" (descending, the
    min(n, 2 n_features) leading ones, those the zero rule drops as 0.0) when asked, plus - modes=J > 0 - "mode_eigenvalues"
    [J], "mode_rows" int64 [J, min(rows_per_mode, n)] (stored-row indices) and "mode_scores" (the same shape).  One
    read-back for the scores (eigenvalues and bandwidth in one transfer), one more for the modes.  A row with a NaN or an
    infinity gives NaN scores, rank 0 and one RuntimeWarning naming the count."""
    n_features, modes, rows_per_mode = _check_features(n_features, modes, rows_per_mode)
    orders = _check_rff_orders(orders)
    bw = _check_kernel("gaussian", bandwidth)
    rows, owner = _float32_rows(x, "vendi_score_rff")
    n, d = int(rows.shape[0]), int(rows.shape[1])
    _check_median_rows("gaussian", bw, n)
    freq = rff_frequencies(d, n_features, seed)
    rows = ops.as_matrix(rows)
    width, state, _ = _rff_width(bw, rows, owner)
    w = ops.upload_host_array(freq, rows.device)
    s, check = ops.rff_moment(rows, w, **width)
    bad = check()                                             # in front of the solver, which refuses a non-finite matrix
    size = min(n, 2 * n_features)
    k = min(rows_per_mode, n)
    if bad:
        bw2_v = float(_bandwidth_tail(state, rows.device).cpu()[0])
        bw_out = _report_bandwidth(state, bw2_v)
        warnings.warn(f"vendi_score_rff: {bad} rows hold a NaN or an infinity: the scores are NaN", RuntimeWarning, stacklevel=2)
        per_order, vendi_1, rank, lam = np.full(len(orders), np.nan), float("nan"), 0, np.full(size, np.nan)
        mode_rows, mode_scores = _nan_modes(modes, k)
    else:
        evals, evecs = ops.eigh_descending(s)
        flat = torch.cat([evals, _bandwidth_tail(state, rows.device)]).cpu().numpy()      # the one read-back of the scores
        lam, bw2_v = flat[:size].copy(), float(flat[-1])
        bw_out = _report_bandwidth(state, bw2_v)
        keep = lam > WHOLE_SET_ZERO_TOL * lam[0]
        lam = np.where(keep, lam, 0.0)
        rank = int(keep.sum())
        per_order = vendi_from_eigenvalues(lam, orders, 0.0)
        vendi_1 = float(per_order[orders.index(1.0)]) if 1.0 in orders else float(vendi_from_eigenvalues(lam, (1.0,), 0.0)[0])
        if modes:
            mr, ms = _mode_rows(rows, w, width, evecs[:modes], rows_per_mode)
            mode_rows, mode_scores = mr.cpu().numpy(), ms.cpu().numpy()
    out = {"vendi_rff": vendi_1, "vendi_rff_per_order": per_order, "vendi_rff_orders": orders, "vendi_rff_rank": rank,
           "vendi_rff_bandwidth": bw_out, "vendi_rff_features": n_features, "vendi_rff_seed": seed}
    if return_eigenvalues:
        out["vendi_rff_eigenvalues"] = lam
    if modes:
        full = np.full(modes, np.nan)
        full[:min(modes, size)] = lam[:modes]
        _mode_fields(out, full, modes, mode_rows, mode_scores)
    return out


def rke_score(x, bandwidth=None):
    """The RKE mode count of the rows of x (a set with stored rows or a device tensor [n, D]) under the Gaussian kernel:
    n^2 / (n + sum_{i != j} exp(-|x_i - x_j|^2 / bw^2)) = 1 / |K / n|_F^2, the order-2 Vendi score - exact, at any number of
    rows, no random features: one XX pass of ops.mmd_rbf_sums at twice gamma.  bandwidth=None: the median pairwise distance
    of x's rows (the shared KAD-side cache when x is a set); the float32 device scalar bw^2 is halved on the device, which is
    exact.  Returns {"rke", "rke_bandwidth", "rke_sum": the kernel sum over ordered pairs i != j}."""
    bw = _check_kernel("gaussian", bandwidth)
    rows, owner = _stored_rows(x, "rke_score")
    n = int(rows.shape[0])
    _check_median_rows("gaussian", bw, n)
    rows = ops.as_rows(rows)
    _, state = _width("gaussian", bw, rows, owner)
    if bw is not None:
        sums = ops.mmd_rbf_sums(rows, rows, gamma=1.0 / (bw * bw), blocks=ops.MMD_XX)
    else:
        sums = ops.mmd_rbf_sums(rows, rows, bw2=state[3] * 0.5, blocks=ops.MMD_XX)       # gamma = 0.5 / (bw^2 / 2) = 1 / bw^2
    sxx, bw2_v = torch.cat([sums[:1], _bandwidth_tail(state, rows.device)]).cpu().tolist()      # the one read-back
    bw_out = _report_bandwidth(state, bw2_v)
    return {"rke": float(n) * n / (n + sxx), "rke_bandwidth": bw_out, "rke_sum": sxx}


def kernel_novelty_score(cand, ref, eta=1.0, bandwidth=None, n_features=1024, seed=0, modes=0, rows_per_mode=8):
    """The novelty spectrum of candidate set `cand` against reference set `ref` (sets with stored float32 rows, or float32
    device tensors): the eigen-decomposition of Lambda = S_cand - eta S_ref (module docstring) - which modes the candidate
    produces more often than eta times the reference holds them.  bandwidth=None: the REFERENCE's median pairwise distance,
    as KAD takes it.  The reference's S is kept on the reference set beside the KAD cache under (bandwidth source,
    n_features, seed) and dropped on append; a cached call returns the bits of an uncached one.  Returns {"ken",
    "novel_mass", "novel_modes", "novel_eigenvalues": the positive ones descending, "ken_eta", "ken_bandwidth"} and - modes=J >
    0 - "mode_eigenvalues" [J] (of Lambda, descending, whatever their sign), "mode_rows" int64 [J, min(rows_per_mode, n)]
    and "mode_scores" over the CANDIDATE's rows.  A row with a NaN or an infinity in either set gives NaN and one
    RuntimeWarning naming the count."""
    n_features, modes, rows_per_mode = _check_features(n_features, modes, rows_per_mode)
    eta = float(eta)
    if not (eta > 0.0 and math.isfinite(eta)):
        raise ValueError(f"eta={eta!r} must be a finite positive number")
    bw = _check_kernel("gaussian", bandwidth)
    ex, _ = _float32_rows(cand, "kernel_novelty_score", "the candidate set")
    ey, owner = _float32_rows(ref, "kernel_novelty_score", "the reference set")
    if ex.shape[1] != ey.shape[1]:
        raise ValueError(f"feature widths differ: {ex.shape[1]} and {ey.shape[1]}")
    n, d = int(ex.shape[0]), int(ex.shape[1])
    _check_median_rows("gaussian", bw, int(ey.shape[0]))
    freq = rff_frequencies(d, n_features, seed)
    ex, ey = ops.as_matrix(ex), ops.as_matrix(ey)
    width, state, source = _rff_width(bw, ey, owner)
    w = ops.upload_host_array(freq, ex.device)
    store = reference_cache(owner).rff if owner is not None else None
    key = (source, n_features, seed)
    s_ref = store.get(key) if store is not None else None
    bad = 0
    if s_ref is None:
        s_ref, check_ref = ops.rff_moment(ey, w, **width)
        bad += check_ref()
        if store is not None and not bad:
            store[key] = s_ref
    s_cand, check_cand = ops.rff_moment(ex, w, **width)
    bad += check_cand()                                       # in front of the solver, which refuses a non-finite matrix
    size = 2 * n_features
    k = min(rows_per_mode, n)
    if bad:
        bw2_v = float(_bandwidth_tail(state, ex.device).cpu()[0])
        bw_out = _report_bandwidth(state, bw2_v)
        warnings.warn(f"kernel_novelty_score: {bad} rows hold a NaN or an infinity: the scores are NaN", RuntimeWarning, stacklevel=2)
        out = novelty_from_eigenvalues(np.full(1, np.nan), eta)
        lam = np.full(size, np.nan)
        mode_rows, mode_scores = _nan_modes(modes, k)
    else:
        shifted = s_cand - eta * s_ref
        shifted.diagonal().add_(eta)                           # Lambda + eta I: PSD, what the solver takes
        evals, evecs = ops.eigh_descending(shifted)
        flat = torch.cat([evals, _bandwidth_tail(state, ex.device)]).cpu().numpy()          # the one read-back of the scores
        lam, bw2_v = flat[:size] - eta, float(flat[-1])
        bw_out = _report_bandwidth(state, bw2_v)
        out = novelty_from_eigenvalues(lam, eta)
        if modes:
            mr, ms = _mode_rows(ex, w, width, evecs[:modes], rows_per_mode)
            mode_rows, mode_scores = mr.cpu().numpy(), ms.cpu().numpy()
    out.update(ken_eta=eta, ken_bandwidth=bw_out)
    if modes:
        _mode_fields(out, lam, modes, mode_rows, mode_scores)
    return out
