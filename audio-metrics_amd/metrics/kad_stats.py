"""Error bars for the Kernel Audio Distance: the closed-form large-sample standard error of the unbiased MMD^2 and a
two-model comparison against one reference set, both from the ROW SUMS of the three kernel blocks (ops.mmd_rbf_row_sums:
every Gram tile computed once - the work of kernel_audio_distance itself, no resampling).

  w_i = sum_{j != i} k(x_i, x_j)    c_i = sum_j k(x_i, y_j)    v_j = sum_{l != j} k(y_j, y_l)    r_j = sum_i k(x_i, y_j)
  mmd^2 = sum w / (n (n - 1)) + sum v / (m (m - 1)) - 2 sum c / (n m)

Standard error: the first-order (Hoeffding) term of the two-sample U-statistic, with the influence values
  a_i = w_i / (n - 1) - c_i / m,   b_j = v_j / (m - 1) - r_j / n:      var = 4 s^2(a) / n + 4 s^2(b) / m      (s^2: ddof = 1).
It describes the case users have - two distributions that DIFFER.  Under equality the first-order term vanishes, the true
variance is O(1 / n^2) and this estimate tends to 0: it is NOT a test of mmd^2 = 0.

Two candidates A and B against one reference R (the relative-similarity test of Bounliphone et al., ICLR 2016): both
distances share the reference rows, so they are correlated, and the reference enters through the DIFFERENCE of its cross
means:  diff = mmd^2(A, R) - mmd^2(B, R) (the sum v term cancels),  rho_j = r^B_j / n_b - r^A_j / n_a,
  var = 4 s^2(a) / n_a + 4 s^2(b) / n_b + 4 s^2(rho) / m,     z = diff / sqrt(var),
one-sided p = Phi(z) (small: A is significantly closer to R than B), two-sided p = 2 Phi(-|z|)."""
import math
import statistics
import warnings

import numpy as np
import torch

from .. import hip_ops as ops
from ..data import AudioMetricsData
from .kad import KAD_SCALE, _finish_bandwidth, _gamma_bits, _resolve_bandwidth, _rows_of


def _vec(a, name):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 1:
        raise ValueError(f"{name} must be a vector of row sums, got shape {a.shape}")
    return a


def _sets(n, m, what):
    if n < 2 or m < 2:
        raise ValueError(f"{what} needs at least 2 rows in every set (got {n} and {m}): the unbiased MMD^2 divides by n (n - 1)")


def mmd_standard_error(w, c, v, r):
    """(mmd^2, standard error) of the unbiased MMD^2 from the four row-sum vectors (w, c: one entry per candidate row; v, r:
    one per reference row) - host arithmetic, float64 numpy.  The error is the first-order term for distributions that
    differ; under equality it tends to 0 and is NOT a test of mmd^2 = 0."""
    w, c, v, r = _vec(w, "w"), _vec(c, "c"), _vec(v, "v"), _vec(r, "r")
    n, m = len(w), len(v)
    if len(c) != n or len(r) != m:
        raise ValueError(f"w and c hold one entry per candidate row ({n}, {len(c)}), v and r one per reference row ({m}, {len(r)})")
    _sets(n, m, "mmd_standard_error")
    mmd2 = w.sum() / (n * (n - 1.0)) + v.sum() / (m * (m - 1.0)) - 2.0 * c.sum() / (float(n) * m)
    a = w / (n - 1.0) - c / m
    b = v / (m - 1.0) - r / n
    var = 4.0 * a.var(ddof=1) / n + 4.0 * b.var(ddof=1) / m
    return float(mmd2), float(math.sqrt(var)) if var == var else float("nan")


def _phi(z):
    return 0.5 * math.erfc(-z / math.sqrt(2.0))


def mmd_difference_test(w_a, c_a, r_a, w_b, c_b, r_b):
    """The comparison of two candidate sets against one reference from their row sums (w_a, c_a: one entry per row of A;
    w_b, c_b: per row of B; r_a, r_b: the cross sums of A and of B per REFERENCE row) - host arithmetic, float64 numpy.
    Returns {"difference": mmd^2(A, R) - mmd^2(B, R), "std_error", "z", "p_value": Phi(z) (small: A is closer),
    "p_value_two_sided"}.  The variance treats A and B as independent samples; when they hold the same rows (identical row
    sums throughout) or the variance is 0, z and both p-values are NaN, with ONE RuntimeWarning."""
    w_a, c_a, r_a = _vec(w_a, "w_a"), _vec(c_a, "c_a"), _vec(r_a, "r_a")
    w_b, c_b, r_b = _vec(w_b, "w_b"), _vec(c_b, "c_b"), _vec(r_b, "r_b")
    na, nb, m = len(w_a), len(w_b), len(r_a)
    if len(c_a) != na or len(c_b) != nb or len(r_b) != m:
        raise ValueError(f"row-sum vectors disagree: A {na}/{len(c_a)}, B {nb}/{len(c_b)}, reference {m}/{len(r_b)}")
    _sets(min(na, nb), m, "mmd_difference_test")
    diff = (w_a.sum() / (na * (na - 1.0)) - 2.0 * c_a.sum() / (float(na) * m)) \
        - (w_b.sum() / (nb * (nb - 1.0)) - 2.0 * c_b.sum() / (float(nb) * m))
    a = w_a / (na - 1.0) - c_a / m
    b = w_b / (nb - 1.0) - c_b / m
    rho = r_b / nb - r_a / na
    var = 4.0 * a.var(ddof=1) / na + 4.0 * b.var(ddof=1) / nb + 4.0 * rho.var(ddof=1) / m
    out = {"difference": float(diff), "std_error": float(math.sqrt(var)) if var == var else float("nan")}
    # The three terms are those of INDEPENDENT samples.  Candidates with the same row sums throughout are one sample handed
    # in twice (their term rho vanishes identically, the a and b terms do not): the difference is 0 by construction, not by
    # chance, and no z belongs to it.
    same = na == nb and np.array_equal(w_a, w_b) and np.array_equal(c_a, c_b) and np.array_equal(r_a, r_b)
    if var > 0.0 and not same:
        z = float(diff) / math.sqrt(var)
        out.update(z=z, p_value=_phi(z), p_value_two_sided=2.0 * _phi(-abs(z)))
    else:
        if same or var == 0.0:                              # (else a NaN sum - a non-finite row: NaN throughout, nothing to warn of)
            warnings.warn("mmd_difference_test: the two candidate sets hold the same rows (or the variance estimate is 0): the "
                          "difference has no sampling distribution to test against; z and the p-values are NaN", RuntimeWarning,
                          stacklevel=2)
        out.update(z=float("nan"), p_value=float("nan"), p_value_two_sided=float("nan"))
    return out


def _checked_rows(what, sets):
    """The stored float32 rows of every (data, name), all of one width - checked before any device call."""
    rows = [_rows_of(data, name) for data, name in sets]
    for e, (_, name) in zip(rows, sets):
        if e.dtype == torch.float64:
            raise NotImplementedError(f"{what} takes float32 rows (the {name} set holds float64 rows; the float64 matrix-core form "
                                      "of the row sums is not implemented)")
    for e in rows[:-1]:
        if e.shape[1] != rows[-1].shape[1]:
            raise ValueError(f"feature widths differ: {e.shape[1]} and {rows[-1].shape[1]}")
    return rows


def _row_sums(cache, gamma, bw2_dev, candidates, ey):
    """(per candidate set: out_x [n, 2]; the reference's v [m] and whether it is fresh; per candidate set: r [m]).  v comes
    from the reference-side cache when its gamma is known there; else the first call carries the YY block."""
    width = {"bw2": bw2_dev} if bw2_dev is not None else {"gamma": gamma}
    v = cache.vrow.get(_gamma_bits(gamma)) if gamma is not None else None
    fresh = v is None
    outs, cross = [], []
    for e in candidates:
        blocks = ops.MMD_XX | ops.MMD_XY | (ops.MMD_YY if v is None else 0)
        out_x, out_y = ops.mmd_rbf_row_sums(e, ey, blocks=blocks, **width)
        if v is None:
            v = out_y[:, 0].clone()
        outs.append(out_x)
        cross.append(out_y[:, 1])
    return outs, v, fresh, cross


def _read_back(outs, cross, v, bw2_dev):
    """The one read-back of a call: every out_x, every r, v and the device bandwidth (0 where a number fixed it)."""
    tail = bw2_dev.to(torch.float64).reshape(1) if bw2_dev is not None else torch.zeros(1, dtype=torch.float64, device=v.device)
    flat = torch.cat([o.reshape(-1) for o in outs] + list(cross) + [v, tail]).cpu().numpy()
    pos, xs, rs = 0, [], []
    for o in outs:
        xs.append(flat[pos:pos + o.numel()].reshape(-1, 2))
        pos += o.numel()
    for r in cross:
        rs.append(flat[pos:pos + r.numel()])
        pos += r.numel()
    return xs, rs, flat[pos:pos + v.numel()], float(flat[-1])


def _finish(cache, bw, gamma, bw2_dev, bw2_v, v, fresh):
    """The bandwidth goes into the cache as in kernel_audio_distance; cache.syy is NOT written (the row sums add up in
    another order than am_mmd_rbf_f32, and later kernel_audio_distance calls keep their bits); a fresh v is stored under its
    gamma.  Returns bw."""
    bw = _finish_bandwidth(cache, bw, gamma, bw2_dev, bw2_v, None)
    if fresh:
        cache.vrow[_gamma_bits(0.5 / bw2_v if bw2_dev is not None else gamma)] = v
    return bw


def kernel_audio_distance_with_error(x: AudioMetricsData, y: AudioMetricsData, bandwidth=None, scale=KAD_SCALE, confidence=0.95):
    """KAD of candidate set `x` against reference set `y` with its closed-form standard error, for the Gram work of
    kernel_audio_distance (one library call; with the reference's row sums cached, the XX and XY blocks only).  Returns
    {"kad", "kad_mmd2", "kad_bandwidth", "kad_std_error": scale * se, "kad_ci_low", "kad_ci_high": kad -/+ the normal quantile
    of `confidence` times the error}.  The error is the first-order term for two distributions that differ; under equality
    it tends to 0, so the interval is NOT a test of kad = 0.  The value agrees with kernel_audio_distance up to the
    summation order (row sums, not one sum per workgroup)."""
    confidence = float(confidence)
    if not 0.0 < confidence < 1.0:
        raise ValueError(f"confidence={confidence!r} must lie strictly between 0 and 1")
    ex, ey = _checked_rows("kernel_audio_distance_with_error", ((x, "candidate"), (y, "reference")))
    cache, bw, gamma, bw2_dev = _resolve_bandwidth(bandwidth, y, ey)
    outs, v, fresh, cross = _row_sums(cache, gamma, bw2_dev, [ex], ey)
    (wc,), (r,), v_host, bw2_v = _read_back(outs, cross, v, bw2_dev)
    bw = _finish(cache, bw, gamma, bw2_dev, bw2_v, v, fresh)
    mmd2, se = mmd_standard_error(wc[:, 0], wc[:, 1], v_host, r)
    scale = float(scale)
    half = statistics.NormalDist().inv_cdf(0.5 + 0.5 * confidence) * scale * se
    return {"kad": scale * mmd2, "kad_mmd2": mmd2, "kad_bandwidth": bw, "kad_std_error": scale * se,
            "kad_ci_low": scale * mmd2 - half, "kad_ci_high": scale * mmd2 + half}


def kernel_audio_distance_compare(a: AudioMetricsData, b: AudioMetricsData, y: AudioMetricsData, bandwidth=None, scale=KAD_SCALE):
    """Is candidate set `a` closer to the reference `y` than candidate set `b`?  Both KADs under ONE bandwidth (that of `y`)
    and the test of their difference that accounts for the shared reference rows.  Returns {"kad_a", "kad_b",
    "kad_difference": kad_a - kad_b, "kad_difference_std_error", "kad_z", "kad_p_value": Phi(z) - small means `a` is
    significantly closer than `b` -, "kad_p_value_two_sided", "kad_bandwidth"}.  Two library calls of the XX and XY blocks
    (the first carries YY too unless the reference's row sums are cached).  Identical sets give NaN for z and the p-values
    and one RuntimeWarning."""
    ea, eb, ey = _checked_rows("kernel_audio_distance_compare", ((a, "candidate A"), (b, "candidate B"), (y, "reference")))
    cache, bw, gamma, bw2_dev = _resolve_bandwidth(bandwidth, y, ey)
    outs, v, fresh, cross = _row_sums(cache, gamma, bw2_dev, [ea, eb], ey)
    (wa, wb), (ra, rb), v_host, bw2_v = _read_back(outs, cross, v, bw2_dev)
    bw = _finish(cache, bw, gamma, bw2_dev, bw2_v, v, fresh)
    scale = float(scale)
    m = len(v_host)
    syy = v_host.sum() / (m * (m - 1.0))
    kad = [scale * float(s[:, 0].sum() / (len(s) * (len(s) - 1.0)) + syy - 2.0 * s[:, 1].sum() / (float(len(s)) * m)) for s in (wa, wb)]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        t = mmd_difference_test(wa[:, 0], wa[:, 1], ra, wb[:, 0], wb[:, 1], rb)
    for wrn in caught:                                      # re-issued from here, so it points at the caller
        warnings.warn(str(wrn.message).replace("mmd_difference_test", "kernel_audio_distance_compare"), wrn.category, stacklevel=2)
    return {"kad_a": kad[0], "kad_b": kad[1], "kad_difference": scale * t["difference"],
            "kad_difference_std_error": scale * t["std_error"], "kad_z": t["z"], "kad_p_value": t["p_value"],
            "kad_p_value_two_sided": t["p_value_two_sided"], "kad_bandwidth": bw}
