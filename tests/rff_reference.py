"""numpy float64 oracles of the random-feature Gaussian Vendi score, the exact RKE score and the novelty spectrum
(audio_metrics_amd.metrics.fkea), from the same float32 rows and the same float32 frequencies the device takes, and the error
bounds the GPU tests hold the device to.  Nothing here comes from the code under test.

  frequencies    numpy.random.default_rng(seed).standard_normal((R, D)) rounded to float32 once
  features       F[l][i] = cos(a) / sqrt(R), F[R + l][i] = sin(a) / sqrt(R),  a = <w_l, x_i> inv_bw, every step in f64
  moment         S = F F^T / n;  its non-zero eigenvalues are those of F^T F / n, which is what eigenvalues() decomposes when
                 n < 2R
  bounds         feature_bound: the float32 dot product of the tile engine is within (D + 16) 2^-24 |x_i| |w_l| of the exact
                 one (the projection bound of tests/test_gpu_swd.py), |d cos|, |d sin| <= |dz| inv_bw, and 2^-50 covers the
                 rounding of a, the evaluation of cos / sin and the scaling (a handful of 2^-53 each).
                 row_delta: |d phi_i| over all 2R entries.  A pair (cos a, sin a) moves by at most |da| along the circle, so
                 the R pairs together move by at most sqrt(R) R^(-1/2) max_l |da_l|: the bound of test 1 at the row's largest
                 |w_l|, times sqrt(R).  (The 2^-50 part has slack for the two entries of a pair.)
                 eigenvalue_bound: phi phi^T moves by at most 2 delta + delta^2 in norm, S with it (a mean), every eigenvalue
                 by Weyl's inequality; + 1e-10 for the solver (am_eigh_sym_f64's pinned accuracy relative to lambda_0 <= 1).
                 log_score_bound: what that does to ln of a score, per order (below)."""
import math

import numpy as np

import vendi_reference as vr

ZERO_TOL = 1e-10                    # the whole-set zero rule (metrics/vendi.py: WHOLE_SET_ZERO_TOL)
NOVELTY_ZERO_TOL = 1e-9             # times (1 + eta)


def frequencies(d, n_features, seed):
    return np.random.default_rng(seed).standard_normal((n_features, d)).astype(np.float32)


def arguments(x, w, inv_bw):
    return (np.asarray(w, dtype=np.float64) @ np.asarray(x, dtype=np.float64).T) * float(inv_bw)


def features(x, w, inv_bw):
    """f64 [2R, n], feature-major"""
    a = arguments(x, w, inv_bw)
    return np.concatenate([np.cos(a), np.sin(a)]) / math.sqrt(len(w))


def moment(x, w, inv_bw):
    f = features(x, w, inv_bw)
    return (f @ f.T) / f.shape[1]


def eigenvalues(x, w, inv_bw):
    """the min(n, 2R) leading eigenvalues of S, descending (the others are zero)"""
    f = features(x, w, inv_bw)
    n = f.shape[1]
    g = (f.T @ f) / n if n < f.shape[0] else (f @ f.T) / n
    return np.linalg.eigvalsh(0.5 * (g + g.T))[::-1].copy()


def apply_zero_rule(lam):
    lam = np.sort(np.asarray(lam, dtype=np.float64))[::-1]
    return lam[lam > ZERO_TOL * lam[0]]


def scores(lam, orders):
    kept = apply_zero_rule(lam)
    return np.array([vr.score(kept, q) for q in orders])


# ---------------------------------------------------------------- bounds
def _norms(a):
    a = np.asarray(a, dtype=np.float64)
    return np.sqrt((a * a).sum(axis=1))


def feature_bound(x, w, inv_bw):
    """[R, n]: the bound on |F - oracle| of the cos row and of the sin row of frequency l at row i"""
    d = np.asarray(x).shape[1]
    return ((d + 16) * 2.0 ** -24 * np.outer(_norms(w), _norms(x)) * float(inv_bw) + 2.0 ** -50) / math.sqrt(len(w))


def row_delta(x, w, inv_bw):
    """the largest |d phi_i| over the rows"""
    d = np.asarray(x).shape[1]
    return float(((d + 16) * 2.0 ** -24 * _norms(x) * _norms(w).max() * float(inv_bw) + 2.0 ** -50).max())


def eigenvalue_bound(x, w, inv_bw):
    delta = row_delta(x, w, inv_bw)
    return 2.0 * delta + delta * delta + 1e-10


def _eta(t):
    return -t * math.log(t) if t > 0.0 else 0.0


def log_score_bound(lam, eps, q):
    """|ln VS_q(device) - ln VS_q(oracle)| when every one of the m eigenvalues `lam` of the oracle (all of them, the tiny ones
    too) is met within eps, and either side may have turned an eigenvalue <= 1e-10 lambda_0 into 0 - so an eigenvalue moves by
    at most e = eps + 1e-10 lambda_0.
      q = 1    ln VS = -sum l ln l.  One term moves by at most min(eta(e), e sup |ln t + 1| over [l - e, l + e]) with eta(t) =
               -t ln t: the first is the modulus of continuity of eta on [0, 1] (|eta(a) - eta(b)| <= eta(|a - b|) for |a - b|
               <= 1 / 2, the step behind Fannes' inequality), the second the mean value theorem where l > e.
      q = inf  ln VS = -ln l_0:  -ln(1 - e / l_0).
      q > 1    ln VS = ln(sum l^q) / (1 - q):  the sum moves by at most sum ((l + e)^q - l^q) = r sum l^q, so ln VS by at most
               -ln(1 - r) / (q - 1)   (-ln(1 - r) >= ln(1 + r) covers both directions); inf when r >= 1."""
    lam = np.sort(np.asarray(lam, dtype=np.float64))[::-1]
    lam = np.maximum(lam, 0.0)
    e = float(eps) + ZERO_TOL * float(lam[0])
    assert e < 0.5
    if q == 1.0:
        total = 0.0
        for l in lam:
            term = _eta(e)
            if l > e:
                sup = max(abs(math.log(l - e) + 1.0), abs(math.log(l + e) + 1.0))
                term = min(term, e * sup)
            total += term
        return total
    if math.isinf(q):
        return -math.log(1.0 - e / float(lam[0])) if e < lam[0] else math.inf
    r = float(np.sum((lam + e) ** q - lam ** q) / np.sum(lam ** q))
    return -math.log(1.0 - r) / (q - 1.0) if r < 1.0 else math.inf


# ---------------------------------------------------------------- the exact routes
def rke_exact(x, bandwidth):
    """n^2 / (n + sum_{i != j} exp(-|x_i - x_j|^2 / bw^2)) and the sum, f64"""
    x = np.asarray(x, dtype=np.float64)
    g = x @ x.T
    sq = np.diag(g)
    d2 = np.maximum((sq[:, None] + sq[None, :]) - 2.0 * g, 0.0)
    k = np.exp(-d2 / float(bandwidth) ** 2)
    s = float(k.sum() - np.trace(k))
    n = len(x)
    return n * n / (n + s), s


def exact_eigenvalues(x, bandwidth):
    """the eigenvalues of the exact K / n, descending"""
    return vr.eigenvalues(x, "gaussian", bandwidth)


def median_bandwidth(x):
    """sqrt of the float32 rounding of the lower median of the f64 squared distances of the unordered pairs (what KAD takes)"""
    x = np.asarray(x, dtype=np.float64)
    g = x @ x.T
    sq = np.diag(g)
    d2 = np.maximum((sq[:, None] + sq[None, :]) - 2.0 * g, 0.0)[np.triu_indices(len(x), 1)]
    d2 = np.sort(d2)
    return math.sqrt(float(np.float32(d2[(len(d2) - 1) // 2])))


# ---------------------------------------------------------------- novelty
def novelty_numbers(lam, eta):
    lam = np.sort(np.asarray(lam, dtype=np.float64))[::-1]
    pos = lam[lam > NOVELTY_ZERO_TOL * (1.0 + eta)]
    if pos.size == 0:
        return {"novel_mass": 0.0, "ken": 0.0, "novel_modes": 0.0, "novel_eigenvalues": pos}
    s = float(pos.sum())
    ken = float(np.sum(pos * np.log(s / pos)))
    return {"novel_mass": s, "ken": ken, "novel_modes": math.exp(ken / s), "novel_eigenvalues": pos}


def novelty(cand, ref, w, inv_bw, eta):
    """(eigenvalues of S_cand - eta S_ref descending, eigenvectors as rows in that order, the candidate's features)"""
    fc = features(cand, w, inv_bw)
    lam, vec = np.linalg.eigh((fc @ fc.T) / fc.shape[1] - eta * moment(ref, w, inv_bw))
    return lam[::-1].copy(), vec.T[::-1].copy(), fc


def mode_rows(f, v, k):
    """(the k rows with the largest f_i^T v after the sign of v is fixed so that the scores sum to >= 0 - ties to the smallest
    index -, their scores)"""
    s = v @ f
    if s.sum() < 0.0:
        s = -s
    order = np.argsort(-s, kind="stable")[:k]
    return order, s[order]


# ---------------------------------------------------------------- the row sets of the tests
def cluster_set(n=1200, d=32, centres=10, spread=0.3, seed=2024):
    """n float32 rows: `centres` N(0, I) centres, a uniformly drawn one per row, plus spread N(0, I)"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centres, d))
    lab = rng.integers(0, centres, n)
    return (c[lab] + spread * rng.standard_normal((n, d))).astype(np.float32)


def planted_sets(d=32, spread=0.3, seed=77):
    """(reference 900 rows from clusters 0..3, candidate 700 rows from clusters 0..4 with their labels, a second candidate of
    700 rows from clusters 0..3): six N(0, I_d) centres"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((6, d))

    def draw(n, k):
        lab = np.arange(n) % k
        rng.shuffle(lab)
        return (c[lab] + spread * rng.standard_normal((n, d))).astype(np.float32), lab
    ref, _ = draw(900, 4)
    cand, lab = draw(700, 5)
    same, _ = draw(700, 4)
    return ref, cand, lab, same
