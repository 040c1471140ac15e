"""Float64 oracle of the classifier-output scores (audio_metrics_amd/metrics/classifier.py, csrc/class_scores.hip): numpy, no
GPU and nothing of the package.  exp and log run in numpy.longdouble (wider than double on x86-64; the code also works where
it is not), and every sum is math.fsum over the terms split into a double head and a double tail, so a sum adds no error
of its own (the column marginals of a group excepted, see class_groups).  Next to each value the functions return the magnitude the tests' error bounds are stated in."""
import math
import os

import numpy as np

ACCURACY_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "class_scores", "accuracy.txt")
LD = np.longdouble
MODES = ("cosine", "kl_softmax", "kl_sigmoid", "kl_bernoulli")


def row_is_finite(l):
    l = np.asarray(l, dtype=np.float64)
    return not (np.isnan(l).any() or (l == np.inf).any() or (l == -np.inf).all())


def row_quantities(l):
    """(h, p, scale) of one row of logits: h = sum p log p, p the posterior as longdouble, scale = sum p |l - M| + |log S| + 1
    (what the bound of h is stated in).  A non-finite row gives (NaN, None, NaN)."""
    l = np.asarray(l, dtype=np.float64)
    if not row_is_finite(l):
        return math.nan, None, math.nan
    d = (l - l.max()).astype(LD)                             # exact in double: computed as the kernel does, then widened
    live = d != -np.inf
    e = np.where(live, np.exp(d), LD(0))
    s = _ld_sum(e)                                           # (as a longdouble: a double S would add 2^-53 of its own)
    u = _ld_sum(np.where(live, e * np.where(live, d, LD(0)), LD(0)))
    log_s = np.log(s)
    h = u / s - log_s
    p = e / s
    scale = float(_ld_sum(np.where(live, p * np.abs(np.where(live, d, LD(0))), LD(0))) + abs(log_s) + 1)
    return float(h), p, scale


def _ld_sum(terms):
    """The sum of finite longdouble terms as a longdouble: the exactly rounded double sum plus the exactly rounded sum of
    what that leaves."""
    t = np.asarray(terms, dtype=LD).ravel()
    head = t.astype(np.float64)
    tail = (t - head.astype(LD)).astype(np.float64)
    both = np.concatenate([head, tail]).tolist()
    first = math.fsum(both)
    rest = math.fsum(both + [-first])
    return LD(first) + LD(rest)


def class_groups(logits, groups):
    """Per group (a sequence of row-index sequences): dict of arrays mean_h, marginal, log_is, nonfinite, plus h (one list
    per group, NaN for a non-finite row) and the two bound magnitudes: row_scale (per row, as row_quantities) and
    marginal_scale = sum pbar |log pbar| + 1 per group."""
    logits = np.asarray(logits, dtype=np.float64)
    out = {k: [] for k in ("mean_h", "marginal", "log_is", "nonfinite", "h", "row_scale", "marginal_scale")}
    for rows in groups:
        hs, scales, ps, bad = [], [], [], 0
        for i in rows:
            h, p, scale = row_quantities(logits[int(i)])
            hs.append(h)
            scales.append(scale)
            if p is None:
                bad += 1
            else:
                ps.append(p)
        out["h"].append(np.array(hs))
        out["row_scale"].append(np.array(scales))
        out["nonfinite"].append(bad)
        if bad:
            for k in ("mean_h", "marginal", "log_is", "marginal_scale"):
                out[k].append(math.nan)
            continue
        n = len(hs)
        mean_h = _ld_sum(np.array(hs, dtype=LD)) / n
        # (the column sums as longdouble sums: n_b terms in a 64-bit significand, n_b 2^-64 relative - the one sum here
        # that is not math.fsum, because there are C of them per group)
        pbar = np.array(ps, dtype=LD).sum(axis=0) / n
        live = pbar > 0
        terms = np.where(live, pbar * np.log(np.where(live, pbar, LD(1))), LD(0))
        m = _ld_sum(terms)
        out["mean_h"].append(float(mean_h))
        out["marginal"].append(float(m))
        out["log_is"].append(float(mean_h - m))
        out["marginal_scale"].append(float(_ld_sum(np.abs(terms))) + 1.0)
    for k in ("mean_h", "marginal", "log_is", "nonfinite", "marginal_scale"):
        out[k] = np.array(out[k], dtype=np.float64)
    return out


def _sigmoid_parts(x):
    """(s, 1 - s, log s, log(1 - s)) of the logistic function in longdouble, in the stable forms."""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    z = np.exp(-np.abs(x))
    l1p = np.log1p(z)
    big, small = 1 / (1 + z), z / (1 + z)
    pos = x >= 0
    return np.where(pos, big, small), np.where(pos, small, big), np.minimum(x, 0) - l1p, np.minimum(-x, 0) - l1p


def pair_value(cand, ref, mode, eps=0.0):
    """(value, scale) of one row pair: scale = the sum of the absolute values of the terms + 1.  cosine: the terms are
    a_c b_c / (|a| |b|).  A pair without a value gives (NaN or +-inf, NaN)."""
    c, r = np.asarray(cand, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(all="ignore"):
        if mode == "cosine":
            na, nb = _ld_sum(c.astype(LD) ** 2) if np.isfinite(c).all() else LD(np.nan), \
                _ld_sum(r.astype(LD) ** 2) if np.isfinite(r).all() else LD(np.nan)
            if not (np.isfinite(na) and np.isfinite(nb)) or na == 0 or nb == 0:
                return math.nan, math.nan
            terms = c.astype(LD) * r.astype(LD) / np.sqrt(na * nb)
        elif mode == "kl_softmax":
            if not (row_is_finite(c) and row_is_finite(r)):
                return math.nan, math.nan
            dr, dc = (r - r.max()).astype(LD), (c - c.max()).astype(LD)
            er, ec = np.exp(dr), np.exp(dc)
            sr, sc = _ld_sum(er), _ld_sum(ec)
            pr = er / sr
            lq = (dc - np.log(sc)) if eps == 0 else np.log(ec / sc + LD(eps))
            live = er > 0
            if (live & (lq == -np.inf)).any():
                return math.inf, math.nan
            terms = np.where(live, pr * (np.where(live, dr, LD(0)) - np.log(sr) - np.where(live, lq, LD(0))), LD(0))
        elif mode in ("kl_sigmoid", "kl_bernoulli"):
            if np.isnan(c).any() or np.isnan(r).any():
                return math.nan, math.nan
            s, ns, ls, lns = _sigmoid_parts(r)
            t, nt, lt, lnt = _sigmoid_parts(c)
            lq, lnq = (lt, lnt) if eps == 0 else (np.log(t + LD(eps)), np.log(nt + LD(eps)))
            one = np.where(s > 0, s * (np.where(s > 0, ls, LD(0)) - np.where(s > 0, lq, LD(0))), LD(0))
            if mode == "kl_sigmoid":
                terms = one
            else:
                zero = np.where(ns > 0, ns * (np.where(ns > 0, lns, LD(0)) - np.where(ns > 0, lnq, LD(0))), LD(0))
                terms = np.concatenate([one, zero])
            if not np.isfinite(terms).all():
                return float(terms.astype(np.float64).sum()), math.nan
        else:
            raise ValueError(mode)
    return float(_ld_sum(terms)), float(_ld_sum(np.abs(terms))) + 1.0


def pair_rows(cand, ref, mode, eps=0.0):
    """(values [N], scales [N]) of the row pairs of two matrices."""
    got = [pair_value(c, r, mode, eps) for c, r in zip(np.asarray(cand), np.asarray(ref))]
    return np.array([g[0] for g in got]), np.array([g[1] for g in got])


def paired_summary(values):
    """(mean, standard error, used, left out) over the finite values: ddof = 1, NaN for fewer than 2."""
    v = np.asarray(values, dtype=np.float64)
    fin = v[np.isfinite(v)]
    used, left = int(fin.size), int(v.size - fin.size)
    if used == 0:
        return math.nan, math.nan, used, left
    mean = math.fsum(fin) / used
    if used < 2:
        return mean, math.nan, used, left
    return mean, math.sqrt(math.fsum((fin - mean) ** 2) / (used - 1) / used), used, left


def split_plan(n, splits, seed=None):
    """The row indices of every split: list positions [k n // splits, (k + 1) n // splits) of the stored order, or of
    numpy.random.default_rng(seed).permutation(n)."""
    order = np.arange(n) if seed is None else np.random.default_rng(seed).permutation(n)
    return [order[k * n // splits:(k + 1) * n // splits] for k in range(splits)]


def inception(logits, splits=10, seed=None):
    """The result dict of inception_score from the definitions (and "groups": the class_groups record behind it)."""
    logits = np.asarray(logits, dtype=np.float64)
    plan = split_plan(len(logits), splits, seed)
    g = class_groups(logits, plan)
    sizes = np.array([len(p) for p in plan], dtype=np.float64)
    per_split = np.exp(g["log_is"])
    mean = math.fsum(per_split) / splits
    ent = np.empty(len(logits))
    for rows, h in zip(plan, g["h"]):
        ent[rows] = -h
    return {"inception_score": mean, "inception_score_std": math.sqrt(math.fsum((per_split - mean) ** 2) / splits),
            "inception_score_per_split": per_split,
            "inception_conditional_entropy": -math.fsum(sizes * g["mean_h"]) / len(logits),
            "inception_marginal_entropy": -math.fsum(sizes * g["marginal"]) / len(logits),
            "inception_n_splits": splits, "row_entropy": ent, "groups": g}


def record_accuracy(section, lines):
    """Replace one section ("## title" and the lines under it) of profiles/class_scores/accuracy.txt, keeping the others:
    the GPU tests write what they measured there.  A tree that cannot be written to is not an error of the test."""
    sections, title = {}, None
    try:
        with open(ACCURACY_FILE) as f:
            for line in f.read().splitlines():
                if line.startswith("## "):
                    title = line[3:]
                    sections[title] = []
                elif title is not None and line.strip():
                    sections[title].append(line)
    except OSError:
        pass
    sections[section] = list(lines)
    try:
        os.makedirs(os.path.dirname(ACCURACY_FILE), exist_ok=True)
        with open(ACCURACY_FILE, "w") as f:
            for title in sorted(sections):
                f.write("## %s\n%s\n\n" % (title, "\n".join(sections[title])))
    except OSError:
        pass
