"""Float64 numpy oracle of the sliced Wasserstein distance (audio_metrics_amd.metrics.sliced restated): the directions, the
projections, the 1-D W_p^p of two uniform empirical measures on the merged grid {i / n} u {j / m}, and the result dict.

  directions   default_rng(seed).standard_normal((L, D)), rows normalised in f64, rounded to float32 once
  projections  z[l, i] = <theta_l, x_i> in f64 from the float32 rows and directions the device reads
  W_p^p        both samples sorted; the breakpoints of the two quantile functions are the merged grid, so
               W_p^p = sum over the grid's cells of (cell length) |x_(i) - y_(j)|^p with i = floor(t n), j = floor(t m)
               (wpp_merged, vectorised; wpp_repeat is the same coupling written as n m atoms of weight 1 / (n m))"""
import math
import os

import numpy as np


def directions(d, n_projections, seed):
    g = np.random.default_rng(seed).standard_normal((n_projections, d))
    return (g / np.sqrt((g * g).sum(axis=1, keepdims=True))).astype(np.float32)


def project(x, theta):
    """float64 [L, N]."""
    return np.asarray(theta, dtype=np.float64) @ np.asarray(x, dtype=np.float64).T


def wpp_merged(xs, ys, p):
    """W_p^p of two SORTED 1-D samples (uniform weights) in f64, on the merged grid with integer breakpoints k m (k <= n)
    and k n (k <= m) in units of 1 / (n m)."""
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    n, m = len(xs), len(ys)
    cuts = np.union1d(np.arange(n + 1, dtype=np.int64) * m, np.arange(m + 1, dtype=np.int64) * n)
    lo, hi = cuts[:-1], cuts[1:]
    diff = np.abs(xs[lo // m] - ys[lo // n])
    return float(np.sum(((hi - lo) / float(n * m)) * (diff if p == 1 else diff * diff)))


def wpp_repeat(xs, ys, p):
    """The same with every atom of x repeated m times and every atom of y n times: n m pairs of weight 1 / (n m)."""
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    diff = np.abs(np.repeat(xs, len(ys)) - np.repeat(ys, len(xs)))
    return float(np.mean(diff if p == 1 else diff * diff))


def per_projection(x, y, theta, p):
    """float64 [L]: W_p^p between the projections of the rows of x and of y on every direction."""
    zx, zy = np.sort(project(x, theta), axis=1), np.sort(project(y, theta), axis=1)
    return np.array([wpp_merged(a, b, p) for a, b in zip(zx, zy)])


def summary(w, p):
    """The result dict from the per-projection W_p^p values."""
    w = np.asarray(w, dtype=np.float64)
    n = len(w)
    swd_pp = float(np.sum(w) / n)
    swd = swd_pp ** (1.0 / p)
    imax = int(np.argmax(w))
    err = math.nan
    if n > 1 and swd > 0.0:
        s = math.sqrt(float(np.sum((w - swd_pp) ** 2)) / (n - 1))
        err = s / (math.sqrt(n) * p * swd ** (p - 1))
    return {"swd": swd, "swd_pp": swd_pp, "swd_p": p, "swd_n_projections": n, "swd_max": float(w[imax]) ** (1.0 / p),
            "swd_max_index": imax, "swd_std_error": err}


def distance(x, y, n_projections, p, seed):
    theta = directions(np.asarray(x).shape[1], n_projections, seed)
    w = per_projection(x, y, theta, p)
    out = summary(w, p)
    out.update(swd_seed=seed, swd_per_projection=w, swd_directions=theta)
    return out


ACCURACY_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "swd", "accuracy.txt")


def record_accuracy(section, lines):
    """Replace one section ("## title" and the lines under it) of profiles/swd/accuracy.txt, keeping the others: the GPU tests
    write what they measured there.  A tree that cannot be written to is not an error of the test."""
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
