"""Float64 numpy oracle of the debiased Sinkhorn divergence (audio_metrics_amd.metrics.sinkhorn restated, with stored cost
matrices and a stable log-sum-exp): soft-min, schedule and the three solves.

  C(a, b) = |a - b|^2 / 2 in f64 from the rows as given (the tests hand in the float32 rows the device reads)
  T_eps(Y, g)(x_i) = -eps log((1 / m) sum_j exp((g_j - C(x_i, y_j)) / eps))
  schedule: diam2, diam2 scaling^2, ... while above blur^2, then blur^2
  XY alternating (f <- T(Y, g)(X); g <- T(X, f)(Y) with the new f), XX / YY symmetric and averaged (p <- (p + T(X, p)(X)) / 2);
  one step per schedule entry, then steps at blur^2 until max |change| <= rtol max |potential| or max_iter steps in all;
  final values from the last potentials; S = mean(f* - p*) + mean(g* - q*)."""
import os

import numpy as np


def half_sq_dists(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    d2 = (x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2.0 * (x @ y.T)
    return 0.5 * np.maximum(d2, 0.0)


def softmin(cost, g, eps):
    """T_eps for every row of the [n, m] cost matrix and potentials g [m]."""
    z = (np.asarray(g, dtype=np.float64)[None, :] - cost) / eps
    mx = z.max(axis=1)
    return -eps * (mx + np.log(np.exp(z - mx[:, None]).sum(axis=1)) - np.log(cost.shape[1]))


def diam2(*sets):
    pooled = np.concatenate([np.asarray(s, dtype=np.float64) for s in sets], axis=0)
    return float(((pooled.max(axis=0) - pooled.min(axis=0)) ** 2).sum())


def schedule(d2, blur, scaling):
    out, eps = [], float(d2)
    while eps > blur * blur:
        out.append(eps)
        eps *= scaling * scaling
    out.append(blur * blur)
    return out


def solve_self(cost, sched, rtol, max_iter):
    """{"star": p*, "steps", "converged", "history": one (eps, largest |potential| the step read, change, magnitude) per step}"""
    p = np.zeros(cost.shape[0])
    history, converged = [], False
    step = 0
    while True:
        eps = sched[min(step, len(sched) - 1)]
        new = 0.5 * (p + softmin(cost, p, eps))
        history.append((eps, float(np.abs(p).max()), float(np.abs(new - p).max()), float(np.abs(new).max())))
        p = new
        step += 1
        if step >= len(sched):
            if history[-1][2] <= rtol * history[-1][3]:
                converged = True
                break
            if step >= max_iter:
                break
    return {"star": softmin(cost, p, sched[-1]), "last": p, "steps": step, "converged": converged, "history": history}


def solve_cross(cost, sched, rtol, max_iter):
    """cost [n, m]; {"f_star", "g_star", "f", "g", "steps", "converged", "history"}"""
    f, g = np.zeros(cost.shape[0]), np.zeros(cost.shape[1])
    history, converged = [], False
    step = 0
    while True:
        eps = sched[min(step, len(sched) - 1)]
        f_new = softmin(cost, g, eps)
        g_new = softmin(cost.T, f_new, eps)
        history.append((eps, float(max(np.abs(g).max(), np.abs(f_new).max())),
                        float(max(np.abs(f_new - f).max(), np.abs(g_new - g).max())),
                        float(max(np.abs(f_new).max(), np.abs(g_new).max()))))
        f, g = f_new, g_new
        step += 1
        if step >= len(sched):
            if history[-1][2] <= rtol * history[-1][3]:
                converged = True
                break
            if step >= max_iter:
                break
    eps = sched[-1]
    return {"f_star": softmin(cost, g, eps), "g_star": softmin(cost.T, f, eps), "f": f, "g": g, "steps": step,
            "converged": converged, "history": history}


def divergence(x, y, blur, scaling=0.5, rtol=1e-5, max_iter=200):
    x, y = np.asarray(x), np.asarray(y)
    xy = solve_cross(half_sq_dists(x, y), schedule(diam2(x, y), blur, scaling), rtol, max_iter)
    xx = solve_self(half_sq_dists(x, x), schedule(diam2(x), blur, scaling), rtol, max_iter)
    yy = solve_self(half_sq_dists(y, y), schedule(diam2(y), blur, scaling), rtol, max_iter)
    ot_xy = xy["f_star"].mean() + xy["g_star"].mean()
    ot_xx, ot_yy = 2.0 * xx["star"].mean(), 2.0 * yy["star"].mean()
    eps = blur * blur
    return {"divergence": float(ot_xy - 0.5 * ot_xx - 0.5 * ot_yy), "ot_xy": float(ot_xy), "ot_xx": float(ot_xx),
            "ot_yy": float(ot_yy), "candidate_potential": xy["f_star"] - xx["star"], "reference_potential": xy["g_star"] - yy["star"],
            "iterations": (xy["steps"], xx["steps"], yy["steps"]), "converged": (xy["converged"], xx["converged"], yy["converged"]),
            "marginal_error": float(np.abs(np.expm1((xy["f"] - xy["f_star"]) / eps)).max()), "xy": xy, "xx": xx, "yy": yy}


def delta(eps, d, x2max, y2max, gmax):
    """Worst-case error of one device soft-min against this oracle on the same float32 rows:
    2^-24 (D + 16) (max |x|^2 + max |y|^2 + max |g|)  - the f32 dot product, d2 and z -  plus  2^-21 eps  - exp and the sum."""
    return 2.0 ** -24 * (d + 16) * (x2max + y2max + gmax) + 2.0 ** -21 * eps


ACCURACY_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sinkhorn", "accuracy.txt")


def record_accuracy(section, lines):
    """Replace one section ("## title" and the lines under it) of profiles/sinkhorn/accuracy.txt, keeping the others: the GPU
    tests write what they measured there.  A tree that cannot be written to is not an error of the test."""
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


def solve_bound(history, d, x2max, y2max):
    """sum over the steps of delta(eps_t): every potential of a device solve lies within it of the oracle's after the same
    steps (soft-min is 1-Lipschitz in g and in C, averaging keeps that); S within four times the largest of the three."""
    return sum(delta(eps, d, x2max, y2max, gmax) for eps, gmax, _, _ in history)
