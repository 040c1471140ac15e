"""Multi-scale kernel sums, test support, host only: a float64 oracle of the three normalised whole-set sums under the
kernels of am_mmd_multi_f32, in the arithmetic include/audio_metrics_hip.h documents, on kad_reference.d2_matrix (and its
optional emulated dot products):

  gaussian  exp(-d2 g), g = 0.5 / (bw2 (c c))      laplacian  exp(-sqrt(d2) h), h = 1 / (c sqrt(bw2))      energy  -sqrt(d2)

Used by tests/test_gpu_mmd_multi.py (the kernels against the oracle) and tests/test_mmd_multi_cpu.py (the oracle itself)."""
import math

import numpy as np

import kad_reference as ka

KINDS = ("gaussian", "laplacian", "energy")


def parameter(kind, bw2, c):
    """The kernel parameter of scale c, formed in the order the device forms it."""
    if kind == "gaussian":
        return 0.5 / (bw2 * (c * c))
    if kind == "laplacian":
        return 1.0 / (c * math.sqrt(bw2))
    return 0.0


def kernel_matrix(kind, d2, bw2=None, c=1.0):
    with np.errstate(over="ignore", invalid="ignore"):
        if kind == "gaussian":
            return np.exp(-d2 * parameter(kind, bw2, c))
        if kind == "laplacian":
            return np.exp(-np.sqrt(d2) * parameter(kind, bw2, c))
        if kind == "energy":
            return -np.sqrt(d2)
    raise ValueError(kind)


def distances(x, y, dots=None):
    """The three d2 matrices (xx, yy, xy) every kernel and scale of a pair of sets is evaluated on."""
    return tuple(ka.d2_matrix(a, b, dots) for a, b in ((x, x), (y, y), (x, y)))


def parts_from_distances(d2, kind, bw2=None, c=1.0):
    """(means, scale) as kad_reference.mmd_parts: means = [Sxx / (n (n - 1)), Syy / (m (m - 1)), Sxy / (n m)] in f64 - Sxx, Syy
    over ordered pairs i != j - and scale = mean |K| over the three blocks."""
    kxx, kyy, kxy = (kernel_matrix(kind, d, bw2, c) for d in d2)
    n, m = kxy.shape
    means = np.array([(kxx.sum() - np.trace(kxx)) / (n * (n - 1.0)), (kyy.sum() - np.trace(kyy)) / (m * (m - 1.0)),
                      kxy.sum() / (float(n) * m)])
    return means, float(np.mean([np.abs(k).mean() for k in (kxx, kyy, kxy)]))


def parts(x, y, kind, bw2=None, c=1.0, dots=None):
    return parts_from_distances(distances(x, y, dots), kind, bw2, c)


def mixture_parts(x, y, kind, bw2, scales):
    """means of the mixture kernel mean_c k_c, from the averaged kernel matrices themselves (not from the per-scale means)."""
    n, m = len(x), len(y)
    out = []
    for a, b, same in ((x, x, True), (y, y, True), (x, y, False)):
        d2 = ka.d2_matrix(a, b)
        k = sum(kernel_matrix(kind, d2, bw2, c) for c in scales) / float(len(scales))
        out.append((k.sum() - np.trace(k)) / (len(a) * (len(a) - 1.0)) if same else k.sum() / (float(n) * m))
    return np.array(out)


def energy_from_means(means):
    """2 E|x - y| - E|x - x'| - E|y - y'| from the means of k = -d: the MMD^2 of that kernel."""
    return ka.mmd2(means)
