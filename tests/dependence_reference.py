"""Dependence of paired sets, test support, host only: a float64 numpy oracle that U-centres the two pair matrices
EXPLICITLY (Szekely & Rizzo 2014; Song et al. 2012) instead of using the row-sum identity of metrics/dependence.py:

  A~_ij = a_ij - A_i / (n - 2) - A_j / (n - 2) + T_a / ((n - 1)(n - 2))   (i != j; 0 on the diagonal)
  U(a, b) = sum_{i != j} A~_ij B~_ij / (n (n - 3))

on kad_reference.d2_matrix (and its optional emulated dot products) and mmd_multi_reference.kernel_matrix; the distance kind is
+sqrt(d2) (the "energy" kernel of the kernel sums with the other sign).

Used by tests/test_dependence_cpu.py (the host arithmetic against it) and tests/test_gpu_dependence.py (the kernel)."""
import numpy as np

import kad_reference as ka
import mmd_multi_reference as mr

KINDS = ("energy", "gaussian", "laplacian")


def pair_matrix(rows, kind, bw2=None, dots=None):
    """a_ij of one side, f64 [n, n], zero diagonal"""
    d2 = ka.d2_matrix(rows, rows, dots)
    m = np.sqrt(d2) if kind == "energy" else mr.kernel_matrix(kind, d2, bw2, 1.0)
    m = np.array(m, dtype=np.float64)
    np.fill_diagonal(m, 0.0)
    return m


def row_sums(a, b):
    """[n, 5] {A_i, B_i, H_i, AA_i, BB_i} of two pair matrices with zero diagonals"""
    return np.stack([a.sum(1), b.sum(1), (a * b).sum(1), (a * a).sum(1), (b * b).sum(1)], axis=1)


def totals(rows):
    """the eight totals dependence_from_sums takes: T_a, T_b, S_ab, S_aa, S_bb, C_ab, C_aa, C_bb"""
    A, B = rows[:, 0], rows[:, 1]
    return np.array([*rows.sum(0), A @ B, A @ A, B @ B])


def u_centre(a):
    n = a.shape[0]
    r = a.sum(1)
    c = a - r[:, None] / (n - 2.0) - r[None, :] / (n - 2.0) + r.sum() / ((n - 1.0) * (n - 2.0))
    np.fill_diagonal(c, 0.0)
    return c


def u_statistic(a, b):
    n = a.shape[0]
    return float((u_centre(a) * u_centre(b)).sum() / (n * (n - 3.0)))


def v_statistic(a, b):
    """the classical double-centred V-statistic: mean of A^_ij B^_ij over all n^2 entries"""
    def centre(m):
        return m - m.mean(1)[:, None] - m.mean(0)[None, :] + m.mean()
    return float((centre(a) * centre(b)).mean())


def statistics(a, b):
    """{"u_ab", "u_aa", "u_bb", "v_ab", "v_aa", "v_bb"} by explicit centring"""
    return {"u_ab": u_statistic(a, b), "u_aa": u_statistic(a, a), "u_bb": u_statistic(b, b),
            "v_ab": v_statistic(a, b), "v_aa": v_statistic(a, a), "v_bb": v_statistic(b, b)}
