"""Host checks of what tests/test_gpu_kd.py stands on: the exact-arithmetic data really is exact on every device form,
and the rounding tolerances of its real-valued cases sit between the emulated error of a correct split-f16 form and the
emulated error of the same form with the lo plane dropped (plain f16 operands) - a tolerance edited past that line would
let a precision loss of two to three orders of magnitude through."""
import math

import numpy as np
import pytest

import kd_reference as kr


@pytest.mark.parametrize("d", [1, 31, 33, 100, 129, 512, 8192, 9000])
def test_exact_rows_give_exact_dot_products(d):
    rng = np.random.default_rng(d)
    x = kr.exact_rows(rng, 48, d)
    y = kr.exact_rows(rng, 40, d)
    x[0] = 3 * np.exp2(8)                                   # the largest magnitude the generator can produce, whole row
    y[0] = -3 * np.exp2(8)
    want = x.astype(np.float64) @ y.astype(np.float64).T
    assert np.all(np.abs(want[0, 0]) == 9 * d * 2.0 ** 16)
    # f32 matmul in any order, the f32 tile form's slab accumulation, and the split form with its hi plane alone
    np.testing.assert_array_equal((x @ y.T).astype(np.float64), want)
    np.testing.assert_array_equal(kr.emulated_dots("f32")(x, y), want)
    np.testing.assert_array_equal(kr.emulated_dots("split")(x, y), want)
    np.testing.assert_array_equal(kr.emulated_dots("hi_only")(x, y), want)
    hi, lo, _ = kr.split_planes(x)
    assert not lo.any()
    # RBF: squared norms and the device's d^2 = |x|^2 + |y|^2 - 2 <x, y> exact in float64 (math.fsum: correctly rounded)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    nx, ny = (x64 ** 2).sum(1), (y64 ** 2).sum(1)
    for i in range(0, 48, 7):
        assert nx[i] == math.fsum(x64[i] ** 2)
        for j in range(0, 40, 9):
            assert (nx[i] + ny[j]) - 2.0 * want[i, j] == math.fsum((x64[i] - y64[j]) ** 2)


def test_exact_rows_scaled_stay_exact_in_the_split_form():
    """The per-row scale sweep of the GPU suite (2^s, s in [-36, 36]) keeps every f32 dot product normal and exact."""
    rng = np.random.default_rng(7)
    x, y = kr.exact_rows(rng, 32, 300), kr.exact_rows(rng, 32, 300)
    want = x.astype(np.float64) @ y.astype(np.float64).T
    for s in (-36, -20, 20, 36):
        xs, ys = (x * np.float32(2.0 ** s)).astype(np.float32), (y * np.float32(2.0 ** s)).astype(np.float32)
        ex = kr.half_scale_exp(np.abs(xs).max(1))
        assert ex.min() >= -60 and ex.max() <= 60
        np.testing.assert_array_equal(kr.emulated_dots("split")(xs, ys), want * 2.0 ** (2 * s))


def test_index_tables_hold_the_first_and_last_rows():
    rng = np.random.default_rng(3)
    i1, i2 = kr.index_tables(rng, 700, 650, 5, 300)
    for t, n in ((i1, 700), (i2, 650)):
        assert t.shape == (5, 300) and t.min() >= 0 and t.max() < n
        for row in t:
            assert len(set(row.tolist())) == 300 and 0 in row and n - 1 in row


def test_oracle_matches_the_reference_formulation():
    """subset_values agrees with oracle.kid_from_features (the reference's subset loop) on its own index tables."""
    import oracle
    rng = np.random.default_rng(11)
    f1, f2 = rng.standard_normal((300, 24)), rng.standard_normal((280, 24)) + 0.2
    for kind, kw in (("poly", dict(degree=2, gamma=0.05, coef0=0.5)), ("rbf", dict(sigma=3.0))):
        ref_kw = dict(kernel_type="rbf", sigma=3.0) if kind == "rbf" else kw
        _, want = oracle.kid_from_features(f1, f2, subsets=3, subset_size=100, seed=5, return_all=True, **ref_kw)
        i1, i2 = oracle.draw_subsets(300, 280, 3, 100, 5)
        got, _ = kr.subset_values(f1, f2, i1, i2, kr.Kernel(kind, **kw))
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("name", [c[0] for c in kr.ROUNDING_CASES])
def test_rounding_tolerance_separates_split_from_plain_f16(name):
    x, y, i1, i2, form, kernel = kr.rounding_case(name)
    want, scale = kr.subset_values(x, y, i1, i2, kernel)
    tol = kr.rounding_tolerance(kr.emulated_errors(x, y, i1, i2, form, kernel, want))
    plain = kr.emulated_errors(x, y, i1, i2, "hi_only", kernel, want)
    assert tol > 0
    # plain f16 operands must fail the GPU check on most subsets of every case (the hi planes are the device's own bits:
    # the emulated error of that form is what the device would show, up to its accumulation order)
    assert np.sum(plain > tol) > len(plain) // 2, f"{name}: tolerance {tol:.3g} does not exclude plain f16 operands {plain}"
    assert tol < 1e-4 * np.abs(want).max() + 5e-7                     # tighter than the golden tests' limit
