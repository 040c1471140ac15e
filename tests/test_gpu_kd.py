"""Kernel distance on every device route against a float64 oracle (tests/kd_reference.py).

Two kinds of data:
  exact    integers in [-3, 3] times a per-row power of two: every dot product is exact on every route, so what is left
           is float64 summation order and exp / pow at the ulp level.  Limit per subset: 1e-12 x mean |K| of its three
           blocks - one wrong diagonal entry, padding entry or tile weight is 10^5 - 10^6 times over it.
  rounding real-valued rows (inputs.pair) at m = 1000; the limit is MARGIN times the error of a CPU emulation of the
           device arithmetic, which tests/test_kd_numerics_cpu.py keeps below the error of plain f16 operands.
Every case asserts the form it takes (am_kd_path: 0 f32 tile, 1 f32 tile with a D % 32 tail, 2 generic pointers for
matrices of >= 4 GiB, 3 split-f16; float64 rows on either side take the kd64 kernels instead)."""
import numpy as np
import pytest
import torch

import kd_reference as kr

pytestmark = pytest.mark.gpu

EXACT = 1e-12
DEV = "cuda:0"
M_SWEEP = [1, 2, 127, 128, 129, 255, 256, 257, 511, 512, 513, 767, 1000, 1024, 1500]
D_SWEEP = [1, 31, 33, 64, 100, 127, 128, 129, 191, 200, 512, 1000, 8192, 9000]
COEF0 = [0.0, 1.0, -1.0, 2.5]
GAMMA = [None, 1e-3, 1.0]                                  # None: 1 / D


@pytest.fixture(scope="module")
def ops():
    import audio_metrics_amd as am
    am._lib.load()
    return am.hip_ops


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def expected_route(m, d, degree=3, rbf=False, big=False):
    """The dispatch rule the suite expects (include/audio_metrics_hip.h, am_kd_path)."""
    if not rbf and degree == 3 and m >= 512 and 128 <= d <= 8192:
        return 3
    if big:
        return 2
    return 1 if d % 32 else 0


def route_of(ops, xt, yt, m, kernel):
    def ld(t):
        return t.stride(0) if t.shape[0] > 1 else (t.shape[1] + 3) // 4 * 4
    x, y = ops.as_matrix(xt), ops.as_matrix(yt)
    return ops.kd_path(x.shape[0], ld(x), y.shape[0], ld(y), x.shape[1], m, kernel.degree, kernel.kind == "rbf")


def kd(ops, xt, yt, i1, i2, kernel):
    """per-subset device values (numpy f64[S]) of hip_ops.kd_poly / kd_rbf"""
    t1, t2 = dev(i1), dev(i2)
    if kernel.kind == "rbf":
        out = ops.kd_rbf(xt, yt, t1, t2, kernel.sigma)
    else:
        gamma = 1.0 / xt.shape[1] if kernel.gamma is None else kernel.gamma
        out = ops.kd_poly(xt, yt, t1, t2, gamma, kernel.coef0, kernel.degree)
    return out.cpu().numpy()


def check_exact(got, x, y, i1, i2, kernel, what=""):
    want, scale = kr.subset_values(x, y, i1, i2, kernel)
    err = np.abs(got - want)
    bad = ~(err <= EXACT * scale)
    assert not bad.any(), f"{what}: subsets {np.flatnonzero(bad)} got {got[bad]} want {want[bad]} (mean|K| {scale[bad]})"
    return want


def run_exact(ops, m, d, S, kernel, route, seed, n1=None, n2=None, xdtype=np.float32, ydtype=np.float32, rows=None):
    rng = np.random.default_rng(seed)
    n1, n2 = n1 or m + 3, n2 or m + 7
    make = rows or (lambda n: kr.exact_rows(rng, n, d))
    x, y = make(n1).astype(xdtype), make(n2).astype(ydtype)
    i1, i2 = kr.index_tables(rng, n1, n2, S, m)
    xt, yt = dev(x), dev(y)
    if route is not None:
        assert route_of(ops, xt, yt, m, kernel) == route
    got = kd(ops, xt, yt, i1, i2, kernel)
    if m == 1:
        assert np.isnan(got).all(), got                                      # the reference's 0 / 0
        return got
    check_exact(got, x, y, i1, i2, kernel, f"m={m} D={d} {vars(kernel)}")
    return got


# ---------------------------------------------------------------------------------------------------- (a) exact data

@pytest.mark.parametrize("i,m", list(enumerate(M_SWEEP)))
@pytest.mark.parametrize("d", [512, 100])
def test_exact_subset_size_sweep(ops, i, m, d):
    """128-row tiles of the f32 forms (D = 100: with the tail), 256-row tiles of the split form (D = 512, m >= 512),
    padding and diagonal removal in partial tiles, every coef0 and gamma in turn."""
    j = i + (d == 100)
    kernel = kr.Kernel("poly", GAMMA[j % 3], COEF0[j % 4], 3)
    run_exact(ops, m, d, 2 if m >= 1500 else 3, kernel, expected_route(m, d), 100 + i + d)


@pytest.mark.parametrize("i,d", list(enumerate(D_SWEEP)))
@pytest.mark.parametrize("m", [600, 200])
def test_exact_width_sweep(ops, i, d, m):
    """every tail instantiation, DP padding to 64 in the split form, both sides of D = 128 and 8192."""
    j = i + (m == 200)
    kernel = kr.Kernel("poly", GAMMA[j % 3], COEF0[j % 4], 3)
    run_exact(ops, m, d, 2 if d >= 8192 else 3, kernel, expected_route(m, d), 300 + i + m)


@pytest.mark.parametrize("degree", [0, 1, 2, 3, 4, 16])
@pytest.mark.parametrize("d", [64, 100])
def test_exact_degree_sweep(ops, degree, d):
    for j, (gamma, coef0) in enumerate([(None, 1.0), (1e-3, -1.0), (1.0, 2.5), (1e-3, 0.0)]):
        kernel = kr.Kernel("poly", gamma, coef0, degree)
        got = run_exact(ops, 300, d, 3, kernel, expected_route(300, d, degree), 500 + 10 * degree + j + d)
        if degree == 0:
            assert (got == 0.0).all(), got                 # every K is 1; the padding term is an integer count


def test_exact_degree_zero_is_zero_at_split_shapes(ops):
    """degree 0 at m = 1000: not the split form (degree 3 only) - the f32 form with 128-row padding - and exactly 0."""
    got = run_exact(ops, 1000, 512, 3, kr.Kernel("poly", None, 2.5, 0), 0, 17)
    assert (got == 0.0).all(), got


@pytest.mark.parametrize("coef0", [0.0, -1.0, 2.5])
@pytest.mark.parametrize("m,d", [(513, 129), (767, 200), (1024, 1000)])
def test_exact_split_form_with_other_coef0(ops, coef0, m, d):
    """the split form's padding term (KW^2 - vq vp) kval(0) depends on coef0 and on m mod 256"""
    for gamma in (1e-3, 1.0):
        run_exact(ops, m, d, 3, kr.Kernel("poly", gamma, coef0, 3), 3, 700 + m + d + int(4 * coef0))


@pytest.mark.parametrize("sigma", [0.5, 3.0, 10.0, 1e3])
@pytest.mark.parametrize("m,d", [(129, 64), (300, 100), (513, 33)])
def test_exact_rbf(ops, sigma, m, d):
    """kd_tile_kernel<2> (D % 32 == 0) and <3> (tail) on f32 rows, kd64_kernel<1> on f64 rows"""
    kernel = kr.Kernel("rbf", sigma=sigma)

    def rows(n, rng=np.random.default_rng(int(sigma * 10) + m)):
        return kr.rbf_rows(rng, n, d, sigma)
    run_exact(ops, m, d, 3, kernel, expected_route(m, d, rbf=True), 900 + m, rows=rows)
    got = run_exact(ops, m, d, 3, kernel, None, 901 + m, rows=rows, xdtype=np.float64, ydtype=np.float64)
    assert np.isfinite(got).all()


@pytest.mark.parametrize("d", [1, 15, 16, 17, 129])
@pytest.mark.parametrize("m", [63, 64, 65])
def test_exact_f64_and_mixed_rows(ops, d, m):
    """float64 on either side: the kd64 kernels (64-row tiles, 16-element slabs)"""
    j = d + m
    poly = kr.Kernel("poly", GAMMA[j % 3], COEF0[j % 4], 3)
    run_exact(ops, m, d, 3, poly, None, 1000 + j, xdtype=np.float64, ydtype=np.float64)
    run_exact(ops, m, d, 3, poly, None, 1001 + j, xdtype=np.float32, ydtype=np.float64)
    run_exact(ops, m, d, 3, kr.Kernel("poly", 1.0, -1.0, 4), None, 1002 + j, xdtype=np.float64, ydtype=np.float32)
    rbf = kr.Kernel("rbf", sigma=3.0)

    def rows(n, rng=np.random.default_rng(j)):
        return kr.rbf_rows(rng, n, d, 3.0)
    run_exact(ops, m, d, 3, rbf, None, 1003 + j, xdtype=np.float64, ydtype=np.float32, rows=rows)


@pytest.mark.parametrize("S,m,d", [(1, 600, 256), (7, 300, 100), (100, 200, 64), (100, 520, 128)])
def test_exact_subset_counts(ops, S, m, d):
    run_exact(ops, m, d, S, kr.Kernel("poly", None, 1.0, 3), expected_route(m, d), 1200 + S + m)


@pytest.mark.parametrize("m,d,ld", [(300, 100, 132), (600, 200, 260)])
def test_exact_row_views(ops, m, d, ld):
    """a column slice (ld > D, ld % 4 == 0) and a row-offset view are read in place; a misaligned view is copied"""
    rng = np.random.default_rng(1300 + m)
    n = m + 40
    base = kr.exact_rows(rng, n + 8, ld)
    kernel = kr.Kernel("poly", 1e-3, -1.0, 3)
    i1, i2 = kr.index_tables(rng, n, n, 3, m)
    bt = dev(base)
    views = {
        "column slice": (bt[:n, :d], base[:n, :d], True),
        "row offset": (bt[5:5 + n, :d], base[5:5 + n, :d], True),
        "misaligned": (bt[3:3 + n, 1:1 + d], base[3:3 + n, 1:1 + d], False),
    }
    for name, (v, host, in_place) in views.items():
        assert (ops.as_matrix(v).data_ptr() == v.data_ptr()) == in_place, name
        assert route_of(ops, v, bt[:n, :d], m, kernel) == expected_route(m, d)
        got = kd(ops, v, bt[:n, :d], i1, i2, kernel)
        check_exact(got, host, base[:n, :d], i1, i2, kernel, name)


@pytest.mark.parametrize("d", [256, 1000])
def test_exact_split_form_per_row_scale(ops, d):
    """rows times 2^s, gamma times 2^-2s, coef0 = 0: the split form's per-row exponents run from -32 to 57 (inside the
    +-60 clamp) and every value must equal the unscaled one, bit for bit, and the oracle"""
    rng = np.random.default_rng(1400 + d)
    m, n = 600, 640
    x, y = kr.exact_rows(rng, n, d), kr.exact_rows(rng, n, d)
    i1, i2 = kr.index_tables(rng, n, n, 3, m)
    base = None
    for s in (-36, -20, 0, 20, 36):
        xs, ys = (x * np.float32(2.0 ** s)).astype(np.float32), (y * np.float32(2.0 ** s)).astype(np.float32)
        kernel = kr.Kernel("poly", 2.0 ** (-2 * s) / d, 0.0, 3)
        xt, yt = dev(xs), dev(ys)
        assert route_of(ops, xt, yt, m, kernel) == 3
        got = kd(ops, xt, yt, i1, i2, kernel)
        check_exact(got, xs, ys, i1, i2, kernel, f"scale 2^{s}")
        if base is None:
            base = got
        np.testing.assert_array_equal(got, base)


def test_single_row_subsets_are_nan(ops):
    """m = 1: the unbiased estimate divides by m (m - 1) = 0 - NaN on the device as in the reference"""
    import oracle
    from audio_metrics_amd.metrics.kd import kid_features_to_metric
    run_exact(ops, 1, 64, 4, kr.Kernel("poly", None, 1.0, 3), 0, 1500)
    run_exact(ops, 1, 100, 4, kr.Kernel("rbf", sigma=3.0), 1, 1501)
    run_exact(ops, 1, 17, 4, kr.Kernel("poly", None, 1.0, 3), None, 1502, xdtype=np.float64, ydtype=np.float64)
    rng = np.random.default_rng(1503)
    for n1, n2 in ((3, 2), (2, 3), (3, 3)):
        f1, f2 = kr.exact_rows(rng, n1, 64), kr.exact_rows(rng, n2, 64)
        got = kid_features_to_metric(dev(f1), dev(f2), kid_subsets=5)
        with np.errstate(divide="ignore", invalid="ignore"):
            want = oracle.kid_from_features(f1.astype(np.float64), f2.astype(np.float64), subsets=5)
        for key in want:
            assert np.isnan(want[key]) and np.isnan(got[key]), (key, got, want)


@pytest.mark.parametrize("poison", ["nan row", "inf element"])
@pytest.mark.parametrize("m,d,dtype", [(512, 128, np.float32), (600, 200, np.float32), (200, 64, np.float32),
                                       (300, 100, np.float32), (65, 17, np.float64)])
def test_non_finite_rows_stay_in_their_subsets(ops, poison, m, d, dtype):
    """a non-finite row makes exactly the subsets whose index list holds it non-finite; the others match the oracle"""
    rng = np.random.default_rng(1600 + m + d)
    n1, n2 = m + 50, m + 60
    x, y = kr.exact_rows(rng, n1, d).astype(dtype), kr.exact_rows(rng, n2, d).astype(dtype)
    r = n1 // 2
    if poison == "nan row":
        x[r] = np.nan
    else:
        x[r, d // 3] = np.inf
    i1, i2 = kr.index_tables(rng, n1, n2, 5, m)
    for s in range(5):                                   # subsets 0, 2, 4 hold row r, 1 and 3 do not
        row = i1[s]
        if s % 2 == 0 and r not in row:
            row[np.flatnonzero((row != 0) & (row != n1 - 1))[0]] = r      # (the first / last rows stay)
        if s % 2 == 1 and r in row:
            row[row == r] = np.setdiff1d(np.arange(n1), row)[0]
    holds = np.array([r in i1[s] for s in range(5)])
    assert holds.tolist() == [True, False, True, False, True]
    kernel = kr.Kernel("poly", None, 1.0, 3)
    xt, yt = dev(x), dev(y)
    if dtype == np.float32:
        assert route_of(ops, xt, yt, m, kernel) == expected_route(m, d)
    got = kd(ops, xt, yt, i1, i2, kernel)
    assert not np.isfinite(got[holds]).any(), got
    clean = ~holds
    check_exact(got[clean], x, y, i1[clean], i2[clean], kernel, poison)


# ---------------------------------------------------------------------------------------------------- (b) rounding

@pytest.mark.parametrize("name", [c[0] for c in kr.ROUNDING_CASES])
def test_rounding_at_real_shapes(ops, name):
    x, y, i1, i2, form, kernel = kr.rounding_case(name)
    want, _ = kr.subset_values(x, y, i1, i2, kernel)
    tol = kr.rounding_tolerance(kr.emulated_errors(x, y, i1, i2, form, kernel, want))
    xt, yt = dev(x), dev(y)
    route = expected_route(kr.ROUNDING_M, x.shape[1], kernel.degree, kernel.kind == "rbf")
    assert (route == 3) == (form == "split") and route_of(ops, xt, yt, kr.ROUNDING_M, kernel) == route
    got = kd(ops, xt, yt, i1, i2, kernel)
    err = np.abs(got - want)
    assert (err <= tol).all(), f"{name}: errors {err} over the limit {tol:.3g} (values {want})"


# ---------------------------------------------------------------------------------------------------- (c) 4 GiB

def test_exact_at_the_4gib_boundary(ops):
    """one f32 buffer a little over 2^32 bytes, filled on the device with integers in [-3, 3]: 2^24 - 1 rows of 64 sit
    256 B under the 32-bit buffer-offset limit (tile form, the last row's offset just below 2^32), 2^24 rows take the
    generic pointer form (poly and RBF), 10 737 419 rows of 100 the generic form with a tail, 2^23 rows of 128 the split
    form; every index table holds the last row.  The oracle fetches only the gathered rows."""
    numel = (1 << 30) + 1024
    g = torch.Generator(device=DEV)
    g.manual_seed(2024)
    big = torch.randint(-3, 4, (numel,), generator=g, device=DEV, dtype=torch.float32)
    try:
        cases = [((1 << 24) - 1, 64, 200, kr.Kernel("poly", None, 1.0, 3), 0),
                 ((1 << 24) - 1, 64, 200, kr.Kernel("rbf", sigma=16.0), 0),
                 (1 << 24, 64, 200, kr.Kernel("poly", 1e-3, -1.0, 3), 2),
                 (1 << 24, 64, 300, kr.Kernel("rbf", sigma=16.0), 2),
                 (10737419, 100, 200, kr.Kernel("poly", None, 2.5, 2), 2),
                 (1 << 23, 128, 600, kr.Kernel("poly", 1e-3, 0.0, 3), 3)]
        rng = np.random.default_rng(2025)
        for rows, d, m, kernel, route in cases:
            v = big[:rows * d].view(rows, d)
            assert ops.as_matrix(v).data_ptr() == v.data_ptr()
            assert route_of(ops, v, v, m, kernel) == route, (rows, d)
            i1, i2 = kr.index_tables(rng, rows, rows, 3, m)
            got = kd(ops, v, v, i1, i2, kernel)
            need = np.unique(np.concatenate([i1.ravel(), i2.ravel()]))
            host = v[torch.as_tensor(need, device=DEV)].cpu().numpy()
            j1, j2 = np.searchsorted(need, i1), np.searchsorted(need, i2)
            check_exact(got, host, host, j1, j2, kernel, f"{rows} x {d}")
    finally:
        del big
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- (d) entry points

@pytest.mark.parametrize("degree,gamma,coef0", [(3, 2.0 ** -9, -0.75), (2, 1e-3, 0.5)])
def test_fused_evaluate_equals_kd_poly_and_the_oracle(ops, degree, gamma, coef0):
    """am_evaluate_f32's KD (features_1 = candidate) with non-default gamma / coef0 / degree: bit for bit kd_poly, and the
    oracle - a swapped or dropped argument shows"""
    rng = np.random.default_rng(1700 + degree)
    m, d, n_ref, n_cand = 520, 200, 700, 650
    ref, cand = kr.exact_rows(rng, n_ref, d), kr.exact_rows(rng, n_cand, d)
    ic, ir = kr.index_tables(rng, n_cand, n_ref, 3, m)
    rt, ct = dev(ref), dev(cand)
    kernel = kr.Kernel("poly", gamma, coef0, degree)
    assert route_of(ops, ct, rt, m, kernel) == expected_route(m, d, degree)
    _, fused = ops.evaluate(rt, ct, ["kd"], idx_cand=dev(ic), idx_ref=dev(ir), gamma=gamma, coef0=coef0, degree=degree)
    direct = kd(ops, ct, rt, ic, ir, kernel)
    np.testing.assert_array_equal(fused, direct)
    check_exact(direct, cand, ref, ic, ir, kernel, "evaluate")


@pytest.mark.parametrize("n1,n2,d,kw", [(2100, 2000, 128, {}),
                                        (1200, 1100, 100, dict(kid_degree=2, kid_gamma=1e-3, kid_coef0=-1.0)),
                                        (900, 800, 64, dict(kernel_type="rbf", kid_sigma=16.0))])
def test_kid_features_to_metric_mean_and_std(ops, n1, n2, d, kw):
    import oracle
    from audio_metrics_amd.metrics.kd import kid_features_to_metric
    rng = np.random.default_rng(1800 + d)
    f1, f2 = kr.exact_rows(rng, n1, d, 0, 0), kr.exact_rows(rng, n2, d, 0, 0)
    S = 4
    got = kid_features_to_metric(dev(f1), dev(f2), kid_subsets=S, rng_seed=31, **kw)
    m = oracle.kd.effective_subset_size(n1, n2)
    i1, i2 = oracle.draw_subsets(n1, n2, S, 1000, 31)
    if kw.get("kernel_type") == "rbf":
        kernel = kr.Kernel("rbf", sigma=kw["kid_sigma"])
    else:
        kernel = kr.Kernel("poly", kw.get("kid_gamma"), kw.get("kid_coef0", 1.0), kw.get("kid_degree", 3))
    assert route_of(ops, dev(f1), dev(f2), m, kernel) == expected_route(m, d, kernel.degree, kernel.kind == "rbf")
    want, scale = kr.subset_values(f1, f2, i1, i2, kernel)
    tol = EXACT * scale.mean()
    assert abs(got["kernel_distance_mean"] - np.mean(want)) <= tol, (got, np.mean(want))
    assert abs(got["kernel_distance_std"] - np.std(want)) <= tol, (got, np.std(want))
