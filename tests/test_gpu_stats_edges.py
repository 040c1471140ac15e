"""The f32 statistics (stats.hip: am_stats_f32, am_colsum_f32, am_scatter_f32, am_stats_merge_f64) and the f64 route at the
edges of their tiles, against numpy float64 on the same f32 values.

    D < 128              scatter_small_kernel (products summed in f64): one 32-column block at D = 1 .. 32 (31, 32: all four
                         accumulator slots), a second block of width 1 and 2 at D = 33, 34, whole blocks at D = 64, 96, four
                         blocks with a ragged last one at D = 127
    D = 128              the unmasked MFMA kernel, and the other side of the 127 / 128 switch
    D = 129, 131, 257    several 128-wide tiles with a ragged last one: the column masks of the FULLD == false kernel on
                         a mirrored off-diagonal tile
    N = 255 .. 257       the 256-row flush of the f32 chains; N = 31 .. 33, 511 .. 513, 1025, 2049: ragged last stages and
                         slabs (the narrow kernel stages 64 rows per step)
The covariance is compared element by element, |got - want|_ij <= STATS_F32_ELEM sqrt(want_ii want_jj), so one wrong strip
or mirrored element cannot hide in a norm; STATS_F32_ELEM comes from test_frechet_reference_cpu.py, which ties it to a
numpy transcription of the documented arithmetic on these very inputs."""
import functools

import numpy as np
import pytest
import torch

import frechet_reference as fr
from test_frechet_reference_cpu import STATS_F32_ELEM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COLSUM_D = [1, 5, 129, 257]
MERGE_D = [1, 255, 257, 513]
MERGE_N = [(1, 1), (1, 40), (40, 1), (300, 500)]
EPS64 = 2.0 ** -52


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    audio_metrics_amd._lib.load()
    return audio_metrics_amd


def to_dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def case(n, d, seed=0):
    """(x f32, f64 mean, f64 covariance) - computed once, shared by the tests of a shape, never modified"""
    x = fr.stats_input(n, d, seed)
    return x, x.astype(np.float64).mean(0), fr.cov_f64(x)


def check_cov(tag, mean, cov, want_mean, want_cov):
    got_mean, got_cov = mean.cpu().numpy(), cov.cpu().numpy()
    rel = fr.elem_rel(got_cov, want_cov)
    tr_rel = abs(np.trace(got_cov) - np.trace(want_cov)) / np.trace(want_cov)
    print(f"{tag}: mean err {np.abs(got_mean - want_mean).max():.2e}  cov elem {rel:.3e} = {rel * 2 ** 24:.1f} x 2^-24 "
          f"(bound {STATS_F32_ELEM:.1e})  trace rel {tr_rel:.2e}")
    np.testing.assert_allclose(got_mean, want_mean, rtol=0, atol=1e-12)
    assert rel <= STATS_F32_ELEM
    assert torch.equal(cov, cov.T)
    return tr_rel


# ------------------------------------------------------------------ am_stats_f32
@pytest.mark.parametrize("d", fr.STATS_D)
@pytest.mark.parametrize("n", fr.STATS_N)
def test_stats_at_tile_and_flush_edges(am, n, d):
    x, want_mean, want_cov = case(n, d)
    mean, cov = am.hip_ops.stats(to_dev(x))
    tr_rel = check_cov(f"stats N={n} D={d}", mean, cov, want_mean, want_cov)
    if n >= 32:
        assert tr_rel <= 1e-7                # the bar the suite holds am_stats_f32 to, at every width of the grid


@pytest.mark.parametrize("d", [1, 5, 129])
def test_one_row_gives_its_own_values_and_a_zero_covariance(am, d):
    x = fr.stats_input(1, d)
    mean, cov = am.hip_ops.stats(to_dev(x))
    assert np.array_equal(mean.cpu().numpy(), x[0].astype(np.float64))
    assert tuple(cov.shape) == (d, d) and not cov.any()


@pytest.mark.parametrize("pad", ["2d", "to4"])
@pytest.mark.parametrize("d", [5, 33, 129])
@pytest.mark.parametrize("n", [33, 513])
def test_row_strided_view_with_other_data_beyond_d(am, n, d, pad):
    """big[:, :D] with 1e6 in the columns past D: a column mask that let one of them through would be seen at once.  A
    2 D-wide parent has a row stride that is no multiple of 4 floats, which the glue repacks; a parent whose width is D
    rounded up past the next multiple of 4 reaches the kernel as it is (ld > D, foreign data in the row's tail)."""
    x, want_mean, want_cov = case(n, d)
    width = 2 * d if pad == "2d" else (d + 4) // 4 * 4 + 4
    big = torch.full((n, width), 1e6, dtype=torch.float32, device=DEV)
    big[:, :d] = to_dev(x)
    view = big[:, :d]
    passed = am.hip_ops.as_matrix(view)
    if pad == "to4":
        assert passed.data_ptr() == view.data_ptr() and passed.stride(0) == width > d
    mean, cov = am.hip_ops.stats(view)
    tr_rel = check_cov(f"view N={n} D={d} ld={width}", mean, cov, want_mean, want_cov)
    assert tr_rel <= 1e-7
    got = am.hip_ops.colsum(view).cpu().numpy()
    err = np.abs(got.astype(np.longdouble) - x.astype(np.longdouble).sum(0)).astype(np.float64)
    assert np.all(err <= n * 2.0 ** -53 * np.abs(x).astype(np.float64).sum(0))
    sc = am.hip_ops.scatter(view, to_dev(want_mean))
    assert fr.elem_rel(sc.cpu().numpy(), want_cov * (n - 1)) <= STATS_F32_ELEM
    assert torch.equal(big[:, d:], torch.full((n, width - d), 1e6, dtype=torch.float32, device=DEV))


# ------------------------------------------------------------------ am_colsum_f32
@pytest.mark.parametrize("d", COLSUM_D)
@pytest.mark.parametrize("n", fr.STATS_N)
def test_colsum_within_the_recursive_summation_bound(am, n, d):
    x, _, _ = case(n, d)
    got = am.hip_ops.colsum(to_dev(x)).cpu().numpy()
    want = x.astype(np.longdouble).sum(0)
    bound = n * 2.0 ** -53 * np.abs(x).astype(np.float64).sum(0)        # holds for any order of the N - 1 additions
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    print(f"colsum N={n} D={d}: max err / bound {float((err / bound).max()):.3f}")
    assert got.shape == (d,) and np.all(err <= bound)


# ------------------------------------------------------------------ am_scatter_f32
@pytest.mark.parametrize("whose", ["own", "foreign"])
@pytest.mark.parametrize("d", fr.SCATTER_D)
@pytest.mark.parametrize("n", fr.SCATTER_N)
def test_scatter_about_its_own_and_a_foreign_mean(am, n, d, whose):
    """foreign: the mean of a superset twice as long, as a rank of a row-sharded set centres its rows on the global mean"""
    big, big_mean, _ = case(2 * n, d, 1)
    x = big[:n]
    mean = big_mean if whose == "foreign" else x.astype(np.float64).mean(0)
    want = fr.scatter_f64(x, mean)
    got = am.hip_ops.scatter(to_dev(x), to_dev(mean))
    rel = fr.elem_rel(got.cpu().numpy(), want)
    print(f"scatter N={n} D={d} {whose} mean: elem {rel:.3e} = {rel * 2 ** 24:.1f} x 2^-24 (bound {STATS_F32_ELEM:.1e})")
    assert rel <= STATS_F32_ELEM
    assert torch.equal(got, got.T)


# ------------------------------------------------------------------ am_stats_merge_f64
def piece_stats(rows):
    return rows.mean(0), fr.cov_f64(rows)


@pytest.mark.parametrize("n1, n2", MERGE_N)
@pytest.mark.parametrize("d", MERGE_D)
def test_merge_against_the_formula_in_its_association_order(am, d, n1, n2):
    rng = np.random.default_rng([d, n1, n2])
    rows = rng.standard_normal((n1 + n2, d)) * (0.5 + rng.random(d)) + rng.standard_normal(d)
    (m1, c1), (m2, c2) = piece_stats(rows[:n1]), piece_stats(rows[n1:])
    assert (n1 > 1 or not c1.any()) and (n2 > 1 or not c2.any())          # a one-row side carries a zero covariance
    want_mean, want_cov, terms = fr.merge_f64(n1, m1, c1, n2, m2, c2)
    t = [to_dev(a) for a in (m1, c1, m2, c2)]
    mean, cov = am.hip_ops.stats_merge(n1, t[0], t[1], n2, t[2], t[3])
    assert mean.data_ptr() != t[0].data_ptr() and cov.data_ptr() != t[1].data_ptr()
    assert np.array_equal(t[0].cpu().numpy(), m1) and np.array_equal(t[1].cpu().numpy(), c1)      # inputs untouched
    err = np.abs(cov.cpu().numpy() - want_cov)
    mean_terms = (np.abs(n1 * m1) + np.abs(n2 * m2)) / (n1 + n2)
    print(f"merge D={d} n={n1}+{n2}: cov err / terms {float((err / np.maximum(terms, 1e-300)).max()) / EPS64:.2f} eps")
    assert np.all(err <= 4 * EPS64 * terms)
    assert np.all(np.abs(mean.cpu().numpy() - want_mean) <= 4 * EPS64 * mean_terms)
    m_in, c_in = t[0].clone(), t[1].clone()
    mean2, cov2 = am.hip_ops.stats_merge(n1, m_in, c_in, n2, t[2], t[3], inplace=True)
    assert mean2.data_ptr() == m_in.data_ptr() and cov2.data_ptr() == c_in.data_ptr()
    assert torch.equal(m_in, mean) and torch.equal(c_in, cov)            # same bits, written into the tensors given
    if n1 + n2 > 2:
        full = fr.cov_f64(rows)
        assert np.abs(cov.cpu().numpy() - full).max() <= 1e-12 * np.abs(full).max()


@pytest.mark.parametrize("d", MERGE_D)
def test_chained_merges_of_three_pieces(am, d):
    rng = np.random.default_rng([d, 3])
    rows = rng.standard_normal((151, d)) * (0.5 + rng.random(d)) + rng.standard_normal(d)
    cuts = [(0, 60), (60, 61), (61, 151)]
    n, mean, cov = 0, None, None
    for lo, hi in cuts:
        m, c = (to_dev(a) for a in piece_stats(rows[lo:hi]))
        if n == 0:
            mean, cov = m, c
        else:
            mean, cov = am.hip_ops.stats_merge(n, mean, cov, hi - lo, m, c, inplace=(hi - lo == 1))
        n += hi - lo
    want = fr.cov_f64(rows)
    assert np.abs(mean.cpu().numpy() - rows.mean(0)).max() <= 1e-13
    assert np.abs(cov.cpu().numpy() - want).max() <= 1e-12 * np.abs(want).max()


# ------------------------------------------------------------------ the f64 route at the new widths
@pytest.mark.parametrize("n, d", [(257, 129), (513, 131), (33, 257)])
def test_float64_route_at_the_new_widths(am, n, d):
    rng = np.random.default_rng([n, d, 64])
    x = rng.standard_normal((n, d)) * 1.3 + 0.2 + 1e-9 * rng.standard_normal((n, d))      # (not representable in f32)
    mean, cov = am.hip_ops.stats_f64(to_dev(x))
    want_mean, want_cov = x.mean(0), fr.cov_f64(x)
    assert np.abs(mean.cpu().numpy() - want_mean).max() <= 1e-13 * max(1.0, np.abs(want_mean).max())
    assert np.abs(cov.cpu().numpy() - want_cov).max() <= 1e-12 * np.abs(want_cov).max()
    assert torch.equal(cov, cov.T)
