"""Per-group Frechet distance on the device (am_frechet_groups_f32 / _f64 and frechet_distance_per_group) against the SVD
oracle of fad_groups_reference.py.

Criterion: |fd - oracle| <= 1e-12 s and |tr_sqrt - oracle| <= 1e-12 s with s = |dmu|^2 + tr cov_x + tr cov_y.  The same
algorithm in numpy float64 lands at 7.4e-16 s; 1e-12 leaves three orders for another summation order and stays four
orders below the 4e-8 s that a missing eigenvalue threshold, or a D x D eigvals route, leaves behind.

One comparison carries another bound.  With the RANK-DEFICIENT reference (12 rows, D = 64) and candidate rows OUTSIDE the span
of the reference rows (randn), the device lands 6.5e-9 s from the SVD oracle (fd; 3.3e-9 s for tr_sqrt) - measured on an
MI355X.  The reason lies in the oracle: the float64 cov_y carries eigenvalues of +-eps |cov_y| in its 53 null directions,
sqrt_psd (eigh, clipped at 0) keeps the square roots of the positive ones, about 1e-8 each, and rows with components out
there pick them up.  The device does not: in M = Xc cov_y Xc^T that dust sits at 1e-16 lambda_max, below the eigenvalue
threshold.  Against an oracle without it - fad_groups_reference.factor_tr_sqrt, the singular values of Xc Yc^T from the
reference ROWS - the same records meet 1e-12 s, and that is asserted; against the SVD oracle this one comparison is held to
10 x the measurement, 6.5e-8 s.  Rows inside the span (drawn from the reference, mixtures of its rows) meet 1e-12 s against
the SVD oracle as every other case does."""
import numpy as np
import pytest
import torch

import fad_groups_reference as fr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-12
FAD_EXACT_REL = 1e-6                # the bar of stats_gather + frechet_batch (test_gpu_fad_inf.py)
SIZES = [1, 2, 3, 15, 16, 17, 64, 127, 128]
N_REF = 600
_CACHE = {}


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    audio_metrics_amd._lib.load()
    return audio_metrics_amd


def reference(d, n=N_REF):
    """seeded reference rows and their f64 statistics, on the host and on the device; computed once per width"""
    if (d, n) not in _CACHE:
        y = np.random.default_rng(1000 + d).standard_normal((n, d)) / np.sqrt(1.0 + 0.1 * np.arange(d))
        mu, cov = fr.reference_stats(y)
        _CACHE[d, n] = (y, mu, cov, torch.as_tensor(mu).to(DEV), torch.as_tensor(cov).to(DEV))
    return _CACHE[d, n]


def candidate_rows(kind, n, d, seed, y):
    rng = np.random.default_rng(seed)
    if kind == "randn":
        return rng.standard_normal((n, d)) * 1.3 + 0.2
    if kind == "unit":
        x = rng.standard_normal((n, d))
        return x / np.linalg.norm(x, axis=1, keepdims=True)
    assert kind == "ref"
    return y[rng.integers(0, len(y), n)].copy()


def run(am, x, idx, offsets, d, mu_dev=None, cov_dev=None):
    """records [B, 5] as numpy, after the deferred index check"""
    _, _, _, mu_d, cov_d = reference(d)
    out, check = am.hip_ops.frechet_groups(x, idx, offsets, mu_d if mu_dev is None else mu_dev, cov_d if cov_dev is None else cov_dev)
    rec = out.cpu().numpy()
    check()
    return rec


def assert_meets(rec, want, tol=TOL, what=""):
    err_fd = np.abs(rec[:, 0] - want["fd"]) / want["scale"]
    err_tr = np.abs(rec[:, 1] - want["tr_sqrt"]) / want["scale"]
    print(what, "fd err / s:", err_fd.max(), " tr_sqrt err / s:", err_tr.max(), " sweeps:", rec[:, 2].max())
    assert (rec[:, 4] == 1).all(), rec[:, 4]
    assert (rec[:, 2] <= 30).all() and (rec[:, 3] <= 2.0 ** -52).all(), rec[:, 2:4]
    assert (err_fd <= tol).all(), (what, err_fd)
    assert (err_tr <= tol).all(), (what, err_tr)


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64).tolist()


# ------------------------------------------------------------------ 1. every group size, both row types, three kinds of rows
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["randn", "unit", "ref"])
@pytest.mark.parametrize("d", [20, 64, 132])
def test_group_sizes(am, d, kind, dtype):
    y, mu, cov, _, _ = reference(d)
    offs = offsets_of(SIZES)
    rows = candidate_rows(kind, offs[-1], d, 7 * d, y).astype(dtype)
    perm = np.random.default_rng(d).permutation(offs[-1])                  # the groups lie scattered in the stored matrix
    stored = np.empty_like(rows)
    stored[perm] = rows
    rec = run(am, torch.as_tensor(stored).to(DEV), torch.as_tensor(perm).to(DEV), offs, d)
    assert_meets(rec, fr.groups_oracle(rows, offs, mu, cov), what=f"D={d} {kind} {np.dtype(dtype).name}")
    assert rec[0, 1] == 0.0 and rec[0, 2] == 0.0                            # one row: zero covariance, no sweep


# ------------------------------------------------------------------ 2. deflation: duplicate rows
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_duplicate_rows(am, dtype):
    d = 64
    y, mu, cov, _, _ = reference(d)
    a = candidate_rows("randn", 10, d, 5, y).astype(dtype)
    a[1] = a[0]
    a[2] = a[0]
    b = np.repeat(candidate_rows("randn", 1, d, 6, y).astype(dtype), 2, axis=0)
    rows, offs = np.concatenate([a, b]), [0, 10, 12]
    rec = run(am, torch.as_tensor(rows).to(DEV), None, offs, d)
    want = fr.groups_oracle(rows, offs, mu, cov)
    assert_meets(rec, want, what="duplicates")
    assert rec[1, 1] == 0.0 and rec[1, 2] == 0.0                            # M = 0 exactly: nothing to rotate
    assert want["fd"][1] == want["scale"][1]


# ------------------------------------------------------------------ 3. rank-deficient reference
def test_rank_deficient_reference(am):
    d = 64
    y, mu, cov, mu_d, cov_d = reference(d, 12)
    rng = np.random.default_rng(12)
    sizes = [5, 40, 100, 128]
    offs = offsets_of(sizes)
    drawn = candidate_rows("ref", offs[-1], d, 13, y)
    mixed = rng.dirichlet(np.ones(12), offs[-1]) @ y                        # convex mixtures: inside the span as well
    for name, rows in (("drawn", drawn), ("mixed", mixed)):
        rec = run(am, torch.as_tensor(rows).to(DEV), None, offs, d, mu_d, cov_d)
        assert_meets(rec, fr.groups_oracle(rows, offs, mu, cov), what="12-row reference, rows " + name)
    outside = candidate_rows("randn", offs[-1], d, 14, y)
    rec = run(am, torch.as_tensor(outside).to(DEV), None, offs, d, mu_d, cov_d)
    want = fr.groups_oracle(outside, offs, mu, cov)
    assert_meets(rec, want, tol=6.5e-8, what="12-row reference, rows outside its span, SVD oracle")
    clean = dict(want)                                                       # the same terms around a dust-free tr sqrt
    clean["tr_sqrt"] = np.array([fr.factor_tr_sqrt(outside[offs[g]:offs[g + 1]], y) for g in range(len(sizes))])
    clean["fd"] = want["fd"] + 2.0 * (want["tr_sqrt"] - clean["tr_sqrt"])
    assert_meets(rec, clean, what="12-row reference, rows outside its span, factor oracle")


# ------------------------------------------------------------------ 4. same bits: row types, repeated calls, index list, strides
def test_bit_identity(am):
    d = 20
    y, _, _, _, _ = reference(d)
    offs = offsets_of(SIZES)
    n = offs[-1]
    x32 = candidate_rows("randn", n, d, 21, y).astype(np.float32)
    t32, t64 = torch.as_tensor(x32).to(DEV), torch.as_tensor(x32.astype(np.float64)).to(DEV)
    base = run(am, t32, None, offs, d)
    assert (base[:, 4] == 1).all()
    same = lambda rec: np.array_equal(rec.view(np.int64), base.view(np.int64))
    assert same(run(am, t64, None, offs, d)), "float32 rows and the same values as float64 rows"
    assert same(run(am, t32, None, offs, d)), "the same call twice"
    assert same(run(am, t32, torch.arange(n, device=DEV), offs, d)), "idx = NULL against an explicit arange"
    wide32 = torch.full((n, d + 4), 7.0, dtype=torch.float32, device=DEV)
    wide32[:, :d] = t32
    assert wide32[:, :d].stride(0) == d + 4 and same(run(am, wide32[:, :d], None, offs, d)), "float32 view with ld > D"
    wide64 = torch.full((n, d + 3), 7.0, dtype=torch.float64, device=DEV)
    wide64[:, :d] = t64
    assert wide64[:, :d].stride(0) == d + 3 and same(run(am, wide64[:, :d], None, offs, d)), "float64 view with ld > D"


# ------------------------------------------------------------------ 5. an index outside the matrix
def test_bad_index_is_reported_and_isolated(am):
    d = 20
    y, _, _, mu_d, cov_d = reference(d)
    sizes = [5, 17, 33]
    offs = offsets_of(sizes)
    x = torch.as_tensor(candidate_rows("randn", 80, d, 31, y).astype(np.float32)).to(DEV)
    idx = torch.as_tensor(np.random.default_rng(3).permutation(80)[:offs[-1]]).to(DEV)
    clean = run(am, x, idx, offs, d)
    for bad_value in (80, -1, 1 << 40):
        bad = idx.clone()
        bad[9] = bad_value                                                   # position 9 lies in group 1
        out, check = am.hip_ops.frechet_groups(x, bad, offs, mu_d, cov_d)
        rec = out.cpu().numpy()
        with pytest.raises(ValueError, match=r"idx\[9\] = %d is outside \[0, 80\)" % bad_value):
            check()
        for g in (0, 2):
            assert np.array_equal(rec[g].view(np.int64), clean[g].view(np.int64)), g


# ------------------------------------------------------------------ 6. a group's record does not depend on its neighbours
def test_groups_are_independent(am):
    d, b, per = 20, 300, 5
    y, mu, cov, _, _ = reference(d)
    rows = candidate_rows("randn", b * per, d, 41, y).astype(np.float32)
    x = torch.as_tensor(rows).to(DEV)
    offs = offsets_of([per] * b)
    rec = run(am, x, None, offs, d)
    assert_meets(rec, fr.groups_oracle(rows, offs, mu, cov), what="300 groups of 5")
    for g in (0, 1, 150, 299):
        alone = run(am, x[g * per:(g + 1) * per], None, [0, per], d)
        assert np.array_equal(alone[0].view(np.int64), rec[g].view(np.int64)), g


# ------------------------------------------------------------------ 7. the front end: routes, labels, stop codes
def host_stats(am, mu, cov, n=N_REF):
    s = am.AudioMetricsData(False)
    s.n, s.mean, s.cov = n, torch.as_tensor(mu), torch.as_tensor(cov)
    return s


def stored(am, rows):
    s = am.AudioMetricsData(True)
    s.add(torch.as_tensor(rows).to(DEV))
    return s


def test_routes(am):
    from audio_metrics_amd.metrics import fad
    d = 64
    y, mu, cov, _, _ = reference(d)
    rows = candidate_rows("randn", 129 + 128, d, 51, y)                      # float64 rows: both routes entirely in f64
    labels = np.array([4] * 129 + [9] * 128)
    mix = np.random.default_rng(5).permutation(len(rows))
    res = am.frechet_distance_per_group(stored(am, rows[mix]), host_stats(am, mu, cov), labels[mix])
    assert res["group_labels"].tolist() == [4, 9] and res["group_sizes"].tolist() == [129, 128]
    assert res["fad_per_group"].dtype == np.float64 and res["group_sizes"].dtype == np.int64
    assert fad.last_info["routes"] == ["batch", "dual"] and fad.last_info["stops"][1] == 1
    assert fad.last_info["sweeps"][0] is None and fad.last_info["iters"][0] >= 1 and fad.last_info["iters"][1] is None
    big, small = fr.group_oracle(rows[:129], mu, cov), fr.group_oracle(rows[129:], mu, cov)
    print("batch route rel err:", abs(res["fad_per_group"][0] - big["fd"]) / big["fd"],
          " dual route err / s:", abs(res["fad_per_group"][1] - small["fd"]) / small["scale"])
    assert abs(res["fad_per_group"][0] - big["fd"]) <= FAD_EXACT_REL * abs(big["fd"])
    assert abs(res["fad_per_group"][1] - small["fd"]) <= TOL * small["scale"]


def test_labels(am):
    d = 20
    y, mu, cov, _, _ = reference(d)
    rows = candidate_rows("randn", 36, d, 61, y).astype(np.float32)
    labels = np.array([7, -3, 10 ** 9] * 10 + [7] * 6)
    ref = host_stats(am, mu, cov)
    for as_torch in (False, True):
        res = am.frechet_distance_per_group(stored(am, rows), ref, torch.as_tensor(labels) if as_torch else labels)
        assert res["group_labels"].tolist() == [-3, 7, 10 ** 9] and res["group_sizes"].tolist() == [10, 16, 10]
        for g, lab in enumerate(res["group_labels"]):
            own = rows[labels == lab]
            alone = am.frechet_distance_per_group(stored(am, own), ref, np.zeros(len(own), dtype=np.int32))
            assert alone["fad_per_group"][0] == res["fad_per_group"][g], lab
            want = fr.group_oracle(own, mu, cov)
            assert abs(res["fad_per_group"][g] - want["fd"]) <= TOL * want["scale"]


def test_non_finite_group_is_named(am):
    d = 20
    y, mu, cov, mu_d, cov_d = reference(d)
    rows = candidate_rows("randn", 12, d, 71, y).astype(np.float32)
    rows[7, 3] = np.nan
    rec = run(am, torch.as_tensor(rows).to(DEV), None, [0, 6, 12], d)
    assert rec[0, 4] == 1 and rec[1, 4] == 4
    with pytest.raises(am._lib.HipLibraryError, match="label 55 .*dual route.*stop code 4"):
        am.frechet_distance_per_group(stored(am, rows), host_stats(am, mu, cov), [11] * 6 + [55] * 6)
    # the batched route names the label too (not a set index within its chunk), and the dual-route group beside it is fine
    big = candidate_rows("randn", 129 + 6, d, 72, y).astype(np.float32)
    big[40, 0] = np.inf
    from audio_metrics_amd.metrics import fad
    with pytest.raises(am._lib.HipLibraryError, match="label -8 .*129 rows, batch route.*stop code"):
        am.frechet_distance_per_group(stored(am, big), host_stats(am, mu, cov), [-8] * 129 + [3] * 6)
    assert fad.last_info["routes"] == ["batch", "dual"] and fad.last_info["stops"][1] == 1
    assert fad.last_info["sweeps"][0] is None and fad.last_info["iters"][1] is None and fad.last_info["sweeps"][1] >= 1
