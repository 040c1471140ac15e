"""What the seven row-sweep entry points share (csrc/row_sweep.h) at the shapes where it can go wrong.

  1  the same-set path of the norms helper: a call with y the very tensor x (one set of norms) returns the bits of a call
     with y a clone of x - two row blocks with an inner-dimension tail (130 x 40), three without (257 x 64);
  2  the four-lane join and the lane geometry: N = 129 rows (a second row block of one row) against M = 257 columns at
     D = 40, every entry point against its own file's oracle and bound, and the rows at the corners of the (wn, nt, r) map
     - 0, 31, 32, 63, 64, 127, 128 - one by one: a wrong join slot or row index gives plausible numbers for the wrong row.

Oracles and bounds are those of the per-file tests (tests/*_reference.py, the exact integer oracle of
tests/test_gpu_knn_search.py); each is computed once."""
import numpy as np
import pytest
import torch

import fidelity_reference as fid
import kmeans_reference as kr
import psr_reference as pr
import sinkhorn_reference as sr
import test_gpu_fld as tfld
import test_gpu_knn_search as tks
import test_gpu_softmin as tsm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, M, D = 129, 257, 40
CORNERS = (0, 31, 32, 63, 64, 127, 128)
SAME_SET = [(130, 40), (257, 64)]


@pytest.fixture(scope="module")
def ops():
    import audio_metrics_amd
    audio_metrics_amd._lib.load()
    return audio_metrics_amd.hip_ops


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(out):
    return [t.cpu().numpy() for t in out if t is not None]


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---------------------------------------------------------------------------------------------------- 1. the same-set path
@pytest.mark.parametrize("n,d", SAME_SET)
def test_a_set_against_itself_has_the_bits_of_a_set_against_its_copy(ops, n, d):
    x = dev(np.random.default_rng(n + d).standard_normal((n, d)).astype(np.float32))
    y = x.clone()
    assert y.data_ptr() != x.data_ptr()
    radii = ops.knn_radii(x, 5)
    radius = 1.2 * float(radii.to(torch.float64).mean())
    eps = float(np.median(sr.half_sq_dists(x.cpu().numpy(), x.cpu().numpy())))
    calls = {
        "knn_search": lambda other: ops.knn_search(x, other, 5, self_offset=-1),
        "sample_scores": lambda other: ops.sample_scores(x, other, radii),
        "softmin": lambda other: ops.softmin(x, other, None, eps=eps),
        "psr": lambda other: ops.psr_scores(x, other, radius),
    }
    for name, call in calls.items():
        same, copy = host(call(x)), host(call(y))
        assert len(same) == len(copy) >= 2
        for s, c in zip(same, copy):
            assert s.dtype == c.dtype and np.array_equal(raw(s), raw(c)), name
    assert np.array_equal(host(calls["knn_search"](x))[1][:, 0], np.arange(n))       # no exclusion: a row finds itself first


# ---------------------------------------------------------------------------------------------------- 2. the join
def check_rows(ok, what):
    """`ok`: per-row verdict [N] (or [N, ...]); every row, and the corner rows named one by one."""
    ok = np.asarray(ok).reshape(N, -1).all(1)
    for i in CORNERS:
        assert ok[i], (what, "row", i)
    assert ok.all(), (what, np.flatnonzero(~ok)[:8])


@pytest.fixture(scope="module")
def integer_case():
    x, y = tks.int_rows(41, N, D), tks.int_rows(42, M, D)
    d2, order = tks.int_oracle(x, y)
    assert d2.max() < 2 ** 24
    return x, y, d2, order


def test_knn_search_join(ops, integer_case):
    x, y, d2, order = integer_case
    got_d, got_i = tks.search(ops, dev(x), dev(y), 5, squared=True)
    tks.check_exact(got_d, got_i, d2, order, 5)
    want_i = order[:, :5]
    want_d = np.take_along_axis(d2, want_i, axis=1).astype(np.float32)
    check_rows((got_i == want_i) & (tks.bits(got_d) == tks.bits(want_d)), "knn_search")


def test_kmeans_assign_join(ops):
    x, c = kr.int_rows(41, N, D), kr.int_rows(42, M, D)
    c[150:200] = c[20:70]                                                  # duplicated centroids, in another column tile
    c[256] = c[0]
    d2 = kr.sq_distances(x, c)                                             # small integers: exact in f64 and in f32
    want, best, _, total = kr.assign(x, c)                                 # the first minimum: ties go to the smallest centroid
    assert d2.max() < 2 ** 24 and sum((row == row.min()).sum() > 1 for row in d2) > 10            # the data does tie
    labels, got, inertia = host(ops.kmeans_assign(dev(x), dev(c)))
    check_rows((labels == want) & (tks.bits(got) == tks.bits(best.astype(np.float32))), "kmeans_assign")
    assert float(inertia) == total                                         # integers: exact in every order


def test_sample_scores_join(ops):
    case = fid.lattice_oracle(N, M, D, 5, False)
    fid.check_lattice_is_not_degenerate(case, False)
    got = host(ops.sample_scores(dev(case["x"]), dev(case["y"]), dev(case["r"])))
    same = [raw(g).reshape(N, -1) == raw(np.asarray(w, dtype=g.dtype)).reshape(N, -1) for g, w in zip(got, case["want"])]
    assert len(same) == 5
    check_rows(np.concatenate(same, axis=1), "sample_scores")


def test_softmin_join(ops):
    x, y = tsm.sets((N, M, D))
    cost = sr.half_sq_dists(x, y)
    eps = float(np.median(cost))
    g = np.random.default_rng(5).standard_normal(M) * eps
    got, _, _ = tsm.run(ops, dev(x), dev(y), g, eps)
    want = sr.softmin(cost, g, eps)
    assert np.isfinite(got).all()
    check_rows(np.abs(got - want) <= tsm.bound(x, y, g, eps), "softmin")


def test_psr_join(ops):
    x, y = pr.latent_pair(N, M, D)
    xt, yt = dev(x), dev(y)
    R = 1.2 * float(ops.knn_radii(yt, 4).to(torch.float64).mean())
    psr, count, _ = host(ops.psr_scores(xt, yt, R))
    psr64, _, dist = pr.psr_f64(x, y, R)
    delta = pr.d2_delta(x, y)
    sure, maybe = ((dist * dist) < R * R - delta).sum(1), ((dist * dist) <= R * R + delta).sum(1)
    assert 0 < count.sum() and (count == 0).sum() < N
    check_rows((np.abs(psr - psr64) <= pr.error_bound(x, y, dist, R)) & (sure <= count) & (count <= maybe), "psr")


def test_fld_loglik_join(ops):
    c = tfld.case((N, M, D))
    ll, stats = tfld.loglik_on_device(ops, dev(c["x"]), dev(c["g"]), c["theta"])
    got, st = ll.cpu().numpy(), stats.cpu().numpy()
    assert np.isfinite(got).all() and st[1] == N and st[2] == 0
    check_rows(np.abs(got - c["loglik"]) <= c["delta"], "fld_loglik")


def test_fld_grad_join(ops):
    # the swapped sweep: the N = 129 rows of the join are the centres, the 257 evaluated rows are its columns
    c = tfld.case((M, N, D))
    dx, dg = dev(c["x"]), dev(c["g"])
    ll, stats = tfld.loglik_on_device(ops, dx, dg, c["theta"])
    _, _, _, a, b = tfld.grad_on_device(ops, dg, dx, c["theta"], ll, stats)
    # the limits of tests/test_gpu_fld.py (test_loglik_and_gradient_sums_within_the_derived_bounds), which has them inline
    big = float(c["delta"].max())
    h = 0.5 * np.exp(-c["theta"])
    lim_a = 2.0 * big * c["a"] + 1e-300
    lim_b = 2.0 * big * h * c["b"] + 2.0 ** -24 * (D + 16) * c["norms"] * h * c["a"] + 1e-300
    assert np.isfinite(a).all() and np.isfinite(b).all() and abs(a.sum() - M) <= 1e-9 * M
    check_rows((np.abs(a - c["a"]) <= lim_a) & (np.abs(h * (b - c["b"])) <= lim_b), "fld_grad")
