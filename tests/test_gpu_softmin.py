"""The soft-min on the device (hip_ops.softmin, csrc/softmin.hip) against the float64 oracle of tests/sinkhorn_reference.py.

  1  every shape x {zero, seeded potentials} x {bounding-box, median, 0.01 x median temperature} within the derived bound
     delta(eps) = 2^-24 (D + 16) (max |x|^2 + max |y|^2 + max |g|) + 2^-21 eps; the largest observed error / delta goes to
     profiles/sinkhorn/accuracy.txt
  2  the hard-min limit: at a temperature a hundredth of every row's gap the result is the search's smallest squared
     distance / 2 + eps log M - the maximum's merge across lanes and chunks against the search's bits
  3  a temperature at which every term but the largest underflows;  4  padded views;  5  damping, change and magnitude;
  6  determinism.

The shapes are the smallest that cross the edges: one row, 128 +- 1 rows, a partial third column tile, D with and without
the inner-dimension tail, a set against itself, and 32 column chunks."""
import math

import numpy as np
import pytest
import torch

import sinkhorn_reference as sr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 1, 1), (127, 129, 33), (130, 300, 40), (130, 300, 64), (257, 130, 96), (130, 130, 64), (130, 4000, 40)]
SELF = (130, 130, 64)                                # x is y
WORST = {}                                           # case -> largest error / delta


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    audio_metrics_amd._lib.load()
    return audio_metrics_amd


@pytest.fixture(scope="module")
def ops(am):
    return am.hip_ops


@pytest.fixture(scope="module", autouse=True)
def accuracy_record():
    yield
    if WORST:
        sr.record_accuracy("one soft-min: largest |device - oracle| / delta(eps) per shape (bound: 1)",
                           [f"{case}: {ratio:.4f}" for case, ratio in WORST.items()])


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def randn(seed, n, d):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def sets(shape, seed=11):
    n, m, d = shape
    x = randn(seed, n, d)
    y = x if shape == SELF else randn(seed + 1, m, d) + np.float32(0.25)
    return x, y


def padded(a, extra, fill):
    """The same rows as a view of a wider buffer whose padding must never be read as data."""
    buf = torch.full((a.shape[0], a.shape[1] + extra), fill, dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = dev(a)
    view = buf[:, :a.shape[1]]
    assert view.stride(0) == a.shape[1] + extra
    return view


def run(ops, x, y, g, eps, **kw):
    out, change, magnitude = ops.softmin(x, y, None if g is None else dev(g), eps=eps, **kw)
    assert out.dtype == change.dtype == magnitude.dtype == torch.float64 and out.is_cuda and change.is_cuda and magnitude.is_cuda
    assert tuple(out.shape) == (x.shape[0],) and change.dim() == 0 and magnitude.dim() == 0
    return out.cpu().numpy(), float(change), float(magnitude)


def bound(x, y, g, eps):
    gmax = 0.0 if g is None else float(np.abs(g).max())
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    return sr.delta(eps, x.shape[1], float((x64 * x64).sum(1).max()), float((y64 * y64).sum(1).max()), gmax)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_the_oracle_within_the_derived_bound(ops, shape):
    n, m, d = shape
    x, y = sets(shape)
    if shape == (130, 4000, 40):
        assert ops.knn_search_chunks(130, 4000, 40, 1) == 32               # the cross-chunk merge
    cost = sr.half_sq_dists(x, y)
    median = float(np.median(cost))
    temperatures = {"diam2": sr.diam2(x, y), "median": median, "0.01 median": 0.01 * median}
    if shape == (1, 1, 1):
        temperatures = {"diam2": max(sr.diam2(x, y), 1e-3), "median": max(median, 1e-3), "0.01 median": max(0.01 * median, 1e-5)}
    dx = dev(x)
    dy = dx if shape == SELF else dev(y)
    potentials = {"zero": None, "seeded": np.random.default_rng(5).standard_normal(m) * median}
    worst = 0.0
    for gname, g in potentials.items():
        for tname, eps in temperatures.items():
            got, change, magnitude = run(ops, dx, dy, g, eps)
            want = sr.softmin(cost, np.zeros(m) if g is None else g, eps)
            err, lim = float(np.abs(got - want).max()), bound(x, y, g, eps)
            print(f"{shape} g={gname} eps={tname}={eps:.4g}: error {err:.3e}, delta {lim:.3e}, ratio {err / lim:.4f}")
            worst = max(worst, err / lim)
            assert np.isfinite(got).all()
            assert err <= lim, (shape, gname, tname, err, lim)
            assert change == magnitude == float(np.abs(got).max())           # no prev: both are max |out|
    WORST["x".join(map(str, shape))] = worst


@pytest.mark.parametrize("shape", [(257, 130, 96), (130, 4000, 40)], ids=lambda s: "x".join(map(str, s)))
def test_hard_min_limit_has_the_bits_of_the_search(ops, shape):
    n, m, d = shape
    x, y = sets(shape)
    dx, dy = dev(x), dev(y)
    d2 = ops.knn_search(dx, dy, 2, squared=True)[0].cpu().numpy().astype(np.float64)
    gap = 0.5 * (d2[:, 1] - d2[:, 0])
    assert gap.min() > 0
    eps = float(gap.min()) / 128.0
    assert (gap / eps >= 100.0).all()
    got, _, _ = run(ops, dx, dy, None, eps)
    want = 0.5 * d2[:, 0] + eps * math.log(m)
    rel = np.abs(got - want) / want
    print(shape, "eps", eps, "largest relative difference", rel.max(), "bound", 2.0 ** -22)
    assert rel.max() <= 2.0 ** -22


def test_every_term_but_the_largest_underflows(ops):
    shape = (130, 300, 40)
    x, y = sets(shape)
    cost = sr.half_sq_dists(x, y)
    part = np.partition(cost, 1, axis=1)
    eps = float((part[:, 1] - part[:, 0]).min()) / 2000.0                  # exp(-2000) = 0 in f64 as in f32
    assert eps > 0 and math.exp(-(part[:, 1] - part[:, 0]).min() / eps) == 0.0
    got, change, magnitude = run(ops, dev(x), dev(y), None, eps)
    assert np.isfinite(got).all() and math.isfinite(change) and math.isfinite(magnitude)
    want = sr.softmin(cost, np.zeros(shape[1]), eps)
    assert np.abs(got - want).max() <= bound(x, y, None, eps)
    assert np.allclose(want, cost.min(axis=1) + eps * math.log(shape[1]), rtol=1e-12)


@pytest.mark.parametrize("shape", [(130, 300, 40), (127, 129, 33)], ids=lambda s: "x".join(map(str, s)))
def test_padded_views_read_no_padding(ops, shape):
    x, y = sets(shape)
    g = np.random.default_rng(6).standard_normal(shape[1]) * 10.0
    eps = float(np.median(sr.half_sq_dists(x, y)))
    plain = run(ops, dev(x), dev(y), g, eps)
    for fill in (math.nan, 1e30):
        wide = run(ops, padded(x, 4 + (-x.shape[1]) % 4, fill), padded(y, 8 + (-y.shape[1]) % 4, fill), g, eps)
        assert np.array_equal(wide[0], plain[0]) and wide[1:] == plain[1:]


def test_damping_change_and_magnitude(ops):
    shape = (130, 300, 40)
    x, y = sets(shape)
    rng = np.random.default_rng(7)
    g, prev = rng.standard_normal(shape[1]) * 10.0, rng.standard_normal(shape[0]) * 10.0
    eps = 5.0
    dx, dy, dprev = dev(x), dev(y), dev(prev)
    plain, _, _ = run(ops, dx, dy, g, eps)
    # damping 0 with prev: the soft-min itself, and the change against prev
    got, change, magnitude = run(ops, dx, dy, g, eps, prev=dprev)
    assert np.array_equal(got, plain)
    assert change == float(np.abs(plain - prev).max()) and magnitude == float(np.abs(plain).max())
    # damping 0.5: the averaged step, in the kernel's own order of operations
    got, change, magnitude = run(ops, dx, dy, g, eps, prev=dprev, damping=0.5)
    want = 0.5 * prev + (1.0 - 0.5) * plain
    assert np.array_equal(got, want)
    assert change == float(np.abs(want - prev).max()) and magnitude == float(np.abs(want).max())
    got, change, _ = run(ops, dx, dy, g, eps, prev=dprev, damping=0.25)
    assert np.allclose(got, 0.25 * prev + 0.75 * plain, rtol=1e-15, atol=0)
    # out may be prev's successor in a loop: prev itself is left alone
    assert np.array_equal(dprev.cpu().numpy(), prev)


@pytest.mark.parametrize("shape", [(130, 4000, 40), SELF], ids=lambda s: "x".join(map(str, s)))
def test_two_calls_give_the_same_bits(ops, shape):
    x, y = sets(shape)
    dx = dev(x)
    dy = dx if shape == SELF else dev(y)
    g = np.random.default_rng(8).standard_normal(shape[1]) * 20.0
    prev = dev(np.random.default_rng(9).standard_normal(shape[0]))
    for eps in (40.0, 0.3):
        a = run(ops, dx, dy, g, eps, prev=prev, damping=0.5)
        b = run(ops, dx, dy, g, eps, prev=prev, damping=0.5)
        assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and a[1:] == b[1:]
    if shape == SELF:                                                      # shared norms or not: the same bits
        a = run(ops, dx, dx, g, 40.0)
        b = run(ops, dx, dev(x), g, 40.0)
        assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))
