"""The sliced Wasserstein distance on the device against the float64 oracle of tests/swd_reference.py.

  1  projection against an f64 matmul of the same float32 rows and directions: every element within
     (D + 16) 2^-24 |x_i| |theta_l| (D products and D - 1 sums of an f32 chain, rounded inputs excluded: they are the same);
     padded row strides with poisoned padding; a projection's bits alone and among 129 others
  2  sort: exactly numpy's order on every input class, at row lengths around the wave (64), the workgroup (1024) and the
     segment sizes, with a padded row stride; bit patterns (every digit of every pass, NaNs, +-0, +-inf, denormals)
     against the sorted keys of the order-preserving transform
  3  merge: W_p^p of device-sorted rows within (n + m + 8) 2^-53 relative of the oracle on the same sorted rows (at most
     n + m - 1 non-negative terms, each a few roundings)
  4  end to end: every per-projection W_p within (D + 16) 2^-24 (max |x_i| + max |y_j|) of the oracle (W_p is 1-Lipschitz in
     the sup norm of the atoms, the atoms are projections of unit directions); the shift closed form within the same bound
  5  exact identities: symmetry, zero, repeatability, chunking, cache
  6  non-finite input

Measured on the MI355X (the figures the tests print): see profiles/swd/accuracy.txt."""
import math
import warnings

import numpy as np
import pytest
import torch

import swd_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MEASURED = {}


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
    for section, lines in MEASURED.items():
        ref.record_accuracy(section, lines)


def rows(seed, n, d, shift=0.0):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32) + np.float32(shift)


def data_set(am, a):
    s = am.AudioMetricsData(True)
    s.add(torch.as_tensor(a).to(DEV))
    return s


def padded(a, extra, poison):
    """The matrix as a device view with a row stride of (columns rounded up to 4) + extra and `poison` in the padding."""
    n, d = a.shape
    buf = torch.full((n, (d + 3) // 4 * 4 + extra), poison, dtype=torch.float32, device=DEV)
    buf[:, :d] = torch.as_tensor(a)
    return buf[:, :d]


# ---------------------------------------------------------------------------------------------------- 1 projection
@pytest.mark.parametrize("n,nl,d", [(1, 1, 1), (127, 5, 33), (130, 130, 40), (257, 64, 96), (130, 300, 64)])
def test_projection_against_f64_matmul(am, ops, n, nl, d):
    x, theta = rows(n + d, n, d, 0.25), am.sliced_directions(d, nl, 5)
    want = ref.project(x, theta)
    bound = (d + 16) * 2.0 ** -24 * np.outer(np.linalg.norm(theta.astype(np.float64), axis=1), np.linalg.norm(x.astype(np.float64), axis=1))
    z = ops.sliced_project(torch.as_tensor(x).to(DEV), torch.as_tensor(theta).to(DEV))
    assert z.shape == (nl, n) and z.dtype == torch.float32
    got = z.cpu().numpy().astype(np.float64)
    ratio = float((np.abs(got - want) / bound).max())
    print(f"projection {n} x {nl} x {d}: largest error / bound {ratio:.4f}")
    MEASURED.setdefault("projection: largest |device - f64| / ((D + 16) 2^-24 |x| |theta|) (bound: 1)", []).append(f"{n} x {nl} x {d}: {ratio:.4f}")
    assert ratio <= 1.0
    # padded views: a row stride above D on both operands, NaN in the padding - the same bits
    zp = ops.sliced_project(padded(x, 4, math.nan), padded(theta, 8, math.nan))
    assert torch.equal(zp, z)


def test_projection_bits_do_not_depend_on_the_other_directions(am, ops):
    n, d = 257, 40
    x = torch.as_tensor(rows(3, n, d)).to(DEV)
    theta = torch.as_tensor(am.sliced_directions(d, 130, 9)).to(DEV)
    z = ops.sliced_project(x, theta)
    for k in (0, 63, 64, 128, 129):
        alone = ops.sliced_project(x, theta[k:k + 1].clone())
        assert torch.equal(alone[0], z[k]), k
    assert torch.equal(ops.sliced_project(x, theta[100:].clone()), z[100:])


# ---------------------------------------------------------------------------------------------------- 2 sort
def keys_of(bits):
    """The order-preserving transform of float32 bit patterns (uint32), NaNs mapped to the largest key."""
    bits = bits.astype(np.uint32)
    nan = (bits & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    key = bits ^ np.where(bits >> np.uint32(31) != 0, np.uint32(0xffffffff), np.uint32(0x80000000))
    return np.where(nan, np.uint32(0xffffffff), key)


def bits_of(keys):
    keys = keys.astype(np.uint32)
    back = np.where(keys >> np.uint32(31) != 0, keys ^ np.uint32(0x80000000), ~keys)
    return np.where(keys == np.uint32(0xffffffff), np.uint32(0x7fc00000), back)


def special_row(n, rng):
    pool = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.0, -1.0,
                     3.4028235e38, -3.4028235e38], dtype=np.float32)
    row = pool[rng.integers(0, len(pool), size=n)]
    row[:min(n, len(pool))] = pool[:min(n, len(pool))]
    bits = row.view(np.uint32).copy()
    bits[rng.integers(0, n, size=max(1, n // 16))] = 0xffc12345                     # NaNs with a sign and a payload
    return bits.view(np.float32)


def sort_on_device(ops, a, in_place=False):
    z = padded(a, 5, -math.inf)                                                     # padding that would sort FIRST if it were read
    out = ops.sort_rows(z, out=z if in_place else None)
    assert out.shape == z.shape and out.dtype == torch.float32
    if in_place:
        assert out is z and bool(torch.isinf(z._base[:, a.shape[1]:]).all())          # the padding was not written either
    return out.cpu().numpy()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, 70001])
def test_sort_rows_is_exact(ops, n):
    rng = np.random.default_rng(n)
    for nl in (1, 3):
        normal = rng.standard_normal((nl, n)).astype(np.float32)
        ordered = np.sort(normal, axis=1)
        plain = {"normals": normal, "all equal": np.full((nl, n), -2.5, dtype=np.float32), "sorted": ordered,
                 "reversed": ordered[:, ::-1].copy()}
        for name, a in plain.items():
            assert np.array_equal(sort_on_device(ops, a), np.sort(a, axis=1)), (name, nl, n)
        assert np.array_equal(sort_on_device(ops, normal, in_place=True), ordered), (nl, n)
        patterns = {"bit patterns": rng.integers(0, 1 << 32, size=(nl, n), dtype=np.uint64).astype(np.uint32).view(np.float32),
                    "special values": np.stack([special_row(n, rng) for _ in range(nl)])}
        for name, a in patterns.items():
            got = sort_on_device(ops, a)
            # the order of the keys, bit for bit: -0.0 before +0.0, NaNs last and canonical
            want_bits = bits_of(np.sort(keys_of(a.view(np.uint32)), axis=1))
            assert np.array_equal(got.view(np.uint32), want_bits), (name, nl, n)
            for r in range(nl):
                finite = a[r][~np.isnan(a[r])]
                assert np.array_equal(got[r, :len(finite)], np.sort(finite)), (name, nl, n, r)     # numpy's order on the non-NaN prefix
                assert int(np.isnan(got[r]).sum()) == n - len(finite) and bool(np.isnan(got[r, len(finite):]).all())
            # a permutation of the input (NaNs canonical): the sorted bits agree
            canon = a.view(np.uint32).copy()
            canon[np.isnan(a)] = 0x7fc00000
            assert np.array_equal(np.sort(canon, axis=1), np.sort(got.view(np.uint32), axis=1)), (name, nl, n)


# ---------------------------------------------------------------------------------------------------- 3 merge
@pytest.mark.parametrize("n,m", [(1, 1), (1, 7), (7, 1), (127, 129), (300, 257), (1025, 1023), (130, 4000), (4000, 130)])
def test_merge_against_the_oracle_on_device_sorted_rows(ops, n, m):
    nl = 3
    rng = np.random.default_rng(100 * n + m)
    zx = ops.sort_rows(torch.as_tensor(rng.standard_normal((nl, n)).astype(np.float32)).to(DEV))
    zy = ops.sort_rows(torch.as_tensor((rng.standard_normal((nl, m)) * 1.5 + 0.3).astype(np.float32)).to(DEV))
    hx, hy = zx.cpu().numpy(), zy.cpu().numpy()
    assert np.array_equal(hx, np.sort(hx, axis=1)) and np.array_equal(hy, np.sort(hy, axis=1))
    rel = (n + m + 8) * 2.0 ** -53
    for p in (1, 2):
        w, bad = ops.sliced_w(zx, zy, p)
        assert w.dtype == torch.float64 and bad.dtype == torch.int32 and bad.cpu().tolist() == [0] * nl
        got = w.cpu().numpy()
        want = np.array([ref.wpp_merged(a, b, p) for a, b in zip(hx, hy)])
        ratio = float((np.abs(got - want) / (rel * want)).max())
        print(f"merge {n} x {m}, p = {p}: largest relative error / bound {ratio:.4f}")
        MEASURED.setdefault("merge: largest relative |device - oracle| / ((n + m + 8) 2^-53) (bound: 1)", []).append(f"{n} x {m}, p = {p}: {ratio:.4f}")
        assert ratio <= 1.0
        swapped, _ = ops.sliced_w(zy, zx, p)
        assert torch.equal(swapped, w)


# ---------------------------------------------------------------------------------------------------- 4 end to end
_SHARED = {}


def e2e(am):
    """Sets, device results and oracle results of the end-to-end case: computed once."""
    if not _SHARED:
        n, m, d, nl = 300, 257, 40, 24
        x, y = rows(21, n, d), rows(22, m, d, 0.3)
        sx, sy = data_set(am, x), data_set(am, y)
        got = {p: am.sliced_wasserstein_distance(sx, sy, n_projections=nl, p=p, seed=7, cache_reference=False, return_projections=True)
               for p in (1, 2)}
        want = {p: ref.distance(x, y, nl, p, 7) for p in (1, 2)}
        _SHARED.update(x=x, y=y, sx=sx, sy=sy, d=d, nl=nl, got=got, want=want)
    return _SHARED


def test_end_to_end_against_the_oracle(am):
    c = e2e(am)
    xmax = float(np.linalg.norm(c["x"].astype(np.float64), axis=1).max())
    ymax = float(np.linalg.norm(c["y"].astype(np.float64), axis=1).max())
    bound = (c["d"] + 16) * 2.0 ** -24 * (xmax + ymax)
    for p in (1, 2):
        got, want = c["got"][p], c["want"][p]
        assert np.array_equal(got["swd_directions"], want["swd_directions"])
        err = np.abs(got["swd_per_projection"] ** (1.0 / p) - want["swd_per_projection"] ** (1.0 / p))
        print(f"end to end p = {p}: largest |W_p - oracle| / bound {err.max() / bound:.4f}; swd {got['swd']:.6f} oracle {want['swd']:.6f}")
        MEASURED.setdefault("end to end: largest per-projection |W_p - oracle| / ((D + 16) 2^-24 (max |x| + max |y|)) (bound: 1)",
                            []).append(f"300 x 257 x 40, L = 24, p = {p}: {err.max() / bound:.4f}")
        assert err.max() <= bound
        assert abs(got["swd"] - want["swd"]) <= bound and abs(got["swd_max"] - want["swd_max"]) <= bound
        assert got["swd_max_index"] == want["swd_max_index"] and got["swd_p"] == p and got["swd_n_projections"] == c["nl"]
        # |a^p - b^p| <= p max(a, b)^(p - 1) |a - b| per projection, so for their mean
        wmax = max(got["swd_max"], want["swd_max"])
        assert abs(got["swd_pp"] - want["swd_pp"]) <= p * wmax ** (p - 1) * bound
        # the host formulas on the device's own per-projection values, against the oracle's restatement of them
        restated = ref.summary(got["swd_per_projection"], p)
        assert all(got[k] == pytest.approx(restated[k], rel=1e-13) for k in restated)


def test_shift_closed_form(am):
    n, d, nl = 257, 33, 16
    rng = np.random.default_rng(8)
    x = (np.round(rng.standard_normal((n, d)) * 256.0) / 256.0).astype(np.float32)       # multiples of 2^-8: x + c is exact in f32
    c = (np.round(rng.standard_normal(d) * 256.0) / 256.0).astype(np.float32)
    y = x + c
    assert np.array_equal(y.astype(np.float64), x.astype(np.float64) + c.astype(np.float64))
    theta = am.sliced_directions(d, nl, 3)
    shift = np.abs(theta.astype(np.float64) @ c.astype(np.float64))
    bound = (d + 16) * 2.0 ** -24 * (np.linalg.norm(x.astype(np.float64), axis=1).max() + np.linalg.norm(y.astype(np.float64), axis=1).max())
    sx, sy = data_set(am, x), data_set(am, y)
    for p in (1, 2):
        got = am.sliced_wasserstein_distance(sx, sy, n_projections=nl, p=p, seed=3, cache_reference=False, return_projections=True)
        err = np.abs(got["swd_per_projection"] ** (1.0 / p) - shift)
        print(f"shift p = {p}: largest |W_p - |<theta, c>|| / bound {err.max() / bound:.4f}")
        assert err.max() <= bound
        assert abs(got["swd_max"] - shift.max()) <= bound


# ---------------------------------------------------------------------------------------------------- 5 exact identities
def test_exact_identities(am):
    from audio_metrics_amd.metrics.kad import reference_cache
    c = e2e(am)
    sx, sy, nl = c["sx"], c["sy"], c["nl"]
    for p in (1, 2):
        first = c["got"][p]["swd_per_projection"]
        kw = dict(n_projections=nl, p=p, seed=7, return_projections=True)
        again = am.sliced_wasserstein_distance(sx, sy, cache_reference=False, **kw)
        assert np.array_equal(again["swd_per_projection"], first) and again["swd"] == c["got"][p]["swd"]          # two calls
        swapped = am.sliced_wasserstein_distance(sy, sx, cache_reference=False, **kw)
        assert np.array_equal(swapped["swd_per_projection"], first) and swapped["swd"] == c["got"][p]["swd"]     # (x, y) and (y, x)
        small = am.sliced_wasserstein_distance(sx, sy, cache_reference=False, chunk_projections=3, **kw)
        assert np.array_equal(small["swd_per_projection"], first)                                                   # chunks of 128 and of 3
        for other in (sx, data_set(am, c["x"])):                                                                    # x is y, and an equal copy
            zero = am.sliced_wasserstein_distance(sx, other, cache_reference=False, **kw)
            assert np.all(zero["swd_per_projection"] == 0.0) and zero["swd"] == 0.0 and zero["swd_max"] == 0.0
            assert math.isnan(zero["swd_std_error"])
    # cached against uncached: the same bits; an append drops the entry
    ref_set = data_set(am, c["y"])
    kw = dict(n_projections=nl, p=2, seed=7, return_projections=True)
    filled = am.sliced_wasserstein_distance(sx, ref_set, **kw)
    assert list(reference_cache(ref_set).sliced) == [(7, nl)]
    kept = reference_cache(ref_set).sliced[(7, nl)][1][0]
    assert kept.shape == (nl, c["y"].shape[0]) and kept.dtype == torch.float32
    for chunk in (128, 5):
        cached = am.sliced_wasserstein_distance(sx, ref_set, chunk_projections=chunk, **kw)
        assert np.array_equal(cached["swd_per_projection"], c["got"][2]["swd_per_projection"]) and cached["swd"] == c["got"][2]["swd"]
    assert np.array_equal(filled["swd_per_projection"], c["got"][2]["swd_per_projection"])
    ref_set.add(torch.as_tensor(c["y"][:5]).to(DEV))
    assert reference_cache(ref_set).sliced == {}
    grown = am.sliced_wasserstein_distance(sx, ref_set, **kw)
    assert not np.array_equal(grown["swd_per_projection"], filled["swd_per_projection"])
    assert list(reference_cache(ref_set).sliced) == [(7, nl)]


# ---------------------------------------------------------------------------------------------------- 6 non-finite input
def test_non_finite_rows(am):
    c = e2e(am)
    x = c["x"].copy()
    x[17, 3] = np.nan
    x[40, 0] = np.inf
    sx = data_set(am, x)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = am.sliced_wasserstein_distance(sx, c["sy"], n_projections=c["nl"], p=2, seed=7, cache_reference=False,
                                             return_projections=True)
    mine = [w for w in caught if issubclass(w.category, RuntimeWarning) and "non-finite" in str(w.message)]
    # a NaN element makes its row's projection NaN on every direction; an infinite one +-inf (or NaN where theta is 0)
    assert len(mine) == 1 and f"{2 * c['nl']} non-finite" in str(mine[0].message)
    assert math.isnan(got["swd"]) and math.isnan(got["swd_pp"]) and math.isnan(got["swd_max"])
    assert got["swd_per_projection"].shape == (c["nl"],) and np.isnan(got["swd_per_projection"]).all()
    assert got["swd_n_projections"] == c["nl"] and got["swd_directions"].shape == (c["nl"], c["d"])
