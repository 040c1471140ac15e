"""Two-sided row sums of the Gaussian kernel blocks on the device (am_mmd_rbf_rows_f32 through hip_ops.mmd_rbf_row_sums)
against the float64 oracle of tests/mmd_rows_reference.py.

  1  exact data: all four normalised vectors within 1e-12 x mean |K|, at tile edges, a lone partial tile, both inner-tail forms
  2  the seams: several Q chunks, diagonal and off-diagonal tiles; a second band of P tiles (more than 64 tiles)
  3  consistency with the whole-set sums, the one-group row sums and the call with the sets swapped
  4  bits: repeatability, another leading dimension, device-fed bandwidth, each block alone
  5  duplicated rows and a set against itself
  6  real-valued rows against the emulated f32 dot products
  7  the NaN pattern of a non-finite row"""
import ctypes

import numpy as np
import pytest
import torch

import inputs as gi
import kad_reference as ka
import kd_reference as kr
import mmd_rows_reference as mr

pytestmark = pytest.mark.gpu

EXACT = 1e-12
DEV = "cuda:0"
SIGMA = 10.0
GAMMA = 1.0 / (2.0 * SIGMA * SIGMA)
NAMES = ("w / (n - 1)", "c / m", "v / (m - 1)", "r / n")


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    audio_metrics_amd._lib.load()
    return audio_metrics_amd


@pytest.fixture(scope="module")
def ops(am):
    return am.hip_ops


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def row_sums(ops, x, y, blocks=7, **width):
    """the device call, checked and read back: (out_x [n, 2], out_y [m, 2]) as numpy"""
    out_x, out_y = ops.mmd_rbf_row_sums(x, y, blocks=blocks, **width)
    for out, rows in ((out_x, x.shape[0]), (out_y, y.shape[0])):
        assert out.dtype == torch.float64 and tuple(out.shape) == (rows, 2) and out.is_cuda and out.is_contiguous()
    return out_x.cpu().numpy(), out_y.cpu().numpy()


def assert_within(got, want, limit, what):
    """every entry of the four normalised vectors within `limit` of the oracle's"""
    failures = []
    for name, g, w in zip(NAMES, mr.normalised(got), mr.normalised(want)):
        err = float(np.abs(g - w).max())
        print(f"{what}: {name} max |err| {err:.3e} limit {limit:.3e}")
        if not err <= limit:
            failures.append((name, err, limit))
    assert not failures, (what, failures)


# ---------------------------------------------------------------------------------------------------- 1. exact data
@pytest.fixture(scope="module")
def exact_cases():
    out = {}
    for d in (32, 100, 512):
        rng = np.random.default_rng(5100 + d)
        x, y = kr.rbf_rows(rng, 785, d, SIGMA), kr.rbf_rows(rng, 300, d, SIGMA)
        out[d] = dict(x=x, y=y, want=mr.row_sums(x, y, GAMMA))
    return out


@pytest.mark.parametrize("d", [32, 100, 512])
def test_exact_data(ops, exact_cases, d):
    c = exact_cases[d]
    assert 0.01 < c["want"]["scale"] < 0.99                          # K spreads over (0, 1)
    got = row_sums(ops, dev(c["x"]), dev(c["y"]), gamma=GAMMA)
    assert_within(got, c["want"], EXACT * c["want"]["scale"], f"D={d}")


@pytest.mark.parametrize("n, m", [(2, 3), (129, 127)])
def test_exact_data_small_shapes(ops, n, m):
    """a lone partial tile; one row past a tile edge against one row short of it"""
    rng = np.random.default_rng(5200 + n)
    x, y = kr.rbf_rows(rng, n, 32, SIGMA), kr.rbf_rows(rng, m, 32, SIGMA)
    want = mr.row_sums(x, y, GAMMA)
    assert_within(row_sums(ops, dev(x), dev(y), gamma=GAMMA), want, EXACT * want["scale"], f"{n} x {m}")


# ---------------------------------------------------------------------------------------------------- 2. seams
def test_chunk_seams(ops):
    """2 100 rows are 17 tiles per side: diagonal and off-diagonal tiles, and every row's sums are put together from the
    partials of several Q chunks (P side) and of several P tiles (Q side)."""
    rng = np.random.default_rng(5300)
    x, y = kr.rbf_rows(rng, 2100, 32, SIGMA), kr.rbf_rows(rng, 2100, 32, SIGMA)
    want = mr.row_sums(x, y, GAMMA)
    assert_within(row_sums(ops, dev(x), dev(y), gamma=GAMMA), want, EXACT * want["scale"], "17 tiles")


def test_band_seam(ops):
    """The P tiles are swept in bands of 64.  8 325 candidate rows are 66 tiles - a full band and a second one of two tiles,
    the last tile partial - in the symmetric sweep (XX: rows of the first band receive their Q-side sums from both bands) and
    as the P side of the cross block (every r_j is added up over both bands); 66 tiles also make chunks of two Q tiles, the
    last chunk of an odd P tile half empty.  Below 10 000 rows: against the numpy oracle."""
    rng = np.random.default_rng(5400)
    x, y = kr.rbf_rows(rng, 64 * 128 + 133, 32, SIGMA), kr.rbf_rows(rng, 300, 32, SIGMA)
    want = mr.row_sums(x, y, GAMMA)
    got = row_sums(ops, dev(x), dev(y), gamma=GAMMA)
    assert_within(got, want, EXACT * want["scale"], "two bands")
    # the sets swapped: the long set is the Q side of the cross block and the YY block has the two bands
    back = row_sums(ops, dev(y), dev(x), gamma=GAMMA)
    swapped = dict(w=want["v"], c=want["r"], v=want["w"], r=want["c"], scale=want["scale"])
    assert_within(back, swapped, EXACT * want["scale"], "two bands, swapped")


# ---------------------------------------------------------------------------------------------------- 3. consistency
def test_consistency_with_the_other_entry_points(ops, exact_cases):
    c = exact_cases[100]
    n, m = len(c["x"]), len(c["y"])
    xt, yt = dev(c["x"]), dev(c["y"])
    limit = EXACT * c["want"]["scale"]
    out_x, out_y = row_sums(ops, xt, yt, gamma=GAMMA)
    # both axes of the cross block add up to the same total
    sc, sr = out_x[:, 1].sum() / (float(n) * m), out_y[:, 1].sum() / (float(n) * m)
    print(f"sum c {sc!r} sum r {sr!r} limit {limit:.3e}")
    assert abs(sc - sr) <= limit
    # the three totals against the whole-set sums
    whole = ka.device_means(ops.mmd_rbf_sums(xt, yt, gamma=GAMMA).cpu().numpy(), n, m)
    mine = ka.device_means([out_x[:, 0].sum(), out_y[:, 0].sum(), out_x[:, 1].sum()], n, m)
    print(f"totals {mine!r} whole-set {whole!r}")
    assert (np.abs(mine - whole) <= limit).all()
    # out_x against the row sums of one group
    res = ops.mmd_rbf_group_sums(xt, None, [0, n], yt, gamma=GAMMA, rows=True)
    res[-1]()
    rows = res[1].cpu().numpy()
    err_w, err_c = np.abs(out_x[:, 0] - rows[:, 0]).max() / (n - 1.0), np.abs(out_x[:, 1] - rows[:, 1]).max() / m
    print(f"one group: w {err_w:.3e} c {err_c:.3e} limit {limit:.3e}")
    assert err_w <= limit and err_c <= limit
    # the sets swapped: r of (X, Y) is c of (Y, X), v is w
    back_x, back_y = row_sums(ops, yt, xt, gamma=GAMMA)
    assert np.abs(out_y[:, 1] - back_x[:, 1]).max() / n <= limit and np.abs(out_x[:, 1] - back_y[:, 1]).max() / m <= limit
    assert np.abs(out_y[:, 0] - back_x[:, 0]).max() / (m - 1.0) <= limit and np.abs(out_x[:, 0] - back_y[:, 0]).max() / (n - 1.0) <= limit


# ---------------------------------------------------------------------------------------------------- 4. bits
def raw_call(am, x, y, blocks, fill, gamma=GAMMA):
    """am_mmd_rbf_rows_f32 on outputs prefilled with `fill`: (out_x, out_y) device tensors"""
    ops, lib = am.hip_ops, am._lib.load()
    (n, d), m = x.shape, y.shape[0]
    out_x = torch.full((n, 2), fill, dtype=torch.float64, device=DEV)
    out_y = torch.full((m, 2), fill, dtype=torch.float64, device=DEV)
    nb = lib.am_mmd_rbf_rows_workspace_bytes(n, m, d, blocks)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    ops._call(lib, "am_mmd_rbf_rows_f32", x.device, ptr(x), n, x.stride(0), ptr(y), m, y.stride(0), d, ctypes.c_void_p(None), gamma,
              blocks, ptr(out_x), ptr(out_y), ptr(ws), nb)
    torch.cuda.synchronize()
    return out_x, out_y


def test_bits(am, ops, exact_cases):
    c = exact_cases[100]
    xt, yt = dev(c["x"]), dev(c["y"])
    first = ops.mmd_rbf_row_sums(xt, yt, gamma=GAMMA)
    again = ops.mmd_rbf_row_sums(xt, yt, gamma=GAMMA)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert not torch.isnan(first[0]).any() and not torch.isnan(first[1]).any()
    # a row view with another leading dimension: the padding must never be read as data
    wide_x = torch.full((len(c["x"]), 112), 1e30, dtype=torch.float32, device=DEV)
    wide_y = torch.full((len(c["y"]), 104), 1e30, dtype=torch.float32, device=DEV)
    wide_x[:, :100], wide_y[:, :100] = xt, yt
    view = ops.mmd_rbf_row_sums(wide_x[:, :100], wide_y[:, :100], gamma=GAMMA)
    assert torch.equal(first[0], view[0]) and torch.equal(first[1], view[1])
    # the bandwidth from device memory: gamma = 0.5 / (double)bw2 formed on the device = the same host expression
    bw2 = np.float32(SIGMA * SIGMA * 1.0009765625)
    fed = ops.mmd_rbf_row_sums(xt, yt, bw2=torch.tensor(bw2, dtype=torch.float32, device=DEV))
    host = ops.mmd_rbf_row_sums(xt, yt, gamma=0.5 / float(bw2))
    assert torch.equal(fed[0], host[0]) and torch.equal(fed[1], host[1])
    assert not torch.equal(fed[0], first[0])
    # each block alone: the bits of the full call in the slots it owns, the sentinel everywhere else
    fill = -7.5
    owns = {1: ((0, 0),), 2: ((1, 0),), 4: ((0, 1), (1, 1))}                  # block -> (output, column)
    for blocks in (1, 2, 4, 5, 6, 3):
        alone = raw_call(am, xt, yt, blocks, fill)
        mine = {slot for b, slots in owns.items() if blocks & b for slot in slots}
        for o in (0, 1):
            for col in (0, 1):
                if (o, col) in mine:
                    assert torch.equal(alone[o][:, col], first[o][:, col]), (blocks, o, col)
                else:
                    assert (alone[o][:, col] == fill).all(), (blocks, o, col)
    # a side no named block writes is not asked for at all
    only_y = ops.mmd_rbf_row_sums(xt, yt, gamma=GAMMA, blocks=ops.MMD_YY)
    assert only_y[0] is None and torch.equal(only_y[1][:, 0], first[1][:, 0]) and torch.isnan(only_y[1][:, 1]).all()
    only_x = ops.mmd_rbf_row_sums(xt, yt, gamma=GAMMA, blocks=ops.MMD_XX)
    assert only_x[1] is None and torch.equal(only_x[0][:, 0], first[0][:, 0]) and torch.isnan(only_x[0][:, 1]).all()


# ---------------------------------------------------------------------------------------------------- 5. duplicates and self
def test_duplicated_rows_and_a_set_against_itself(ops):
    """Self pairs go by INDEX: two copies of a row stay each other's pair with k = 1, and with Y = X (the same tensor) the
    cross sums keep the diagonal that w drops."""
    rng = np.random.default_rng(5500)
    x = kr.rbf_rows(rng, 300, 100, SIGMA)
    x[200] = x[17]                                                    # a pair in different tiles
    x[140] = x[139]                                                   # neighbours in one tile
    want = mr.row_sums(x, x, GAMMA, same=True)
    xt = dev(x)
    got = row_sums(ops, xt, xt, gamma=GAMMA)
    assert_within(got, want, EXACT * want["scale"], "Y = X")
    out_x, out_y = got
    others = mr.row_sums(np.delete(x, 200, axis=0), x[:2], GAMMA)["w"]          # row 17 without its copy
    assert abs((out_x[17, 0] - others[17]) - 1.0) <= EXACT * want["scale"] * 299
    assert (np.abs((out_x[:, 1] - out_x[:, 0]) - 1.0) <= 2 * EXACT * want["scale"] * 300).all()     # c_i = w_i + k(x_i, x_i)
    assert np.array_equal(out_x[:, 0], out_y[:, 0])                  # the same block, the same order: XX and YY of one set


# ---------------------------------------------------------------------------------------------------- 6. real-valued rows
@pytest.mark.parametrize("kind, d", [("randn", 64), ("unit", 512)])
def test_real_valued_rows(ops, kind, d):
    """The mean of each of the four normalised vectors within MARGIN x the emulated error of that statistic (the
    rounding_tolerance form of kd_reference: the f32 dot products rounded once per 32-element slab; MARGIN covers the matrix
    cores' rounding after every product).  The four means ARE the statistics xx, xy, yy, xy of
    test_gpu_kad.py::test_sums_on_real_valued_rows, and the dot products are those of am_mmd_rbf_f32 bit for bit (the same
    engine and slab order), so the rows are the rows of that test (seed 800 + d) and the limits the limits it holds
    am_mmd_rbf_f32 to.  An emulated error is a signed sum of a million roundings and can cancel by accident: with seed
    950 + d, unit rows, D = 512, it was 3.2e-12 (xx), 1.1e-11 (yy) but 1.1e-12 (xy) against a device error of 3.0e-11 in xy -
    the error am_mmd_rbf_f32 has on those rows too, which is what the last assertion pins: on real-valued rows the totals of
    the row sums and the whole-set sums differ by their f64 summation order only."""
    n = m = 1000
    y, x = gi.pair(kind, 800 + d, m, n, d)
    pairs = ka.pair_values(y)
    gamma = 0.5 / float(pairs[ka.lower_median_rank(len(pairs))])     # the kernel width KAD itself would take
    want = mr.row_sums(x, y, gamma)
    emulated = mr.row_sums(x, y, gamma, dots=kr.emulated_dots("f32"))
    xt, yt = dev(x), dev(y)
    got = row_sums(ops, xt, yt, gamma=gamma)
    failures = []
    for name, g, w, e in zip(NAMES, mr.normalised(got), mr.normalised(want), mr.normalised(emulated)):
        err, limit = abs(g.mean() - w.mean()), kr.MARGIN * abs(e.mean() - w.mean())
        print(f"{kind} D={d} mean {name}: device {g.mean()!r} oracle {w.mean()!r} |err| {err:.3e} limit {limit:.3e}")
        if not err <= limit:
            failures.append((name, err, limit))
    assert not failures, failures
    whole = ka.device_means(ops.mmd_rbf_sums(xt, yt, gamma=gamma).cpu().numpy(), n, m)
    mine = ka.device_means([got[0][:, 0].sum(), got[1][:, 0].sum(), got[0][:, 1].sum()], n, m)
    print(f"{kind} D={d} totals {mine!r} am_mmd_rbf_f32 {whole!r}")
    assert (np.abs(mine - whole) <= EXACT * want["scale"]).all()


# ---------------------------------------------------------------------------------------------------- 7. a NaN row
def test_a_nan_row_in_x(ops, exact_cases):
    """Every sum the row takes part in is NaN and no other: all of w (each row pairs with it), its own c, all of r; the other
    rows' c and all of v are the bits of the clean run."""
    c = exact_cases[100]
    yt = dev(c["y"])
    clean_x, clean_y = row_sums(ops, dev(c["x"]), yt, gamma=GAMMA)
    bad = c["x"].copy()
    victim = 401
    bad[victim, 17] = np.nan
    out_x, out_y = row_sums(ops, dev(bad), yt, gamma=GAMMA)
    assert np.isnan(out_x[:, 0]).all()
    assert np.isnan(out_x[victim, 1]) and np.isnan(out_y[:, 1]).all()
    assert np.array_equal(np.delete(out_x[:, 1], victim), np.delete(clean_x[:, 1], victim))
    assert np.array_equal(out_y[:, 0], clean_y[:, 0])
