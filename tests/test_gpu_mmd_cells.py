"""Unit-pair sums of the Gaussian kernel blocks on the device (am_mmd_rbf_cells_f32 through hip_ops.mmd_rbf_cell_sums) against
the float64 oracle of tests/mmd_cells_reference.py.

  1  exact data: all three cell matrices, per position pair, within 1e-12 x mean |K|; tile and cell edges, both inner-tail forms
  2  the seams: 17 tiles per side, several Q chunks; the within matrices equal their transposes bit for bit
  3  consistency with the whole-set sums and with the two-sided row sums folded per 32 rows
  4  position lists: a permuted list into a shuffled store, -1 pads in the middle, an index out of range and the flag word
  5  units: ragged cell offsets against the host fold of the device's own cells (bits) and against the oracle
  6  bits: repeatability, another leading dimension, device-fed bandwidth, each block alone, untouched outputs
  7  duplicated rows and a set against itself
  8  real-valued rows against the emulated f32 dot products
  9  the NaN pattern of a non-finite row"""
import ctypes

import numpy as np
import pytest
import torch

import inputs as gi
import kad_reference as ka
import kd_reference as kr
import mmd_cells_reference as mc

pytestmark = pytest.mark.gpu

EXACT = 1e-12
DEV = "cuda:0"
SIGMA = 10.0
GAMMA = 1.0 / (2.0 * SIGMA * SIGMA)
CELL = 32
PAIRS = float(CELL * CELL)
BLOCKS = ("xx", "yy", "xy")


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


def cell_sums(ops, x, y, **kw):
    """the device call, checked and read back: dict of numpy matrices (None for a block that was not asked for)"""
    out = ops.mmd_rbf_cell_sums(x, y, **kw)
    for o in out:
        assert o is None or (o.dtype == torch.float64 and o.is_cuda and o.is_contiguous() and o.dim() == 2)
    return {k: (None if o is None else o.cpu().numpy()) for k, o in zip(BLOCKS, out)}


def assert_within(got, want, limit, what, pairs=None):
    """every entry of the three matrices, per position pair of a full cell pair (`pairs`: dict of the pair counts of every
    entry, for units of several cells), within `limit` of the oracle's"""
    failures = []
    for k in BLOCKS:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        err = float((np.abs(got[k] - want[k]) / (PAIRS if pairs is None else pairs[k])).max())
        print(f"{what}: {k} {got[k].shape} max |err| per pair {err:.3e} limit {limit:.3e}")
        if not err <= limit:
            failures.append((k, err, limit))
    assert not failures, (what, failures)


# ---------------------------------------------------------------------------------------------------- 1. exact data
@pytest.fixture(scope="module")
def exact_cases():
    out = {}
    for d in (32, 100, 512):
        rng = np.random.default_rng(6100 + d)
        x, y = kr.rbf_rows(rng, 785, d, SIGMA), kr.rbf_rows(rng, 300, d, SIGMA)
        out[d] = dict(x=x, y=y, want=mc.unit_sums(x, y, GAMMA))
    return out


@pytest.mark.parametrize("d", [32, 100, 512])
def test_exact_data(ops, exact_cases, d):
    c = exact_cases[d]
    assert 0.01 < c["want"]["scale"] < 0.99                          # K spreads over (0, 1)
    got = cell_sums(ops, dev(c["x"]), dev(c["y"]), gamma=GAMMA)
    assert got["xx"].shape == (25, 25) and got["yy"].shape == (10, 10) and got["xy"].shape == (25, 10)
    assert_within(got, c["want"], EXACT * c["want"]["scale"], f"D={d}")


@pytest.mark.parametrize("n, m", [(2, 3), (33, 31), (129, 127)])
def test_exact_data_small_shapes(ops, n, m):
    """a lone partial cell; one row past a cell edge against one row short of it; the same at a tile edge"""
    rng = np.random.default_rng(6200 + n)
    x, y = kr.rbf_rows(rng, n, 32, SIGMA), kr.rbf_rows(rng, m, 32, SIGMA)
    want = mc.unit_sums(x, y, GAMMA)
    assert_within(cell_sums(ops, dev(x), dev(y), gamma=GAMMA), want, EXACT * want["scale"], f"{n} x {m}")


# ---------------------------------------------------------------------------------------------------- 2. seams
def test_chunk_seams_and_exact_symmetry(ops):
    """2 100 rows are 17 tiles and 66 cells per side: diagonal and off-diagonal tiles, several Q chunks per P tile, a last
    tile of two cells.  Every within value is written to [a][b] and [b][a]: the matrices equal their transposes bit for bit."""
    rng = np.random.default_rng(6300)
    x, y = kr.rbf_rows(rng, 2100, 32, SIGMA), kr.rbf_rows(rng, 2100, 32, SIGMA)
    want = mc.unit_sums(x, y, GAMMA)
    got = cell_sums(ops, dev(x), dev(y), gamma=GAMMA)
    assert got["xx"].shape == (66, 66)
    assert_within(got, want, EXACT * want["scale"], "17 tiles")
    assert np.array_equal(got["xx"], got["xx"].T) and np.array_equal(got["yy"], got["yy"].T)
    assert not np.isnan(got["xx"]).any() and not np.isnan(got["xy"]).any()


# ---------------------------------------------------------------------------------------------------- 3. consistency
def test_consistency_with_the_other_entry_points(ops, exact_cases):
    c = exact_cases[100]
    n, m = len(c["x"]), len(c["y"])
    xt, yt = dev(c["x"]), dev(c["y"])
    got = cell_sums(ops, xt, yt, gamma=GAMMA)
    # the total of each matrix against the whole-set sums: relative 1e-13
    whole = ops.mmd_rbf_sums(xt, yt, gamma=GAMMA).cpu().numpy()
    for k, w in zip(BLOCKS, whole):
        rel = abs(got[k].sum() - w) / abs(w)
        print(f"total {k}: cells {got[k].sum()!r} am_mmd_rbf_f32 {w!r} relative {rel:.3e}")
        assert rel <= 1e-13, (k, rel)
    # cell rows and columns summed against the two-sided row sums folded per 32 rows
    out_x, out_y = (t.cpu().numpy() for t in ops.mmd_rbf_row_sums(xt, yt, gamma=GAMMA))
    ox, oy = mc.cell_offsets(n)[:-1], mc.cell_offsets(m)[:-1]
    limit = EXACT * c["want"]["scale"]
    for what, mine, theirs, partners in (("w", got["xx"].sum(1), np.add.reduceat(out_x[:, 0], ox), n), ("w by column", got["xx"].sum(0), np.add.reduceat(out_x[:, 0], ox), n),
                                         ("v", got["yy"].sum(1), np.add.reduceat(out_y[:, 0], oy), m), ("c", got["xy"].sum(1), np.add.reduceat(out_x[:, 1], ox), m),
                                         ("r", got["xy"].sum(0), np.add.reduceat(out_y[:, 1], oy), n)):
        err = float(np.abs(mine - theirs).max()) / (CELL * float(partners))
        print(f"{what}: max |err| per pair {err:.3e} limit {limit:.3e}")
        assert err <= limit, (what, err)


# ---------------------------------------------------------------------------------------------------- raw calls
def raw_call(am, x, y, blocks=7, fill=-7.5, gamma=GAMMA, idx_x=None, idx_y=None, units_x=None, units_y=None):
    """am_mmd_rbf_cells_f32 on outputs prefilled with `fill`: (xx, yy, xy device tensors, the flag word)"""
    ops, lib = am.hip_ops, am._lib.load()
    (n, d), m = x.shape, y.shape[0]
    p1, p2 = (n if idx_x is None else idx_x.numel()), (m if idx_y is None else idx_y.numel())
    u1 = -(-p1 // CELL) if units_x is None else len(units_x) - 1
    u2 = -(-p2 // CELL) if units_y is None else len(units_y) - 1
    outs = [torch.full(s, fill, dtype=torch.float64, device=DEV) for s in ((u1, u1), (u2, u2), (u1, u2))]
    nb = lib.am_mmd_rbf_cells_workspace_bytes(p1, p2, d, blocks)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
    ptr = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())
    host = lambda u: ctypes.c_void_p(None) if u is None else ctypes.cast((ctypes.c_int64 * len(u))(*u), ctypes.c_void_p)
    ops._call(lib, "am_mmd_rbf_cells_f32", x.device, ptr(x), n, x.stride(0), ptr(idx_x), p1, host(units_x), u1, ptr(y), m, y.stride(0),
              ptr(idx_y), p2, host(units_y), u2, d, ctypes.c_void_p(None), gamma, blocks, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
              ptr(ws), nb)
    torch.cuda.synchronize()
    return outs[0], outs[1], outs[2], int(ws[:8].view(torch.int64).item())


# ---------------------------------------------------------------------------------------------------- 4. lists
def test_position_lists(am, ops, exact_cases):
    c = exact_cases[100]
    x, y = c["x"], c["y"]
    n, m = len(x), len(y)
    xt, yt = dev(x), dev(y)
    dense = ops.mmd_rbf_cell_sums(xt, yt, gamma=GAMMA)
    # the rows stored in another order and listed back into place: the bits of the dense call
    rng = np.random.default_rng(6400)
    px, py = rng.permutation(n), rng.permutation(m)
    ix, iy = np.argsort(px), np.argsort(py)                          # x[px][ix] is x
    listed = ops.mmd_rbf_cell_sums(dev(x[px]), dev(y[py]), idx_x=dev(ix), idx_y=dev(iy), gamma=GAMMA)
    for a, b in zip(dense, listed):
        assert torch.equal(a, b)
    one_side = ops.mmd_rbf_cell_sums(dev(x[px]), yt, idx_x=dev(ix), gamma=GAMMA)
    for a, b in zip(dense, one_side):
        assert torch.equal(a, b)
    # -1 pads in the middle of a list: rows move into other cells, the pads contribute nothing, the flag stays 0
    idx = np.full(352, -1, dtype=np.int64)
    idx[:50], idx[64:100], idx[100:301], idx[320:351] = np.arange(50), np.arange(100, 136), np.arange(300, 501), np.arange(700, 731)
    idy = np.full(96, -1, dtype=np.int64)
    idy[3:70], idy[75:96] = np.arange(67), np.arange(279, 300)
    want = mc.unit_sums(x, y, GAMMA, idx_x=idx, idx_y=idy)
    got = cell_sums(ops, xt, yt, idx_x=dev(idx), idx_y=dev(idy), gamma=GAMMA)
    assert got["xx"].shape == (11, 11) and got["yy"].shape == (3, 3)
    assert_within(got, want, EXACT * want["scale"], "lists with pads")
    padded = raw_call(am, xt, yt, idx_x=dev(idx), idx_y=dev(idy))
    assert padded[3] == 0
    for k, t in zip(BLOCKS, padded[:3]):
        assert np.array_equal(t.cpu().numpy(), got[k])
    # an index out of range is an empty position like -1, and the flag word names it: 1 + its position
    bad = idx.copy()
    assert bad[70] >= 0
    clean = bad.copy()
    bad[70], clean[70] = n + 5, -1
    flagged, pad = raw_call(am, xt, yt, idx_x=dev(bad), idx_y=dev(idy)), raw_call(am, xt, yt, idx_x=dev(clean), idx_y=dev(idy))
    assert flagged[3] == 71 and pad[3] == 0
    for a, b in zip(flagged[:3], pad[:3]):
        assert torch.equal(a, b)
    changed = np.flatnonzero((flagged[0].cpu().numpy() != padded[0].cpu().numpy()).any(1))
    assert changed.tolist() == list(range(11))                        # cell 2 lost a row: its row and column, i.e. one entry per row
    assert np.array_equal(np.delete(np.delete(flagged[0].cpu().numpy(), 2, 0), 2, 1), np.delete(np.delete(padded[0].cpu().numpy(), 2, 0), 2, 1))
    with pytest.raises(ValueError, match=r"idx_x\[70\] = 790"):
        ops.mmd_rbf_cell_sums(xt, yt, idx_x=dev(bad), idx_y=dev(idy), gamma=GAMMA)
    # the largest flagged position of a list is reported
    bad[300] = -2
    assert raw_call(am, xt, yt, idx_x=dev(bad), blocks=1)[3] == 301


# ---------------------------------------------------------------------------------------------------- 5. units
def host_fold(cells, ua, ub):
    """the unit pair's cells added in row-major order, one Python float at a time"""
    out = np.zeros((len(ua) - 1, len(ub) - 1))
    for u in range(len(ua) - 1):
        for v in range(len(ub) - 1):
            s = 0.0
            for a in range(ua[u], ua[u + 1]):
                for b in range(ub[v], ub[v + 1]):
                    s += float(cells[a, b])
            out[u, v] = s
    return out


def test_ragged_units(ops):
    rng = np.random.default_rng(6500)
    x, y = kr.rbf_rows(rng, 170, 100, SIGMA), kr.rbf_rows(rng, 190, 100, SIGMA)       # 6 cells a side, the last one partial
    ux, uy = [0, 1, 4, 6], [0, 3, 4, 6]
    xt, yt = dev(x), dev(y)
    cells = cell_sums(ops, xt, yt, gamma=GAMMA)
    got = cell_sums(ops, xt, yt, units_x=ux, units_y=uy, gamma=GAMMA)
    for k, (a, b) in zip(BLOCKS, ((ux, ux), (uy, uy), (ux, uy))):
        assert got[k].shape == (3, 3)
        assert np.array_equal(got[k], host_fold(cells[k], a, b)), k
    want = mc.unit_sums(x, y, GAMMA, units_x=ux, units_y=uy)
    cx, cy = np.diff(ux) * float(CELL), np.diff(uy) * float(CELL)
    assert_within(got, want, EXACT * want["scale"], "ragged units", dict(xx=np.outer(cx, cx), yy=np.outer(cy, cy), xy=np.outer(cx, cy)))
    # units on one side only: the other side's units are its cells
    half = cell_sums(ops, xt, yt, units_x=ux, gamma=GAMMA)
    assert np.array_equal(half["xx"], got["xx"]) and np.array_equal(half["yy"], cells["yy"])
    assert np.array_equal(half["xy"], host_fold(cells["xy"], ux, list(range(7))))
    # one unit per side: the three totals
    whole = cell_sums(ops, xt, yt, units_x=[0, 6], units_y=[0, 6], gamma=GAMMA)
    assert whole["xx"].shape == (1, 1) and whole["xy"][0, 0] == host_fold(cells["xy"], [0, 6], [0, 6])[0, 0]


# ---------------------------------------------------------------------------------------------------- 6. bits
def test_bits(am, ops, exact_cases):
    c = exact_cases[100]
    xt, yt = dev(c["x"]), dev(c["y"])
    first = ops.mmd_rbf_cell_sums(xt, yt, gamma=GAMMA)
    again = ops.mmd_rbf_cell_sums(xt, yt, gamma=GAMMA)
    for a, b in zip(first, again):
        assert torch.equal(a, b) and not torch.isnan(a).any()
    # a row view with another leading dimension: the padding must never be read as data
    wide_x = torch.full((len(c["x"]), 112), 1e30, dtype=torch.float32, device=DEV)
    wide_y = torch.full((len(c["y"]), 104), 1e30, dtype=torch.float32, device=DEV)
    wide_x[:, :100], wide_y[:, :100] = xt, yt
    view = ops.mmd_rbf_cell_sums(wide_x[:, :100], wide_y[:, :100], gamma=GAMMA)
    for a, b in zip(first, view):
        assert torch.equal(a, b)
    # the bandwidth from device memory: gamma = 0.5 / (double)bw2 formed on the device = the same host expression
    bw2 = np.float32(SIGMA * SIGMA * 1.0009765625)
    fed = ops.mmd_rbf_cell_sums(xt, yt, bw2=torch.tensor(bw2, dtype=torch.float32, device=DEV))
    host = ops.mmd_rbf_cell_sums(xt, yt, gamma=0.5 / float(bw2))
    for a, b, f in zip(fed, host, first):
        assert torch.equal(a, b) and not torch.equal(a, f)
    # each block alone: the bits of the full call in its own output, the fill pattern in the others
    fill = -7.5
    for blocks in (1, 2, 4, 5, 6, 3):
        alone = raw_call(am, xt, yt, blocks, fill)
        for b in range(3):
            if blocks & (1 << b):
                assert torch.equal(alone[b], first[b]), (blocks, b)
            else:
                assert (alone[b] == fill).all(), (blocks, b)
    # with units too: a block that is not named is not touched
    alone = raw_call(am, xt, yt, 4, fill, units_x=[0, 10, 25], units_y=[0, 3, 10])
    assert (alone[0] == fill).all() and (alone[1] == fill).all() and not (alone[2] == fill).any()
    # the wrapper does not ask for the outputs of blocks that are not named
    only = ops.mmd_rbf_cell_sums(xt, yt, gamma=GAMMA, blocks=ops.MMD_XX | ops.MMD_XY)
    assert only[1] is None and torch.equal(only[0], first[0]) and torch.equal(only[2], first[2])


# ---------------------------------------------------------------------------------------------------- 7. duplicates and self
def test_duplicated_rows_and_a_set_against_itself(ops):
    """Self pairs go by POSITION: two copies of a row stay each other's pair with k = 1, and with Y = X (the same tensor) the
    cross matrix keeps the diagonal that the within matrix drops."""
    rng = np.random.default_rng(6600)
    x = kr.rbf_rows(rng, 300, 100, SIGMA)
    x[200] = x[17]                                                    # a pair in different tiles
    x[140] = x[139]                                                   # neighbours in one cell
    want = mc.unit_sums(x, x, GAMMA, same=True)
    xt = dev(x)
    got = cell_sums(ops, xt, xt, gamma=GAMMA)
    assert_within(got, want, EXACT * want["scale"], "Y = X")
    assert np.array_equal(got["xx"], got["yy"])                       # the same block, the same order
    limit = EXACT * want["scale"] * PAIRS
    rows = np.diag(np.diff(mc.cell_offsets(300)).astype(np.float64))  # k(x_i, x_i) = 1 for every row of a diagonal cell
    assert np.abs((got["xy"] - got["xx"]) - rows).max() <= 2 * limit


# ---------------------------------------------------------------------------------------------------- 8. real-valued rows
@pytest.mark.parametrize("kind, d", [("randn", 64), ("unit", 512)])
def test_real_valued_rows(ops, kind, d):
    """The mean of each of the three matrices (per pair) within MARGIN x the emulated error of that statistic - the method
    and the limits of test_gpu_mmd_rows.py::test_real_valued_rows: the rows of that test (seed 800 + d), the f32 dot products
    rounded once per 32-element slab, MARGIN for the matrix cores' rounding after every product.  The dot products are those
    of am_mmd_rbf_f32 bit for bit (the same engine and slab order), which the last assertion pins: on real-valued rows the
    totals of the cells and the whole-set sums differ by their f64 summation order only."""
    n = m = 1000
    y, x = gi.pair(kind, 800 + d, m, n, d)
    pairs = ka.pair_values(y)
    gamma = 0.5 / float(pairs[ka.lower_median_rank(len(pairs))])     # the kernel width KAD itself would take
    want = mc.unit_sums(x, y, gamma)
    emulated = mc.unit_sums(x, y, gamma, dots=kr.emulated_dots("f32"))
    xt, yt = dev(x), dev(y)
    got = cell_sums(ops, xt, yt, gamma=gamma)
    means = lambda s: ka.device_means([s["xx"].sum(), s["yy"].sum(), s["xy"].sum()], n, m)
    failures = []
    for k, g, w, e in zip(BLOCKS, means(got), means(want), means(emulated)):
        err, limit = abs(g - w), kr.MARGIN * abs(e - w)
        print(f"{kind} D={d} mean {k}: device {g!r} oracle {w!r} |err| {err:.3e} limit {limit:.3e}")
        if not err <= limit:
            failures.append((k, err, limit))
    assert not failures, failures
    whole = ka.device_means(ops.mmd_rbf_sums(xt, yt, gamma=gamma).cpu().numpy(), n, m)
    print(f"{kind} D={d} totals {means(got)!r} am_mmd_rbf_f32 {whole!r}")
    assert (np.abs(means(got) - whole) <= EXACT * want["scale"]).all()


# ---------------------------------------------------------------------------------------------------- 9. a NaN row
def test_a_nan_row_in_x(ops, exact_cases):
    """Exactly the cells of the row's own cell row and column are NaN: row and column 12 of XX, row 12 of XY; every other
    entry, and all of YY, holds the bits of the clean run.  With units: the row and column of its unit."""
    c = exact_cases[100]
    yt = dev(c["y"])
    clean = cell_sums(ops, dev(c["x"]), yt, gamma=GAMMA)
    bad = c["x"].copy()
    victim = 401                                                      # cell 12
    bad[victim, 17] = np.nan
    got = cell_sums(ops, dev(bad), yt, gamma=GAMMA)
    hit = np.zeros((25, 25), dtype=bool)
    hit[12, :] = hit[:, 12] = True
    assert np.array_equal(np.isnan(got["xx"]), hit) and np.array_equal(got["xx"][~hit], clean["xx"][~hit])
    assert np.isnan(got["xy"][12]).all() and np.array_equal(np.delete(got["xy"], 12, 0), np.delete(clean["xy"], 12, 0))
    assert np.array_equal(got["yy"], clean["yy"])
    units = cell_sums(ops, dev(bad), yt, units_x=[0, 5, 12, 13, 25], gamma=GAMMA)
    hit = np.zeros((4, 4), dtype=bool)
    hit[2, :] = hit[:, 2] = True
    assert np.array_equal(np.isnan(units["xx"]), hit) and np.array_equal(np.isnan(units["xy"]), np.repeat(hit[:, :1], 10, 1))
