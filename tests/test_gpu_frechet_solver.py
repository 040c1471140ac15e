"""The f64 Newton-Schulz solve (frechet.hip, frechet_batch.hip, ns_engine.h) against independent float64 oracles at the
widths where tile_product changes path, and the iteration budget / block hand-off pinned to a model of the rule.

Every input is an f64 device tensor built by tests/frechet_reference.py: no embeddings, no f32.  The bound SOLVER_REL is
relative to tr Cx + tr Cy and comes from test_frechet_reference_cpu.py, which asserts that a numpy transcription of the
documented iteration meets an eighth of it on these very matrices.  What the widths reach in tile_product (32 x 32 tiles,
16-deep slabs dealt to four waves, two register buffers):
    D % 4 != 0           the scalar operand fetch (the only path for D = 33, 50, 130, ...)
    D = 33, 65, 97       a last tile row / column of width 1
    D = 17, 33, 49, 65   a last slab of one column
    D <= 48              waves that own no slab
    D = 130, 132         nine slabs, ragged last one: the second refill of the double buffer
"""
import numpy as np
import pytest
import torch

import frechet_reference as fr
from test_frechet_reference_cpu import FAD_EXACT_REL, FAD_TERMS_REL, SOLVER_REL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("fd", "tr_sqrt", "iters", "resid")


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    audio_metrics_amd._lib.load()
    return audio_metrics_amd


def dev(*arrays):
    return tuple(torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(DEV) for a in arrays)


def batch_record(am, mx, cx, my, cy, **kw):
    """the five doubles { fd, tr_sqrt, iters, resid, stop } of frechet_batch with B = 1 (shared y)"""
    out = torch.full((1, 5), -7.0, dtype=torch.float64, device=DEV)
    res = am.hip_ops.frechet_batch(mx[None], cx[None], my, cy, out=out, **kw)[0]
    rec = out[0].cpu().tolist()
    assert [res[k] for k in KEYS] + [res["stop"]] == rec[:2] + [int(rec[2]), rec[3], int(rec[4])]
    return rec


def enqueue_record(am, mu_x, cov_x, mu_y, cov_y, max_iter=64, tol=1e-13):
    """the five doubles of am_frechet_enqueue_f64, driven block by block as am_frechet_f64 does"""
    ops, lib = am.hip_ops, am._lib.load()
    d = mu_x.numel()
    nb = lib.am_frechet_workspace_bytes(d)
    ws = torch.empty(nb, dtype=torch.uint8, device=mu_x.device)
    out = torch.zeros(8, dtype=torch.float64, device=mu_x.device)
    first, block = 0, lib.am_frechet_first_block()
    while first < max_iter:
        n_iter = min(block, max_iter - first)
        ops._call(lib, "am_frechet_enqueue_f64", mu_x.device, ops._ptr(mu_x), ops._ptr(cov_x), ops._ptr(mu_y), ops._ptr(cov_y), d,
                  first, n_iter, max_iter, tol, ops._ptr(out), ops._ptr(ws), nb)
        rec = out.cpu().tolist()
        first += n_iter
        if int(rec[4]) != 0:
            break
    return rec[:5]


def check_against(tag, rec, fd, tr, bound, stops):
    print(f"{tag}: fd err {abs(rec[0] - fd):.3e} tr_sqrt err {abs(rec[1] - tr):.3e} bound {bound:.3e} "
          f"iters {int(rec[2])} resid {rec[3]:.2e} stop {int(rec[4])}")
    assert int(rec[4]) in stops, (tag, rec)
    assert abs(rec[0] - fd) <= bound and abs(rec[1] - tr) <= bound, (tag, rec, fd, tr)


# ------------------------------------------------------------------ 1. closed form at every edge
@pytest.mark.parametrize("cond", fr.COND)
@pytest.mark.parametrize("d", fr.D_EDGES)
def test_closed_form_at_every_tile_edge(am, d, cond):
    mu_x, cx, mu_y, cy, tr = fr.commuting_pair(d, cond, 0)
    fd, bound = fr.fd_closed(mu_x, cx, mu_y, cy, tr), SOLVER_REL * fr.solver_scale(cx, cy)
    t = dev(mu_x, cx, mu_y, cy)
    single = am.hip_ops.frechet(*t)
    rec = batch_record(am, *t)
    check_against(f"D={d} cond={cond:g} batch", rec, fd, tr, bound, (1, 2))
    check_against(f"D={d} cond={cond:g} single", [single[k] for k in KEYS] + [rec[4]], fd, tr, bound, (1, 2))
    _, m_iters, m_stop, _ = fr.ns_model(cx, cy)
    if m_stop == 1 and int(rec[4]) == 1:
        assert abs(int(rec[2]) - m_iters) <= 1 and abs(single["iters"] - m_iters) <= 1, (rec, m_iters)


# ------------------------------------------------------------------ 2. general and rank-deficient pairs
@pytest.mark.parametrize("d", fr.GENERAL_D)
def test_full_rank_sample_covariances(am, d):
    p = fr.sample_pair(d, 4 * d, 4 * d, 1)
    fd, tr = fr.fd_psd(*p)
    bound = SOLVER_REL * fr.solver_scale(p[1], p[3])
    t = dev(*p)
    single = am.hip_ops.frechet(*t)
    rec = batch_record(am, *t)
    check_against(f"general D={d} batch", rec, fd, tr, bound, (1, 2))
    check_against(f"general D={d} single", [single[k] for k in KEYS] + [rec[4]], fd, tr, bound, (1, 2))


@pytest.mark.parametrize("d, rows_x, rows_y", fr.RANK_DEFICIENT)
def test_rank_deficient_pairs_stop_on_the_trace(am, d, rows_x, rows_y):
    p = fr.sample_pair(d, rows_x, rows_y, 0)
    fd, tr = fr.fd_psd(*p)
    bound = FAD_EXACT_REL * abs(fd) + FAD_TERMS_REL * fr.solver_scale(p[1], p[3])
    t = dev(*p)
    single = am.hip_ops.frechet(*t)
    rec = batch_record(am, *t)
    check_against(f"rank-deficient D={d} rows {rows_x}/{rows_y} batch", rec, fd, tr, bound, (2,))
    check_against(f"rank-deficient D={d} rows {rows_x}/{rows_y} single", [single[k] for k in KEYS] + [rec[4]], fd, tr, bound, (2,))


# ------------------------------------------------------------------ 3. degenerate pairs
@pytest.mark.parametrize("d", fr.DEGENERATE_D)
def test_zero_covariance_is_stop_3_and_exact(am, d):
    mu_x, mu_y, cy = fr.dyadic_pair(d, 0)
    cx = np.zeros((d, d))
    want = fr.fd_of(mu_x, cx, mu_y, cy, 0.0)                   # every term a multiple of 2^-20: exact in any order
    t = dev(mu_x, cx, mu_y, cy)
    rec = batch_record(am, *t)
    single = am.hip_ops.frechet(*t)
    assert int(rec[4]) == 3 and rec[1] == 0.0 and rec[0] == want, (rec, want)
    assert single["tr_sqrt"] == 0.0 and single["fd"] == want
    assert enqueue_record(am, *t) == rec
    # and with x and y exchanged (Cy = 0): the product is the same zero
    t = dev(mu_y, cy, mu_x, cx)
    rec = batch_record(am, *t)
    assert int(rec[4]) == 3 and rec[1] == 0.0 and rec[0] == want


@pytest.mark.parametrize("d", fr.DEGENERATE_D)
def test_equal_covariances_leave_the_mean_term(am, d):
    mu_x, cx, mu_y, _, _ = fr.commuting_pair(d, fr.EQUAL_PAIR_COND, 0)
    t = dev(mu_x, cx, mu_y, cx)
    rec = batch_record(am, *t)
    single = am.hip_ops.frechet(*t)
    bound = SOLVER_REL * 2.0 * float(np.trace(cx))
    dmu = float(((mu_x - mu_y) ** 2).sum())
    print(f"Cx = Cy D={d}: fd - |dmu|^2 = {rec[0] - dmu:.3e} (bound {bound:.3e}) stop {int(rec[4])}")
    assert int(rec[4]) in (1, 2)
    assert abs(rec[0] - dmu) <= bound and abs(rec[1] - np.trace(cx)) <= bound
    assert [single[k] for k in KEYS] == [rec[0], rec[1], int(rec[2]), rec[3]]


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("d", fr.DEGENERATE_D)
def test_non_finite_entry_is_an_error_and_stop_4(am, d, bad):
    mu_x, cx, mu_y, cy, _ = fr.commuting_pair(d, 1e4, 0)
    cx = cx.copy()
    cx[d - 1, d // 2] = bad
    t = dev(mu_x, cx, mu_y, cy)
    with pytest.raises(am._lib.HipLibraryError):
        am.hip_ops.frechet(*t)
    out = torch.full((1, 5), -7.0, dtype=torch.float64, device=DEV)
    with pytest.raises(am._lib.HipLibraryError, match="set 0"):
        am.hip_ops.frechet_batch(t[0][None], t[1][None], t[2], t[3], out=out)
    assert int(out[0, 4].item()) == 4
    with pytest.raises(am._lib.HipLibraryError):
        am.hip_ops.frechet_async(*t).result()


# ------------------------------------------------------------------ 4. iteration budget and block hand-off
@pytest.fixture(scope="module")
def budget_case(am):
    d, cond, seed = fr.BUDGET_PAIR
    mu_x, cx, mu_y, cy, tr = fr.commuting_pair(d, cond, seed)
    t = dev(mu_x, cx, mu_y, cy)
    model = {b: fr.ns_model(cx, cy, max_iter=b) for b in fr.BUDGETS}
    recs = {b: batch_record(am, *t, max_iter=b) for b in fr.BUDGETS}
    return t, fr.solver_scale(cx, cy), model, recs


def test_budget_ends_where_the_model_says(budget_case):
    _, scale, model, recs = budget_case
    spent = [b for b in fr.BUDGETS if model[b][2] == 0]
    assert spent == [1, 2, 15, 16, 17]
    for b in fr.BUDGETS:
        m_tr, m_iters, m_stop, _ = model[b]
        rec = recs[b]
        print(f"budget {b}: device tr_sqrt {rec[1]!r} iters {int(rec[2])} stop {int(rec[4])}; model {m_tr!r} {m_iters} {m_stop}")
        if m_stop == 0:
            assert int(rec[4]) == 0 and int(rec[2]) == b + 1, (b, rec)
        else:
            assert int(rec[4]) == 1 and abs(int(rec[2]) - m_iters) <= 1, (b, rec)
        assert abs(rec[1] - m_tr) <= SOLVER_REL * scale, (b, rec, m_tr)
    traces = [recs[b][1] for b in fr.BUDGETS]
    assert all(hi >= lo for lo, hi in zip(traces, traces[1:])), traces
    assert recs[31] == recs[32] == recs[64]


@pytest.mark.parametrize("budget", [16, 17, 64])
def test_every_entry_point_hands_blocks_over_alike(am, budget_case, budget):
    """16: one block that is also the last; 17: a second block of one iteration; 64: the solve converges in the second
    block, so am_frechet_f64's loop, FrechetJob.result's continuation and the batch's loop each enqueue twice."""
    t, _, _, recs = budget_case
    rec = recs[budget]
    single = am.hip_ops.frechet(*t, max_iter=budget)
    job = am.hip_ops.frechet_async(*t, max_iter=budget).result()
    assert [single[k] for k in KEYS] == [rec[0], rec[1], int(rec[2]), rec[3]]
    assert [job[k] for k in KEYS] == [rec[0], rec[1], int(rec[2]), rec[3]]
    assert enqueue_record(am, *t, max_iter=budget) == rec
    per_set = am.hip_ops.frechet_batch(t[0][None], t[1][None], t[2][None], t[3][None], max_iter=budget)[0]
    assert [per_set[k] for k in KEYS] + [per_set["stop"]] == [rec[0], rec[1], int(rec[2]), rec[3], int(rec[4])]


# ------------------------------------------------------------------ 5. operand alignment
@pytest.mark.parametrize("d", [32, 100])
def test_covariance_one_double_into_a_buffer(am, d):
    """D % 4 == 0 with a base that is 8-byte aligned only: the vector fetch must not be taken, and the scalar fetch reads the
    same numbers, so the record is the aligned call's."""
    mu_x, cx, mu_y, cy, tr = fr.commuting_pair(d, 1e4, 0)
    t = dev(mu_x, cx, mu_y, cy)
    aligned = batch_record(am, *t)
    flat_x = torch.zeros(d * d + 1, dtype=torch.float64, device=DEV)
    flat_y = torch.zeros(d * d + 1, dtype=torch.float64, device=DEV)
    off_x, off_y = flat_x[1:].view(d, d), flat_y[1:].view(d, d)
    off_x.copy_(t[1])
    off_y.copy_(t[3])
    assert off_x.is_contiguous() and off_x.data_ptr() % 32 == 8 and am.hip_ops._f64(off_x, "cov").data_ptr() == off_x.data_ptr()
    for cov_x, cov_y in ((off_x, t[3]), (t[1], off_y), (off_x, off_y)):
        assert batch_record(am, t[0], cov_x, t[2], cov_y) == aligned
        single = am.hip_ops.frechet(t[0], cov_x, t[2], cov_y)
        assert [single[k] for k in KEYS] == [aligned[0], aligned[1], int(aligned[2]), aligned[3]]
    assert abs(aligned[1] - tr) <= SOLVER_REL * fr.solver_scale(cx, cy)


# ------------------------------------------------------------------ 6. exact scaling
@pytest.mark.parametrize("e", [40, -40])
@pytest.mark.parametrize("d", [33, 64])
def test_powers_of_two_scale_exactly(am, d, e):
    """Covariances times 2^e and means times 2^(e/2): the product scales by 2^(2e), its norm by the same (an even power, so
    the square roots are exact too), the normalised iterate is unchanged bit for bit, and fd and tr_sqrt scale by 2^e."""
    mu_x, cx, mu_y, cy, _ = fr.commuting_pair(d, 1e4, 0)
    base = batch_record(am, *dev(mu_x, cx, mu_y, cy))
    s, h = 2.0 ** e, 2.0 ** (e // 2)
    rec = batch_record(am, *dev(mu_x * h, cx * s, mu_y * h, cy * s))
    assert rec[2:] == base[2:], (rec, base)
    assert rec[0] == base[0] * s and rec[1] == base[1] * s, (rec, base)


# ------------------------------------------------------------------ 7. batches
def batch_bound(kind, fd, cx, cy):
    scale = fr.solver_scale(cx, cy)
    return FAD_EXACT_REL * abs(fd) + FAD_TERMS_REL * scale if kind == "rank" else SOLVER_REL * scale


BATCH_STOPS = {"well": (1, 2), "rank": (2,), "zero": (3,), "cond": (1, 2), "same": (1, 2)}


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("d", fr.BATCH_D)
def test_batch_of_five_kinds(am, monkeypatch, d, shared, split):
    sets = fr.batch_sets(d, shared)
    b = len(sets)
    mu_x, cov_x = (torch.stack(dev(*[s[k] for s in sets])) for k in (1, 2))
    if shared:
        mu_y, cov_y = dev(sets[0][3], sets[0][4])
    else:
        mu_y, cov_y = (torch.stack(dev(*[s[k] for s in sets])) for k in (3, 4))
    if split:
        per_set = max(int(am._lib.load().am_frechet_batch_workspace_bytes(1, d)), 1)
        monkeypatch.setattr(am.hip_ops, "FRECHET_BATCH_WS_CAP", 2 * per_set + per_set // 2)
        chunk = max(1, min(b, am.hip_ops.FRECHET_BATCH_WS_CAP // per_set))          # as frechet_batch computes it
        assert chunk == 2 and b > 2 * chunk                                       # chunks of 2, 2 and 1 sets
    out = torch.full((b, 5), -7.0, dtype=torch.float64, device=DEV)
    got = am.hip_ops.frechet_batch(mu_x, cov_x, mu_y, cov_y, out=out)
    recs = out.cpu().tolist()
    again = am.hip_ops.frechet_batch(mu_x, cov_x, mu_y, cov_y)
    assert again == got
    for i, (kind, mx, cx, my, cy, fd, tr) in enumerate(sets):
        assert [got[i][k] for k in KEYS] + [got[i]["stop"]] == [recs[i][0], recs[i][1], int(recs[i][2]), recs[i][3], int(recs[i][4])]
        check_against(f"B=5 D={d} shared={shared} split={split} {kind}", recs[i], fd, tr, batch_bound(kind, fd, cx, cy), BATCH_STOPS[kind])
        if kind == "zero":
            assert recs[i][1] == 0.0
        t = dev(mx, cx, my, cy)
        assert enqueue_record(am, *t) == recs[i], (kind, recs[i])
        single = am.hip_ops.frechet(*t)
        assert [single[k] for k in KEYS] == [recs[i][0], recs[i][1], int(recs[i][2]), recs[i][3]]
