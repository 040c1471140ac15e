"""The classifier two-sample test on the device against the float64 oracle of tests/c2st_reference.py: the fused pass
(hip_ops.logit_pass, csrc/logit.hip) within derived rounding bounds at every tile, slab and model-padding edge, its bit-level
invariances, the argument checks, and classifier_two_sample_test end to end.

Bounds, not constants.  With u = 2^-53:
  |z - exact| <= (D + 2) u (sum_d |a_d x_d| + |b|)
  every sum:    (terms + 8) u sum |terms|, plus what the z bound passes on through |dr/dz| <= 1/4 and |dloss/dz| <= 1
(the oracle supplies the absolute sums).  End to end a logit may differ from the oracle's by the distance of the two models,
at most (g_device + g_oracle) / l2 by strong convexity, times sqrt(|x~|^2 + 1), plus the pass bound; the summary figures are
then EQUAL wherever no oracle logit - and no candidate / reference pair of one fold - lies within that distance of a change
of sign.  That precondition is asserted from the oracle alone, before the device is touched; the seeds were chosen so that
it holds for every row."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import c2st_reference as cr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -53
BAD_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -4
ROWS = (1, 63, 64, 65, 129)                    # tile edges
DIMS = (1, 3, 15, 16, 17, 64, 130)             # slab edges (slabs of 32 columns, MFMA steps of 4)
MODELS = (1, 2, 5, 16)                         # model padding
L2, TOL = 1e-3, 1e-8


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    audio_metrics_amd._lib.load()
    return audio_metrics_amd


def wide_ld(d):
    return (d + 3) // 4 * 4 + 4


def on_device(rows, ld=None, poison=float("nan")):
    """the rows on the device with row stride ld (None: as they come), the padding poisoned"""
    t = torch.as_tensor(rows).to(DEV)
    if ld is None:
        return t
    buf = torch.full((t.shape[0], ld), poison, dtype=t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t
    view = buf[:, :t.shape[1]]
    assert view.shape[0] == 1 or view.stride(0) == ld
    return view


def case(n, d, k, seed=0, dtype=np.float32):
    """rows around a mean far from 0, coefficients of mixed sign and size, folds -1..K with one fold left without a row (K >=
    3) and - from 3 rows on - one row with a NaN and one with an inf"""
    rng = np.random.default_rng(1000 * n + 10 * d + k + seed)
    rows = (rng.standard_normal((n, d)) * 1.5 + rng.standard_normal(d)).astype(dtype)
    coef = rng.standard_normal((k, d + 1)) * np.exp(rng.uniform(-2.0, 1.0, (k, 1))) / np.sqrt(d)
    fold = rng.integers(-1, k + 1, n).astype(np.int32)
    if k >= 3:
        fold[fold == 1] = 0                                                         # a fold with no row
    bad = []
    if n >= 3:
        bad = rng.choice(n, 2, replace=False).tolist()
        rows[bad[0], rng.integers(d)] = np.nan
        rows[bad[1], rng.integers(d)] = np.inf
        fold[bad[0]], fold[bad[1]] = 0, k                                           # they would hold out of / train a model
    return rows, coef, fold, bad


def run(am, rows, fold, label, coef, want_z=True):
    sums, z, counts = am.hip_ops.logit_pass(rows, torch.as_tensor(fold).to(DEV), label, torch.as_tensor(coef).to(DEV), want_z=want_z)
    return sums, z, counts


def bits(*tensors):
    return [t.view(torch.int64).cpu().numpy().copy() for t in tensors]


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def check_against_oracle(am, rows, coef, fold, bad, label, ld, what):
    ref = cr.logit_pass(rows, fold, label, coef)
    sums, z, counts = (t.cpu().numpy() for t in run(am, on_device(rows, ld), fold, label, coef))
    n, d = rows.shape
    k = coef.shape[0]
    assert np.array_equal(counts, ref["counts"]), (what, counts, ref["counts"])
    assert np.array_equal(np.isnan(z), np.isnan(ref["z"])), what
    assert all(np.isnan(z[i]) for i in bad)
    own = ~np.isnan(ref["z"])
    idx = np.flatnonzero(own)
    err_z = np.abs(z[own] - ref["z"][own])
    bound_z = cr.z_bound(ref["z_abs"][idx, fold[idx]], d)
    err_s, bound_s = np.abs(sums - ref["sums"]), cr.sums_bound(ref)
    worst_z = float((err_z / bound_z).max()) if len(idx) else 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        worst_s = float(np.nanmax(np.where(bound_s > 0.0, err_s / bound_s, np.where(err_s == 0.0, 0.0, np.inf))))
    print(f"ACCURACY pass {what}: largest error over bound: z {worst_z:.3f}, sums {worst_s:.3f}")
    assert np.isfinite(sums).all(), what
    assert (err_z <= bound_z).all(), (what, worst_z)
    assert (err_s <= bound_s).all(), (what, worst_s)
    empty = ref["terms"] == 0
    assert (sums[empty] == 0.0).all()                                               # a model without training rows


# ------------------------------------------------------------------ 1. the pass against the oracle
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n", ROWS)
def test_pass_within_the_rounding_bounds(am, n, d):
    """every tile edge against every slab edge; the models, the label, the row type and the row stride take turns"""
    turn = ROWS.index(n) * len(DIMS) + DIMS.index(d)
    k = MODELS[turn % 4]
    label = (turn // 4) % 2
    dtype = (np.float32, np.float64)[(turn // 2) % 2]
    ld = (None, wide_ld(d))[(turn // 3) % 2]
    rows, coef, fold, bad = case(n, d, k, dtype=dtype)
    check_against_oracle(am, rows, coef, fold, bad, label, ld, f"N={n} D={d} K={k} label={label} {np.dtype(dtype).name} ld={ld}")


@pytest.mark.parametrize("k", MODELS)
@pytest.mark.parametrize("label", (0, 1))
@pytest.mark.parametrize("dtype", (np.float32, np.float64))
@pytest.mark.parametrize("wide", (False, True))
def test_pass_every_model_count_label_row_type_and_stride(am, k, label, dtype, wide):
    n, d = 129, 17
    rows, coef, fold, bad = case(n, d, k, seed=5, dtype=dtype)
    ld = wide_ld(d) if wide else None
    check_against_oracle(am, rows, coef, fold, bad, label, ld, f"N={n} D={d} K={k} label={label} {np.dtype(dtype).name} ld={ld}")


def test_pass_one_workgroup_takes_two_blocks(am):
    """16 449 rows are 257 blocks of 64 on a grid of 256 workgroups: workgroup 0 takes blocks 0 and 256, the last of one row"""
    n, d, k = 16449, 8, 5
    rows, coef, fold, bad = case(n, d, k)
    fold[-1] = 2
    check_against_oracle(am, rows, coef, fold, bad, 1, None, f"N={n} D={d} K={k}")


# ------------------------------------------------------------------ 2. bits
@pytest.mark.parametrize("n, d, k", [(129, 17, 5), (65, 130, 16), (1, 3, 2), (16449, 8, 5)])
def test_bits_row_types_repeat_models_stride_and_slices(am, n, d, k):
    rows, coef, fold, _ = case(n, d, k, seed=9)
    label = 1
    base = bits(*run(am, on_device(rows), fold, label, coef))
    assert same_bits(base, bits(*run(am, on_device(rows.astype(np.float64)), fold, label, coef)))      # float32 rows and their float64 copies
    assert same_bits(base, bits(*run(am, on_device(rows), fold, label, coef)))                          # two calls
    for dtype in (np.float32, np.float64):                                                              # a wider ld, the padding poisoned
        assert same_bits(base, bits(*run(am, on_device(rows.astype(dtype), wide_ld(d)), fold, label, coef)))
    sums_only, none, counts = run(am, on_device(rows), fold, label, coef, want_z=False)
    assert none is None and same_bits([base[0], base[2]], bits(sums_only, counts))                      # without z_out
    # a row-slice view that starts at a 64-row boundary of a larger matrix
    big = np.concatenate([np.full((128, d), 7.0, dtype=np.float32), rows, np.full((5, d), -3.0, dtype=np.float32)])
    for ld in (None, wide_ld(d)):
        whole = on_device(big, ld)
        assert same_bits(base, bits(*run(am, whole[128:128 + n], fold, label, coef)))
    # fewer models in the call: a model's sums and the logits of its fold are unchanged
    for fewer in sorted({1, min(3, k)}):
        if fewer == k:
            continue
        fold_fewer = np.where(fold < fewer, fold, fewer).astype(np.int32)                               # the other folds train every model
        sums, z, _ = bits(*run(am, on_device(rows), fold_fewer, label, coef[:fewer]))
        assert np.array_equal(sums, base[0][:fewer])
        held = (fold >= 0) & (fold < fewer)
        assert np.array_equal(z[held], base[1][held])
    # a row's logit does not depend on the rows around it
    if n > 70:
        _, z_tail, _ = bits(*run(am, on_device(rows[37:]), fold[37:], label, coef))
        assert np.array_equal(z_tail, base[1][37:])


# ------------------------------------------------------------------ 3. argument checks, no device work
def test_arguments_are_refused_with_the_documented_codes(am):
    lib = am._lib.load()
    n, d, k = 64, 8, 3
    host = (ctypes.c_double * 4096)()
    p = ctypes.cast(host, ctypes.c_void_p)
    nb = lib.am_logit_pass_workspace_bytes(n, d, k)
    assert nb >= 8 * (k * (d + 2) + 2) and lib.am_logit_pass_workspace_bytes(16449, d, k) >= 256 * 8 * (k * (d + 2) + 2)
    assert lib.am_logit_pass_workspace_bytes(16449, d, k) == lib.am_logit_pass_workspace_bytes(10 ** 6, d, k)       # the grid stops at 256

    def call(name="am_logit_pass_f32", x=p, n=n, ld=d, d=d, fold=p, label=1, coef=p, k=k, sums=p, z=p, counts=p, ws=p, nb=nb):
        return getattr(lib, name)(x, n, ld, d, fold, label, coef, k, sums, z, counts, ws, nb, None)

    for name in ("am_logit_pass_f32", "am_logit_pass_f64"):
        assert call(name, n=0) == BAD_SHAPE and call(name, d=0, ld=8) == BAD_SHAPE and call(name, d=8193, ld=8196) == BAD_SHAPE
        assert call(name, ld=4) == BAD_SHAPE                                                            # ld < D
        assert call(name, k=0) == BAD_SHAPE and call(name, k=17) == BAD_SHAPE
        assert call(name, label=2) == BAD_ARG and call(name, label=-1) == BAD_ARG
        for null in ("x", "fold", "coef", "sums", "counts"):
            assert call(name, **{null: None}) == BAD_ARG, (name, null)
        assert call(name, nb=nb - 1) == WORKSPACE and "am_logit_pass_workspace_bytes" in lib.am_last_error().decode()
        assert call(name, ws=None) == WORKSPACE
    assert call("am_logit_pass_f32", ld=10, d=6) == BAD_SHAPE                                           # float32: ld % 4 != 0
    assert call("am_logit_pass_f32", x=ctypes.c_void_p(p.value + 8)) == BAD_SHAPE                       # float32: not 16-byte aligned
    for bad in ((0, d, k), (n, 0, k), (n, 8193, k), (n, d, 0), (n, d, 17)):
        assert lib.am_logit_pass_workspace_bytes(*bad) == 0, bad
    ops = am.hip_ops
    x = torch.zeros((4, 6), device=DEV)
    fold = torch.zeros(4, dtype=torch.int32, device=DEV)
    coef = torch.zeros((2, 7), dtype=torch.float64, device=DEV)
    for args, words in (((x, fold, 2, coef), "label"), ((x, fold, 1, coef[:, :6]), "coef"), ((x, fold[:3], 1, coef), "fold"),
                        ((x, fold.long(), 1, coef), "fold"), ((x, fold, 1, torch.zeros((17, 7), dtype=torch.float64, device=DEV)), "coef")):
        with pytest.raises(ValueError, match=words):
            ops.logit_pass(*args)


# ------------------------------------------------------------------ 4. end to end
E2E_D = 6
E2E_SHIFT = 0.5
E2E_SEEDS = {"rows": 1, "songs": 1}             # chosen on the CPU: the precondition holds, the accuracies are 0.76 and 0.70


def data_of(am, rows, steps=(97, 31, 150)):
    s = am.AudioMetricsData(True, device=DEV)
    k, i = 0, 0
    while k < len(rows):
        s.add(torch.as_tensor(np.ascontiguousarray(rows[k:k + steps[i % len(steps)]])).to(DEV))
        k += steps[i % len(steps)]
        i += 1
    return s


def e2e_case(name, seed=None):
    """float64 rows, d = 6, mean shift 0.5: 300 against 260 independent rows, or 24 against 20 songs of 12 windows with the
    rows - and so the labels - in scrambled order; and the oracle's answers, with its per-row distance bound at g_device = TOL"""
    seed = E2E_SEEDS[name] if seed is None else seed
    rng = np.random.default_rng(7000 + seed)
    law = cr.law(rng, E2E_D)
    if name == "rows":
        x, y, gx, gy = cr.draw(rng, 300, law, E2E_SHIFT), cr.draw(rng, 260, law), None, None
    else:
        (x, gx), (y, gy) = cr.draw_songs(rng, 24, 12, law, 0.5, E2E_SHIFT), cr.draw_songs(rng, 20, 12, law, 0.5)
        px, py = rng.permutation(len(x)), rng.permutation(len(y))
        x, gx, y, gy = x[px], gx[px] * 7 - 30, y[py], gy[py] + 1000
    fold_rng = np.random.default_rng(seed)
    fx = cr.folds(len(x) if gx is None else gx, 5, fold_rng)
    fy = cr.folds(len(y) if gy is None else gy, 5, fold_rng)
    mu, sigma = cr.pooled(x, y)
    thetas, norms, zx, zy = cr.fit(x, y, fx, fy, 5, L2, mu, sigma)
    reach_x = np.sqrt((((x - mu) / sigma) ** 2).sum(axis=1) + 1.0)
    reach_y = np.sqrt((((y - mu) / sigma) ** 2).sum(axis=1) + 1.0)
    return dict(x=x, y=y, gx=gx, gy=gy, fx=fx, fy=fy, mu=mu, sigma=sigma, thetas=thetas, norms=norms, zx=zx, zy=zy, reach_x=reach_x,
                reach_y=reach_y, seed=seed, summary=cr.summary(zx, zy, fx, fy, gx, gy))


def pass_slack(c):
    """the pass bound of a logit in row coordinates, generously: (D + 2) u (sum |a x| + |b|) <= (D + 2) u |theta|_1 (|x|_max / sigma_min + |mu / sigma|_max + 1)"""
    scale = max(np.abs(c["x"]).max(), np.abs(c["y"]).max()) / c["sigma"].min() + np.abs(c["mu"] / c["sigma"]).max() + 1.0
    return (E2E_D + 2) * U * np.abs(c["thetas"]).sum(axis=1).max() * scale * 4.0


def distance_bound(c, g_device):
    """per row: (g_device + g_oracle) / l2 sqrt(|x~|^2 + 1) + the pass bound, with the model of the row's fold"""
    per_model = (g_device + c["norms"]) / L2
    return per_model[c["fx"]] * c["reach_x"] + pass_slack(c), per_model[c["fy"]] * c["reach_y"] + pass_slack(c)


def precondition_holds(c):
    """no oracle logit within its bound of 0, no candidate / reference pair of one fold within their bounds of a tie - from
    the oracle alone, with g_device at its ceiling TOL"""
    bx, by = distance_bound(c, np.full(5, TOL))
    if not ((c["norms"] <= 1e-13).all() and (np.abs(c["zx"]) > bx).all() and (np.abs(c["zy"]) > by).all()):
        return False
    for k in range(5):
        a, b = c["fx"] == k, c["fy"] == k
        gap = np.abs(c["zx"][a][:, None] - c["zy"][b][None, :])
        if not (gap > bx[a][:, None] + by[b][None, :]).all():
            return False
    return True


@pytest.mark.parametrize("name", ["rows", "songs"])
def test_end_to_end_against_the_oracle(am, name):
    c = e2e_case(name)
    assert precondition_holds(c)                                                    # from the oracle alone, before any device call
    cand, ref = data_of(am, c["x"]), data_of(am, c["y"])
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        got = am.classifier_two_sample_test(cand, ref, groups=c["gx"], ref_groups=None if c["gy"] is None else torch.as_tensor(c["gy"]).to(DEV),
                                            folds=5, l2=L2, seed=c["seed"], tol=TOL, return_rows=True)
        plain = am.classifier_two_sample_test(cand, ref, groups=c["gx"], ref_groups=c["gy"], folds=5, l2=L2, seed=c["seed"], tol=TOL)
    assert got["c2st_converged"].all() and (got["c2st_gradient_norm"] <= TOL).all() and got["c2st_rows_nonfinite"] == 0
    assert np.array_equal(got["c2st_candidate_fold"], c["fx"]) and np.array_equal(got["c2st_reference_fold"], c["fy"])
    assert got["c2st_candidate_fold"].dtype == np.int32 and got["c2st_candidate_logit"].dtype == np.float64
    bx, by = distance_bound(c, got["c2st_gradient_norm"])
    ex, ey = np.abs(got["c2st_candidate_logit"] - c["zx"]), np.abs(got["c2st_reference_logit"] - c["zy"])
    print(f"ACCURACY end to end {name}: passes {got['c2st_passes']}, gradient norms {got['c2st_gradient_norm']}, largest logit error "
          f"{max(ex.max(), ey.max()):.3e}, largest error over bound {max((ex / bx).max(), (ey / by).max()):.3e}; accuracy "
          f"{got['c2st_accuracy']!r}, holdout {got['c2st_accuracy_holdout']!r}, z {got['c2st_z']!r}, p {got['c2st_p_value']!r}, auc {got['c2st_auc']!r}")
    assert (ex <= bx).all() and (ey <= by).all()                                    # every row, in stored row order
    for key in ("c2st_accuracy", "c2st_accuracy_holdout", "c2st_z", "c2st_p_value", "c2st_auc", "c2st_holdout_rows"):
        assert got[key] == c["summary"][key], (key, got[key], c["summary"][key])
        assert plain[key] == got[key], key
    assert got["c2st_std_error"] == pytest.approx(c["summary"]["c2st_std_error"], rel=1e-12)
    assert got["c2st_log_loss"] == pytest.approx(c["summary"]["c2st_log_loss"], abs=1e-4)
    assert 0.5 < got["c2st_accuracy"] < 1.0 and 0.5 < got["c2st_auc"] < 1.0
    # the weights are in the coordinates of the rows: they reproduce the logit of a held-out row
    z = c["x"] @ got["c2st_weights"].T + got["c2st_intercepts"]
    assert np.allclose(z[np.arange(len(z)), c["fx"]], got["c2st_candidate_logit"], rtol=0, atol=1e-9)
    assert got["c2st_weights"].shape == (5, E2E_D) and got["c2st_intercepts"].shape == (5,)
    assert "c2st_candidate_logit" not in plain and plain["c2st_passes"] == got["c2st_passes"]


def test_warnings_for_a_non_finite_row_and_for_the_pass_limit(am):
    """float32 rows; row 17 of the candidate set holds a NaN, row 3 of the reference an inf"""
    c = e2e_case("rows")
    x, y = c["x"].astype(np.float32), c["y"].astype(np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        clean = am.classifier_two_sample_test(data_of(am, x), data_of(am, y), seed=c["seed"], return_rows=True)
    assert clean["c2st_converged"].all() and clean["c2st_rows_nonfinite"] == 0
    assert np.abs(clean["c2st_candidate_logit"] - c["zx"]).max() <= 1e-3             # float32 rows: the oracle's model up to the rows' rounding
    x[17, 2], y[3, 5] = np.nan, np.inf
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = am.classifier_two_sample_test(data_of(am, x), data_of(am, y), seed=c["seed"], return_rows=True)
    assert len(caught) == 1 and caught[0].category is RuntimeWarning and "2 row(s)" in str(caught[0].message)
    assert got["c2st_rows_nonfinite"] == 2 and got["c2st_converged"].all()
    assert np.flatnonzero(np.isnan(got["c2st_candidate_logit"])).tolist() == [17] and np.flatnonzero(np.isnan(got["c2st_reference_logit"])).tolist() == [3]
    assert got["c2st_candidate_fold"][17] == -1 and got["c2st_reference_fold"][3] == -1
    assert np.isfinite([got[k] for k in ("c2st_accuracy", "c2st_std_error", "c2st_log_loss", "c2st_auc", "c2st_z", "c2st_p_value")]).all()
    keep = np.arange(len(x)) != 17
    assert np.abs(got["c2st_candidate_logit"][keep] - clean["c2st_candidate_logit"][keep]).max() <= 0.5      # one row of 300 left out
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = am.classifier_two_sample_test(data_of(am, c["x"]), data_of(am, c["y"]), seed=c["seed"], max_passes=3)
    assert len(caught) == 1 and caught[0].category is RuntimeWarning and "have not reached" in str(caught[0].message)
    assert got["c2st_passes"] == 3 and not got["c2st_converged"].any() and np.isfinite(got["c2st_accuracy"])
    with pytest.raises(NotImplementedError, match="mixed pair"):
        am.classifier_two_sample_test(data_of(am, x), data_of(am, c["y"]))
