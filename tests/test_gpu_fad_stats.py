"""The Frechet-distance error bars on the device against the float64 numpy oracle of tests/fad_stats_reference.py:
am_frechet_maps_f64 (the distance bit for bit, the two maps), am_frechet_influence_f32 / _f64 (a derived rounding bound per
row, the device-side sums, bit-level invariances, non-finite rows) and the two public entry points end to end.

Shapes: D in {8, 63, 65, 130, 257} - below one 16-deep k slab, either side of a 64-column tile, three ragged column tiles,
five - and N in {D + 1, 64, 65, 257, 1000} (kept where N > D): one row tile, a tail row tile, several workgroups.

The tolerances of the maps and of the end-to-end figures are MEASURED (profiles/fad_error/accuracy.txt holds the figures of
the run they were taken from) and asserted at 4x the measurement: the arithmetic is deterministic, the margin is for other
seeds.  Every test prints its figures (a line starting with ACCURACY) before it asserts."""
import warnings

import numpy as np
import pytest
import torch

import fad_stats_reference as fr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DIMS = (8, 63, 65, 130, 257)
ROWS = (9, 64, 65, 257, 1000)
U = 2.0 ** -53
MARGIN = 4.0
BAD_SHAPE = -2                   # AM_ERR_BAD_SHAPE

# largest relative errors measured per D (profiles/fad_error/accuracy.txt), covariances of condition number 100:
#   |map_xy map_yx - I|_max,  |A cov_x A - cov_y|_F / |cov_y|_F,  |A - oracle|_F / |oracle|_F,  the same for A^-1
MAPS_MEASURED = {
    8: (9.992e-15, 2.115e-15, 9.374e-15, 1.248e-14),
    63: (1.865e-14, 5.777e-15, 1.334e-14, 1.453e-14),
    65: (2.986e-14, 6.809e-15, 1.338e-14, 1.318e-14),
    130: (3.086e-14, 8.358e-15, 1.895e-14, 2.002e-14),
    257: (5.396e-14, 1.104e-14, 2.337e-14, 2.464e-14),
}
# end to end on float32 rows (the sets' statistics come from the float32 statistics kernels, the oracle's from float64 numpy,
# which is where these figures come from - the row pass itself is checked against its rounding bound above): relative error
# of the standard error (rows or songs as units); largest error of an influence value over the largest |psi|; absolute error
# of z; relative error of the p-values
E2E_MEASURED = {"std_error": 3.656e-09, "rows": 3.259e-08, "z": 6.261e-10, "p": 1.353e-09}


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    audio_metrics_amd._lib.load()
    return audio_metrics_amd


def dev64(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


@pytest.fixture(scope="module")
def solves(am):
    """per D: statistics of condition number 100, the plain solve, the maps solve, and the oracle's maps - computed once"""
    out = {}
    for d in DIMS:
        rng = np.random.default_rng(9000 + d)
        cov_x, cov_y = fr.with_condition(rng, d, 100.0), fr.with_condition(rng, d, 100.0, 0.5)
        mu_x, mu_y = rng.standard_normal(d), rng.standard_normal(d)
        args = [dev64(t) for t in (mu_x, cov_x, mu_y, cov_y)]
        out[d] = dict(mu_x=mu_x, cov_x=cov_x, mu_y=mu_y, cov_y=cov_y, args=args, plain=am.hip_ops.frechet(*args),
                      maps=am.hip_ops.frechet_maps(*args), oracle=fr.maps(cov_x, cov_y))
    return out


# ------------------------------------------------------------------ 1. the solver with its maps
@pytest.mark.parametrize("d", DIMS)
def test_maps_distance_bits_symmetry_and_accuracy(am, solves, d):
    s = solves[d]
    plain, got = s["plain"], s["maps"]
    assert got["stop"] == 1
    for key in ("fd", "tr_sqrt", "iters", "resid"):
        assert got[key] == plain[key], key                                          # bit for bit
    assert abs(got["fd"] - fr.frechet(s["mu_x"], s["cov_x"], s["mu_y"], s["cov_y"])) <= 1e-10 * abs(got["fd"])
    a_dev, inv_dev = got["map_xy"], got["map_yx"]
    assert torch.equal(a_dev, a_dev.T) and torch.equal(inv_dev, inv_dev.T)          # exactly symmetric
    a, a_inv = a_dev.cpu().numpy(), inv_dev.cpu().numpy()
    want_a, want_inv = s["oracle"]
    figures = (np.abs(a @ a_inv - np.eye(d)).max(),
               np.linalg.norm(a @ s["cov_x"] @ a - s["cov_y"]) / np.linalg.norm(s["cov_y"]),
               np.linalg.norm(a - want_a) / np.linalg.norm(want_a),
               np.linalg.norm(a_inv - want_inv) / np.linalg.norm(want_inv))
    print(f"ACCURACY maps D={d}: iters {got['iters']}, |A A^-1 - I|_max {figures[0]:.3e}, |A Cx A - Cy|/|Cy| {figures[1]:.3e}, "
          f"|A - oracle|/|oracle| {figures[2]:.3e}, |A^-1 - oracle|/|oracle| {figures[3]:.3e}")
    assert np.linalg.eigvalsh(a).min() > 0.0
    for value, measured in zip(figures, MAPS_MEASURED[d]):
        assert value <= MARGIN * measured, (figures, MAPS_MEASURED[d])


def test_maps_are_nan_without_convergence_and_the_distance_stays(am, solves):
    s = solves[65]
    capped = am.hip_ops.frechet_maps(*s["args"], max_iter=3)
    plain = am.hip_ops.frechet(*s["args"], max_iter=3)
    assert capped["stop"] == 0 and capped["iters"] >= 3
    assert all(capped[k] == plain[k] for k in ("fd", "tr_sqrt", "iters", "resid")) and np.isfinite(capped["fd"])
    assert torch.isnan(capped["map_xy"]).all() and torch.isnan(capped["map_yx"]).all()


# ------------------------------------------------------------------ 2. the row pass against a derived bound
def influence_case(solves, d, n, dtype=np.float32, seed=0):
    """rows and the DEVICE's own terms of the candidate side: B = I - map_xy, lin = 2 (mu_x - mu_y), a c0 of that scale"""
    s = solves[d]
    rng = np.random.default_rng(100 * d + n + seed)
    rows = (rng.standard_normal((n, d)) * 1.5 + s["mu_x"]).astype(dtype)
    b = torch.eye(d, dtype=torch.float64, device=DEV) - s["maps"]["map_xy"]
    lin = dev64(2.0 * (s["mu_x"] - s["mu_y"]))
    c0 = -float((b * s["args"][1]).sum().item())
    return rows, s["args"][0], b, lin, c0


def oracle_of(rows, mu, b, lin, c0):
    args = (rows.astype(np.float64), mu.cpu().numpy(), b.cpu().numpy(), lin.cpu().numpy(), c0)
    return fr.psi(*args), fr.psi_bound(*args)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n", ROWS)
def test_row_pass_within_the_rounding_bound(am, solves, d, n):
    """An entry of T = C B is D products, the fold adds lin, multiplies by c and sums D terms, c0 is one more addition: in any
    order of summation psi stays within gamma = (2 D + 8) 2^-53 (|c|^T |B| |c| + |lin|^T |c| + |c0|).  The sums: N additions in
    either order differ by at most N 2^-53 sum |psi|."""
    if n <= d:
        n = d + 1
    rows, mu, b, lin, c0 = influence_case(solves, d, n)
    psi, sums = am.hip_ops.frechet_influence(torch.as_tensor(rows).to(DEV), mu, b, lin, c0)
    psi, sums = psi.cpu().numpy(), sums.cpu().numpy()
    want, scale = oracle_of(rows, mu, b, lin, c0)
    gamma = (2 * d + 8) * U * scale
    worst = float(np.max(np.abs(psi - want) / gamma))
    print(f"ACCURACY rows D={d} N={n}: largest |psi_dev - psi_oracle| / gamma = {worst:.3f}")
    assert psi.shape == (n,) and np.isfinite(psi).all()
    assert (np.abs(psi - want) <= gamma).all()
    assert abs(sums[0] - psi.sum()) <= n * U * np.abs(psi).sum()
    assert abs(sums[1] - (psi * psi).sum()) <= n * U * (psi * psi).sum()
    assert sums[2] == n and sums[3] == 0


# ------------------------------------------------------------------ 3. bits
@pytest.mark.parametrize("d", DIMS)
def test_bits_row_types_repeat_tail_tile_and_padding(am, solves, d):
    n = max(65, d + 1)
    rows, mu, b, lin, c0 = influence_case(solves, d, n)
    run = am.hip_ops.frechet_influence
    r32 = torch.as_tensor(rows).to(DEV)
    psi, sums = run(r32, mu, b, lin, c0)
    psi64, sums64 = run(r32.double(), mu, b, lin, c0)
    assert torch.equal(psi, psi64) and torch.equal(sums, sums64)                    # float32 rows and their float64 copies
    again, sums_again = run(r32, mu, b, lin, c0)
    assert torch.equal(psi, again) and torch.equal(sums, sums_again)                # two calls
    head, _ = run(r32[:n - 1], mu, b, lin, c0)                                      # without the last row (N = 65: the tail tile)
    assert torch.equal(psi[:n - 1], head)
    ld = (d + 3) // 4 * 4 + 8
    for dtype in (torch.float32, torch.float64):                                    # a padded ld, the padding poisoned
        buf = torch.full((n, ld), float("nan"), dtype=dtype, device=DEV)
        buf[:, :d] = r32
        view = buf[:, :d]
        assert view.stride(0) == ld
        padded, sums_padded = run(view, mu, b, lin, c0)
        assert torch.equal(psi, padded) and torch.equal(sums, sums_padded)


# ------------------------------------------------------------------ 4. non-finite rows
@pytest.mark.parametrize("poison", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("d, n, row", [(8, 65, 64), (65, 257, 70), (257, 300, 0)])
def test_a_non_finite_row_is_marked_and_left_out(am, solves, d, n, row, poison):
    rows, mu, b, lin, c0 = influence_case(solves, d, n, seed=1)
    clean, _ = am.hip_ops.frechet_influence(torch.as_tensor(rows).to(DEV), mu, b, lin, c0)
    rows[row, d // 2] = poison
    psi, sums = am.hip_ops.frechet_influence(torch.as_tensor(rows).to(DEV), mu, b, lin, c0)
    psi, sums, clean = psi.cpu().numpy(), sums.cpu().numpy(), clean.cpu().numpy()
    assert np.isnan(psi[row])
    keep = np.arange(n) != row
    assert np.array_equal(psi[keep], clean[keep])                                   # that row only, the others bit for bit
    assert sums[2] == n - 1 and sums[3] == 1 and np.isfinite(sums[:2]).all()
    assert abs(sums[0] - psi[keep].sum()) <= n * U * np.abs(psi[keep]).sum()


def test_shape_limits_are_refused(am, solves):
    rows, mu, b, lin, c0 = influence_case(solves, 8, 64)
    lib, ops = am._lib.load(), am.hip_ops
    r32 = torch.as_tensor(rows).to(DEV)
    psi, sums = torch.empty(64, dtype=torch.float64, device=DEV), torch.empty(4, dtype=torch.float64, device=DEV)
    ws = torch.empty(4096, dtype=torch.uint8, device=DEV)
    tail = (ops._ptr(mu), ops._ptr(b), ops._ptr(lin), c0, ops._ptr(psi), ops._ptr(sums), ops._ptr(ws), 4096, None)
    assert lib.am_frechet_influence_f32(ops._ptr(r32), 64, 4, 8, *tail) == BAD_SHAPE      # ld < D
    assert lib.am_frechet_influence_f32(ops._ptr(r32), 32, 10, 8, *tail) == BAD_SHAPE     # ld % 4 != 0
    assert lib.am_frechet_influence_f64(ops._ptr(r32), 1, 8193, 8193, *tail) == BAD_SHAPE  # D > 8192
    assert lib.am_frechet_influence_f32(ops._ptr(r32), 0, 8, 8, *tail) == BAD_SHAPE       # no rows


# ------------------------------------------------------------------ 5. end to end
E2E_D = 65


def data_of(am, rows, steps=(97, 31, 150)):
    s = am.AudioMetricsData(True, device=DEV)
    k, i = 0, 0
    while k < len(rows):
        s.add(torch.as_tensor(np.ascontiguousarray(rows[k:k + steps[i % len(steps)]])).to(DEV))
        k += steps[i % len(steps)]
        i += 1
    return s


@pytest.fixture(scope="module")
def e2e():
    """float32 rows as windows of songs: candidates A (100 songs x 5) and B (110 x 4, the law of A shifted a little) against
    a reference (130 x 5), the windows 0.4 as wide as the songs, mixing matrices near the identity so that the covariances
    are well conditioned and the solve converges - and the oracle's answers on the same values, computed once"""
    rng = np.random.default_rng(6500)
    law_a, law_y = fr.law(rng, E2E_D, 0.03, 0.15), fr.law(rng, E2E_D, 0.03, 0.15)
    law_b = (law_a[0], law_a[1] + 0.04 * rng.standard_normal(E2E_D))
    (a, ga), (b, gb), (y, gy) = fr.draw_songs(rng, 100, 5, law_a, 0.4), fr.draw_songs(rng, 110, 4, law_b, 0.4), fr.draw_songs(rng, 130, 5, law_y, 0.4)
    a, b, y = (t.astype(np.float32) for t in (a, b, y))
    ga, gy = ga[::-1] * 3 + 5, gy + 40                                              # labels of any values, not ascending
    a64, b64, y64 = (t.astype(np.float64) for t in (a, b, y))
    fa, psi_a, psi_ya = fr.influences(a64, y64)
    return dict(a=a, b=b, y=y, ga=ga, gb=gb, gy=gy, fa=fa, psi_a=psi_a, psi_ya=psi_ya,
                plain=fr.compare(a64, b64, y64), grouped=fr.compare(a64, b64, y64, ga, gb, gy))


def rel(got, want):
    return abs(got - want) / abs(want)


def test_with_error_end_to_end(am, e2e):
    cand, ref = data_of(am, e2e["a"]), data_of(am, e2e["y"])
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        plain = am.frechet_distance_with_error(cand, ref)
        rows = am.frechet_distance_with_error(cand, ref, return_rows=True)
        grouped = am.frechet_distance_with_error(cand, ref, groups=e2e["ga"], ref_groups=torch.as_tensor(e2e["gy"]).to(DEV), return_rows=True)
        fad = am.frechet_distance(cand, ref)
    assert plain["fad"] == rows["fad"] == grouped["fad"] == fad                     # no tolerance
    want = fr.standard_error(e2e["psi_a"], e2e["psi_ya"])
    want_grouped = fr.standard_error(e2e["psi_a"], e2e["psi_ya"], e2e["ga"], e2e["gy"])
    scale = np.abs(e2e["psi_a"]).max()
    figures = (rel(plain["fad_std_error"], want), rel(rows["fad_std_error"], want), rel(grouped["fad_std_error"], want_grouped),
               np.abs(rows["candidate_influence"] - e2e["psi_a"]).max() / scale, np.abs(rows["reference_influence"] - e2e["psi_ya"]).max() / scale)
    print(f"ACCURACY with_error D={E2E_D}: fad {fad!r} (oracle {e2e['fa']!r}), se {plain['fad_std_error']!r} (oracle {want!r}); relative "
          f"error of the se from the device sums {figures[0]:.3e}, from the rows {figures[1]:.3e}, by song {figures[2]:.3e}; largest "
          f"row error / largest |psi|: candidate {figures[3]:.3e}, reference {figures[4]:.3e}; map residual {plain['fad_map_residual']:.3e}")
    assert abs(fad - e2e["fa"]) <= 1e-4 * abs(e2e["fa"])
    assert all(v <= MARGIN * E2E_MEASURED["std_error"] for v in figures[:3]), figures
    assert all(v <= MARGIN * E2E_MEASURED["rows"] for v in figures[3:]), figures
    assert want_grouped > 1.5 * want                                                # the windows of a song move together
    assert (plain["fad_units_candidate"], plain["fad_units_reference"]) == (len(e2e["a"]), len(e2e["y"]))
    assert (grouped["fad_units_candidate"], grouped["fad_units_reference"]) == (100, 130)
    z95 = 1.959963984540054
    for got in (plain, grouped):
        assert got["fad_ci_low"] == pytest.approx(got["fad"] - z95 * got["fad_std_error"], rel=1e-13)
        assert got["fad_ci_high"] == pytest.approx(got["fad"] + z95 * got["fad_std_error"], rel=1e-13)
    assert 0.0 <= plain["fad_map_residual"] < 1e-9
    assert rows["candidate_influence"].dtype == np.float64 and rows["candidate_influence"].shape == (len(e2e["a"]),)
    assert rows["reference_influence"].shape == (len(e2e["y"]),)


def test_compare_end_to_end(am, e2e):
    a, b, ref = data_of(am, e2e["a"]), data_of(am, e2e["b"]), data_of(am, e2e["y"])
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        plain = am.frechet_distance_compare(a, b, ref)
        grouped = am.frechet_distance_compare(a, b, ref, groups_a=e2e["ga"], groups_b=e2e["gb"], ref_groups=e2e["gy"])
        swapped = am.frechet_distance_compare(b, a, ref)
        mixed = data_of(am, e2e["y"].astype(np.float64))                            # float64 reference rows: converted per side
        other = am.frechet_distance_compare(a, b, mixed)
    assert plain["fad_a"] == am.frechet_distance(a, ref) and plain["fad_b"] == am.frechet_distance(b, ref)
    assert plain["fad_difference"] == plain["fad_a"] - plain["fad_b"]
    for name, got, (wa, wb, want) in (("rows", plain, e2e["plain"]), ("songs", grouped, e2e["grouped"])):
        figures = (rel(got["fad_difference_std_error"], want["std_error"]), abs(got["fad_z"] - want["z"]),
                   rel(got["fad_p_value"], want["p_value"]), rel(got["fad_p_value_two_sided"], want["p_value_two_sided"]))
        print(f"ACCURACY compare D={E2E_D} by {name}: difference {got['fad_difference']!r} (oracle {want['difference']!r}), z {got['fad_z']!r} "
              f"(oracle {want['z']!r}), p {got['fad_p_value']!r}; relative error of the se {figures[0]:.3e}, error of z {figures[1]:.3e}, "
              f"relative error of p {figures[2]:.3e}, of the two-sided p {figures[3]:.3e}")
        assert figures[0] <= MARGIN * E2E_MEASURED["std_error"] and figures[1] <= MARGIN * E2E_MEASURED["z"]
        assert figures[2] <= MARGIN * E2E_MEASURED["p"] and figures[3] <= MARGIN * E2E_MEASURED["p"]
    assert swapped["fad_z"] == -plain["fad_z"] and swapped["fad_p_value_two_sided"] == plain["fad_p_value_two_sided"]
    assert swapped["fad_p_value"] == pytest.approx(1.0 - plain["fad_p_value"], abs=1e-12)
    assert other["fad_z"] == pytest.approx(plain["fad_z"], abs=1e-3) and other["fad_b"] == pytest.approx(plain["fad_b"], rel=1e-5)


def test_a_solve_that_stops_early_gives_nan_errors_and_one_warning(am, e2e, monkeypatch):
    cand, other, ref = data_of(am, e2e["a"]), data_of(am, e2e["b"]), data_of(am, e2e["y"])
    real = am.hip_ops.frechet_maps
    monkeypatch.setattr(am.hip_ops, "frechet_maps", lambda mu_x, cov_x, mu_y, cov_y, max_iter=64, tol=1e-13: real(mu_x, cov_x, mu_y, cov_y, 3, tol))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = am.frechet_distance_with_error(cand, ref, return_rows=True)
    assert len(caught) == 1 and caught[0].category is RuntimeWarning and "stop code 0" in str(caught[0].message)
    assert np.isfinite(got["fad"]) and all(np.isnan(got[k]) for k in ("fad_std_error", "fad_ci_low", "fad_ci_high", "fad_map_residual"))
    assert np.isnan(got["candidate_influence"]).all() and np.isnan(got["reference_influence"]).all()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = am.frechet_distance_compare(cand, other, ref)
    assert len(caught) == 1 and caught[0].category is RuntimeWarning
    assert np.isfinite(got["fad_difference"]) and all(np.isnan(got[k]) for k in ("fad_difference_std_error", "fad_z", "fad_p_value", "fad_p_value_two_sided"))
