"""The mathematics and the host logic of the Frechet-distance error bars, without a GPU.

The float64 numpy oracle (tests/fad_stats_reference.py) is checked against what it claims to estimate: leave-one-out
differences of the distance, and the spread of the distance over repeated draws.  Then the package's numpy functions are held
against the oracle, and frechet_distance_with_error / frechet_distance_compare run with hip_ops replaced by the oracle: every
raise fires before a device call, the NaN-and-one-warning cases, labels in any order."""
import types
import warnings

import numpy as np
import pytest
import torch

import fad_stats_reference as fr

D = 8
DRAWS = 300


@pytest.fixture(scope="module")
def fs():
    from audio_metrics_amd.metrics import fad_stats
    return fad_stats


# ------------------------------------------------------------------ the oracle against the quantity it estimates
def test_oracle_maps_are_the_transport_map_and_its_inverse():
    rng = np.random.default_rng(7)
    cx, cy = fr.with_condition(rng, 12, 50.0), fr.with_condition(rng, 12, 80.0, 0.3)
    a, a_inv = fr.maps(cx, cy)
    assert np.abs(a @ cx @ a - cy).max() <= 1e-11 * np.abs(cy).max()
    assert np.abs(a @ a_inv - np.eye(12)).max() <= 1e-11
    assert np.linalg.eigvalsh(a).min() > 0.0
    half, _ = fr.product_powers(cx, cy)
    assert np.abs(cx @ a - half).max() <= 1e-11 * np.abs(half).max()           # (cov_x cov_y)^(1/2) = cov_x A


def test_influence_matches_leave_one_out():
    """(n - 1) (fd - fd without row i) against psi_i for 40 rows of each side, d = 8, 300 x 250 rows.  Measured: correlation
    0.99996 (candidate) and 0.9997 (reference), largest difference 0.66 on a scale of 27 - O(1 / n), as the theory says."""
    rng = np.random.default_rng(100)
    lx, ly = fr.law(rng, D), fr.law(rng, D)
    x, y = fr.draw(rng, 300, lx), fr.draw(rng, 250, ly)
    fd, psi_x, psi_y = fr.influences(x, y)
    sx, sy = fr.stats(x), fr.stats(y)
    loo_x = [(len(x) - 1) * (fd - fr.frechet(*fr.stats(np.delete(x, i, axis=0)), *sy)) for i in range(40)]
    loo_y = [(len(y) - 1) * (fd - fr.frechet(*sx, *fr.stats(np.delete(y, i, axis=0)))) for i in range(40)]
    cx, cy = np.corrcoef(loo_x, psi_x[:40])[0, 1], np.corrcoef(loo_y, psi_y[:40])[0, 1]
    print(f"leave-one-out correlation: candidate {cx:.6f}, reference {cy:.6f}; largest difference "
          f"{np.abs(np.array(loo_x) - psi_x[:40]).max():.3f} on a scale of {np.abs(psi_x[:40]).max():.1f}")
    assert cx >= 0.999 and cy >= 0.999


@pytest.mark.parametrize("n, m", [(400, 500), (2000, 1500)])
def test_calibration_independent_rows(n, m):
    """Mean estimated standard error / empirical standard deviation of the oracle's distance over 300 seeded draws, d = 8.
    Measured: 1.007 at (400, 500), 1.023 at (2000, 1500); the ratio's own noise over 300 draws is about 4 %."""
    rng = np.random.default_rng(200 + n)
    lx, ly = fr.law(rng, D), fr.law(rng, D)
    fds, ses = [], []
    for _ in range(DRAWS):
        fd, psi_x, psi_y = fr.influences(fr.draw(rng, n, lx), fr.draw(rng, m, ly))
        fds.append(fd)
        ses.append(fr.standard_error(psi_x, psi_y))
    ratio = np.mean(ses) / np.std(fds, ddof=1)
    print(f"({n}, {m}): estimated / empirical = {ratio:.3f}")
    assert 0.85 <= ratio <= 1.15


def test_calibration_songs():
    """48 against 40 songs of 16 windows each, the windows 0.3 as wide as the songs, 300 draws.  Measured: the row-level
    estimate is 0.277 of the empirical standard deviation, the cluster-robust one 1.060."""
    rng = np.random.default_rng(300)
    lx, ly = fr.law(rng, D), fr.law(rng, D)
    fds, by_row, by_song = [], [], []
    for _ in range(DRAWS):
        (x, gx), (y, gy) = fr.draw_songs(rng, 48, 16, lx), fr.draw_songs(rng, 40, 16, ly)
        fd, psi_x, psi_y = fr.influences(x, y)
        fds.append(fd)
        by_row.append(fr.standard_error(psi_x, psi_y))
        by_song.append(fr.standard_error(psi_x, psi_y, gx, gy))
    sd = np.std(fds, ddof=1)
    print(f"songs: row-level / empirical = {np.mean(by_row) / sd:.3f}, cluster-robust / empirical = {np.mean(by_song) / sd:.3f}")
    assert 0.85 <= np.mean(by_song) / sd <= 1.15
    assert np.mean(by_row) / sd < 0.5


def test_two_model_test_under_equality():
    """A and B: 600 rows each from ONE law, against a shared 500-row reference, 300 draws.  Measured: z has mean -0.04 and
    standard deviation 0.988; the two-sided 5 % level rejects in 4.7 % of the draws."""
    rng = np.random.default_rng(400)
    lx, ly = fr.law(rng, D), fr.law(rng, D)
    zs, ps = [], []
    for _ in range(DRAWS):
        _, _, t = fr.compare(fr.draw(rng, 600, lx), fr.draw(rng, 600, lx), fr.draw(rng, 500, ly))
        zs.append(t["z"])
        ps.append(t["p_value_two_sided"])
    sd, rate = np.std(zs, ddof=1), float(np.mean(np.array(ps) < 0.05))
    print(f"equal models: z mean {np.mean(zs):.3f}, sd {sd:.3f}, rejection rate {rate:.3f}")
    assert 0.8 <= sd <= 1.2 and rate <= 0.10


# ------------------------------------------------------------------ the package's numpy functions against the oracle
@pytest.fixture(scope="module")
def sample():
    rng = np.random.default_rng(500)
    lx, lb, ly = fr.law(rng, D), fr.law(rng, D), fr.law(rng, D)
    (a, ga), (b, gb), (y, gy) = fr.draw_songs(rng, 12, 9, lx), fr.draw_songs(rng, 10, 11, lb), fr.draw_songs(rng, 14, 8, ly)
    fa, psi_a, psi_ya = fr.influences(a, y)
    fb, psi_b, psi_yb = fr.influences(b, y)
    return dict(a=a, b=b, y=y, ga=ga * 7 - 20, gb=gb, gy=gy + 1000, fa=fa, fb=fb, psi_a=psi_a, psi_b=psi_b, psi_ya=psi_ya, psi_yb=psi_yb)


def test_standard_error_and_difference_test_match_the_oracle(fs, sample):
    s = sample
    for gx, gy in ((None, None), (s["ga"], None), (None, s["gy"]), (s["ga"], s["gy"])):
        assert fs.frechet_standard_error(s["psi_a"], s["psi_ya"], gx, gy) == pytest.approx(fr.standard_error(s["psi_a"], s["psi_ya"], gx, gy), rel=1e-12)
    for ga, gb, gy in ((None, None, None), (s["ga"], s["gb"], s["gy"]), (None, s["gb"], None)):
        got = fs.frechet_difference_test(s["fa"], s["fb"], s["psi_a"], s["psi_b"], s["psi_ya"], s["psi_yb"], ga, gb, gy)
        want = fr.difference_test(s["fa"], s["fb"], s["psi_a"], s["psi_b"], s["psi_ya"], s["psi_yb"], ga, gb, gy)
        assert list(got) == ["difference", "std_error", "z", "p_value", "p_value_two_sided"]
        for key in want:
            assert got[key] == pytest.approx(want[key], rel=1e-12), key
    swapped = fs.frechet_difference_test(s["fb"], s["fa"], s["psi_b"], s["psi_a"], s["psi_yb"], s["psi_ya"])
    plain = fs.frechet_difference_test(s["fa"], s["fb"], s["psi_a"], s["psi_b"], s["psi_ya"], s["psi_yb"])
    assert swapped["z"] == -plain["z"] and swapped["p_value"] == pytest.approx(1.0 - plain["p_value"], abs=1e-15)
    assert plain["p_value_two_sided"] == pytest.approx(2.0 * min(plain["p_value"], 1.0 - plain["p_value"]), rel=1e-12)


def test_labels_in_any_order_give_the_sorted_result(fs, sample):
    s = sample
    perm = np.random.default_rng(1).permutation(len(s["psi_a"]))
    assert fs.frechet_standard_error(s["psi_a"][perm], s["psi_ya"], s["ga"][perm]) == \
        pytest.approx(fs.frechet_standard_error(s["psi_a"], s["psi_ya"], s["ga"]), rel=1e-13)
    relabel = {g: k for k, g in enumerate(sorted(set(s["ga"].tolist()), reverse=True))}       # other values, other order
    other = np.array([relabel[g] for g in s["ga"]])
    assert fs.frechet_standard_error(s["psi_a"], s["psi_ya"], other) == pytest.approx(fs.frechet_standard_error(s["psi_a"], s["psi_ya"], s["ga"]), rel=1e-13)


def test_numpy_functions_raise_and_warn(fs, sample):
    s = sample
    with pytest.raises(ValueError, match="at least 2 units"):
        fs.frechet_standard_error(s["psi_a"], s["psi_ya"], np.zeros(len(s["psi_a"]), dtype=np.int64))
    with pytest.raises(ValueError, match="at least 2 units"):
        fs.frechet_standard_error(s["psi_a"][:1], s["psi_ya"])
    with pytest.raises(ValueError, match="one label per row"):
        fs.frechet_standard_error(s["psi_a"], s["psi_ya"], s["ga"][:-1])
    with pytest.raises(ValueError, match="integer labels"):
        fs.frechet_standard_error(s["psi_a"], s["psi_ya"], s["ga"].astype(np.float64))
    with pytest.raises(ValueError, match="per reference row"):
        fs.frechet_difference_test(1.0, 2.0, s["psi_a"], s["psi_b"], s["psi_ya"], s["psi_yb"][:-1])
    bad = s["psi_a"].copy()
    bad[3] = np.nan
    for call in (lambda: fs.frechet_standard_error(bad, s["psi_ya"]),
                 lambda: fs.frechet_standard_error(np.zeros(5), np.zeros(6))):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            assert np.isnan(call())
        assert len(caught) == 1 and caught[0].category is RuntimeWarning
    for call in (lambda: fs.frechet_difference_test(1.0, 2.0, bad, s["psi_b"], s["psi_ya"], s["psi_yb"]),
                 lambda: fs.frechet_difference_test(1.0, 1.0, s["psi_a"], s["psi_a"], s["psi_ya"], s["psi_ya"])):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            t = call()
        assert len(caught) == 1 and caught[0].category is RuntimeWarning
        assert all(np.isnan(t[k]) for k in ("std_error", "z", "p_value", "p_value_two_sided")) and t["difference"] == t["difference"]


# ------------------------------------------------------------------ the entry points with hip_ops replaced by the oracle
def stub(rows, store=True, n=None):
    """what the entry points read of an AudioMetricsData"""
    rows = np.asarray(rows)
    mean, cov = fr.stats(rows)
    return types.SimpleNamespace(embeddings=torch.as_tensor(rows) if store else None, n=len(rows) if n is None else n,
                                 mean=torch.as_tensor(mean), cov=torch.as_tensor(cov), store_embeddings=store)


@pytest.fixture
def host_ops(fs, monkeypatch):
    """hip_ops.frechet_maps / frechet_influence computed by the oracle on the host; the calls are recorded"""
    import audio_metrics_amd.data as data
    calls = []
    knobs = {"stop": 1, "zero": False}

    def frechet_maps(mu_x, cov_x, mu_y, cov_y, max_iter=64, tol=1e-13):
        calls.append("frechet_maps")
        mu_x, cov_x, mu_y, cov_y = (t.numpy() for t in (mu_x, cov_x, mu_y, cov_y))
        a, a_inv = fr.maps(cov_x, cov_y)
        if knobs["stop"] != 1:
            a, a_inv = np.full_like(a, np.nan), np.full_like(a, np.nan)
        return dict(fd=fr.frechet(mu_x, cov_x, mu_y, cov_y), tr_sqrt=0.0, iters=9, resid=0.0, stop=knobs["stop"],
                    map_xy=torch.as_tensor(a), map_yx=torch.as_tensor(a_inv))

    def frechet_influence(rows, mu, b, lin, c0):
        calls.append("frechet_influence")
        p = fr.psi(rows.numpy().astype(np.float64), mu.numpy(), b.numpy(), lin.numpy(), c0)
        p = np.where(np.isfinite(p), 0.0 if knobs["zero"] else p, np.nan)
        fin = np.isfinite(p)
        return torch.as_tensor(p), torch.as_tensor([p[fin].sum(), (p[fin] ** 2).sum(), float(fin.sum()), float((~fin).sum())])

    monkeypatch.setattr(fs.ops, "frechet_maps", frechet_maps)
    monkeypatch.setattr(fs.ops, "frechet_influence", frechet_influence)
    monkeypatch.setattr(fs.ops, "as_rows", lambda e, name="embeddings": e)
    monkeypatch.setattr(data, "default_device", lambda: torch.device("cpu"))
    return types.SimpleNamespace(calls=calls, knobs=knobs)


def test_entry_points_follow_the_oracle_on_the_host(fs, sample, host_ops):
    s = sample
    a, b, y = stub(s["a"].astype(np.float32)), stub(s["b"]), stub(s["y"])            # a mixed pair: float32 against float64 rows
    fa, psi_a, psi_ya = fr.influences(s["a"].astype(np.float32).astype(np.float64), s["y"])
    got = fs.frechet_distance_with_error(a, y)
    assert list(got) == ["fad", "fad_std_error", "fad_ci_low", "fad_ci_high", "fad_map_residual", "fad_units_candidate", "fad_units_reference"]
    assert got["fad"] == pytest.approx(fa, rel=1e-12) and got["fad_std_error"] == pytest.approx(fr.standard_error(psi_a, psi_ya), rel=1e-9)
    assert got["fad_ci_high"] - got["fad"] == pytest.approx(1.959963984540054 * got["fad_std_error"], rel=1e-9)
    assert got["fad_ci_low"] + got["fad_ci_high"] == pytest.approx(2.0 * got["fad"], rel=1e-12)
    assert 0.0 <= got["fad_map_residual"] < 1e-10
    assert (got["fad_units_candidate"], got["fad_units_reference"]) == (len(s["a"]), len(s["y"]))
    wide = fs.frechet_distance_with_error(a, y, confidence=0.99)
    assert wide["fad_ci_high"] - wide["fad"] == pytest.approx(2.5758293035489004 * got["fad_std_error"], rel=1e-9)
    rows = fs.frechet_distance_with_error(a, y, groups=s["ga"], ref_groups=torch.as_tensor(s["gy"]), return_rows=True)
    assert rows["fad_std_error"] == pytest.approx(fr.standard_error(psi_a, psi_ya, s["ga"], s["gy"]), rel=1e-9)
    assert (rows["fad_units_candidate"], rows["fad_units_reference"]) == (12, 14)
    assert rows["candidate_influence"].shape == (len(s["a"]),) and rows["reference_influence"].shape == (len(s["y"]),)
    assert np.allclose(rows["candidate_influence"], psi_a, rtol=1e-9, atol=1e-9) and np.allclose(rows["reference_influence"], psi_ya, rtol=1e-9, atol=1e-9)
    perm = np.random.default_rng(3).permutation(len(s["a"]))                        # the same rows and labels in another order
    shuffled = fs.frechet_distance_with_error(stub(s["a"].astype(np.float32)[perm]), y, groups=s["ga"][perm], ref_groups=s["gy"])
    assert shuffled["fad_std_error"] == pytest.approx(rows["fad_std_error"], rel=1e-9)
    cmp_ = fs.frechet_distance_compare(a, b, y, groups_a=s["ga"], ref_groups=s["gy"])
    wa, wb, want = fr.compare(s["a"].astype(np.float32).astype(np.float64), s["b"], s["y"], s["ga"], None, s["gy"])
    assert list(cmp_) == ["fad_a", "fad_b", "fad_difference", "fad_difference_std_error", "fad_z", "fad_p_value", "fad_p_value_two_sided"]
    assert cmp_["fad_a"] == pytest.approx(wa, rel=1e-12) and cmp_["fad_b"] == pytest.approx(wb, rel=1e-12)
    for key, name in (("std_error", "fad_difference_std_error"), ("z", "fad_z"), ("p_value", "fad_p_value"), ("p_value_two_sided", "fad_p_value_two_sided")):
        assert cmp_[name] == pytest.approx(want[key], rel=1e-8), key


def test_every_raise_fires_before_a_device_call(fs, sample, host_ops):
    s = sample
    a, y = stub(s["a"]), stub(s["y"])
    one_unit = np.zeros(len(s["a"]), dtype=np.int64)
    cases = [
        (lambda: fs.frechet_distance_with_error(stub(s["a"], store=False), y), "keeps none"),
        (lambda: fs.frechet_distance_with_error(a, stub(s["y"], store=False)), "keeps none"),
        (lambda: fs.frechet_distance_with_error(stub(s["a"], n=len(s["a"]) + 5), y), "statistics describe"),
        (lambda: fs.frechet_distance_with_error(stub(s["a"][:D]), y), "frechet_distance_per_group"),
        (lambda: fs.frechet_distance_with_error(a, stub(s["y"][:D])), "singular"),
        (lambda: fs.frechet_distance_with_error(stub(s["a"][:, :D - 1]), y), "widths differ"),
        (lambda: fs.frechet_distance_with_error(a, y, groups=one_unit), "fewer than 2 units"),
        (lambda: fs.frechet_distance_with_error(a, y, ref_groups=np.zeros(len(s["y"]), dtype=np.int64)), "fewer than 2 units"),
        (lambda: fs.frechet_distance_with_error(a, y, groups=s["ga"][:-1]), "one label per row"),
        (lambda: fs.frechet_distance_with_error(a, y, groups=s["ga"].astype(np.float32)), "integer labels"),
        (lambda: fs.frechet_distance_with_error(a, y, confidence=1.0), "confidence"),
        (lambda: fs.frechet_distance_compare(a, stub(s["b"], store=False), y), "keeps none"),
        (lambda: fs.frechet_distance_compare(a, stub(s["b"][:D]), y), "frechet_distance_per_group"),
        (lambda: fs.frechet_distance_compare(a, stub(s["b"][:, :D - 1]), y), "widths differ"),
        (lambda: fs.frechet_distance_compare(a, stub(s["b"]), y, groups_b=np.zeros(len(s["b"]), dtype=np.int64)), "fewer than 2 units"),
    ]
    for call, words in cases:
        with pytest.raises(ValueError, match=words):
            call()
        assert host_ops.calls == [], words


def one_warning(call):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = call()
    assert len(caught) == 1 and caught[0].category is RuntimeWarning, [str(w.message) for w in caught]
    return out, str(caught[0].message)


def test_nan_and_one_warning_cases(fs, sample, host_ops):
    s = sample
    a, b, y = stub(s["a"]), stub(s["b"]), stub(s["y"])
    error_keys = ("fad_std_error", "fad_ci_low", "fad_ci_high")
    test_keys = ("fad_difference_std_error", "fad_z", "fad_p_value", "fad_p_value_two_sided")
    # a solve that did not converge: no row pass at all
    host_ops.knobs["stop"] = 0
    got, msg = one_warning(lambda: fs.frechet_distance_with_error(a, y, return_rows=True))
    assert "stop code 0" in msg and np.isfinite(got["fad"]) and all(np.isnan(got[k]) for k in error_keys)
    assert np.isnan(got["candidate_influence"]).all() and got["reference_influence"].shape == (len(s["y"]),)
    assert host_ops.calls == ["frechet_maps"]
    got, msg = one_warning(lambda: fs.frechet_distance_compare(a, b, y))
    assert "stop codes 0 and 0" in msg and np.isfinite(got["fad_difference"]) and all(np.isnan(got[k]) for k in test_keys)
    host_ops.knobs["stop"] = 1
    # a row with a non-finite element, through the device sums and through the rows
    rows = s["a"].copy()
    rows[5, 2] = np.inf
    broken = stub(s["a"])
    broken.embeddings = torch.as_tensor(rows)
    for kwargs in ({}, {"groups": s["ga"]}, {"return_rows": True}):
        got, msg = one_warning(lambda: fs.frechet_distance_with_error(broken, y, **kwargs))
        assert "not finite" in msg and np.isfinite(got["fad"]) and all(np.isnan(got[k]) for k in error_keys)
    assert np.isnan(got["candidate_influence"][5]) and np.isfinite(np.delete(got["candidate_influence"], 5)).all()
    got, msg = one_warning(lambda: fs.frechet_distance_compare(a, broken, y))
    assert "not finite" in msg and all(np.isnan(got[k]) for k in test_keys)
    # influence values that vanish throughout (what equal statistics give): a variance of 0, on both routes
    host_ops.knobs["zero"] = True
    for kwargs in ({}, {"return_rows": True}):
        got, msg = one_warning(lambda: fs.frechet_distance_with_error(a, y, **kwargs))
        assert "variance estimate is 0" in msg and np.isfinite(got["fad"]) and all(np.isnan(got[k]) for k in error_keys)
    got, msg = one_warning(lambda: fs.frechet_distance_compare(a, b, y))
    assert "variance estimate is 0" in msg and all(np.isnan(got[k]) for k in test_keys)
    host_ops.knobs["zero"] = False
    # the same object as both models
    host_ops.calls.clear()
    got, msg = one_warning(lambda: fs.frechet_distance_compare(a, a, y))
    assert "same set" in msg and got["fad_difference"] == 0.0 and got["fad_a"] == got["fad_b"] and all(np.isnan(got[k]) for k in test_keys)
