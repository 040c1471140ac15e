"""kernel_audio_distance_with_error and kernel_audio_distance_compare end to end on the device, against the float64 oracle of
tests/mmd_rows_reference.py: exact data, 300 candidate rows against 785 reference rows, D = 100, a fixed bandwidth and the
median one; the reference-side cache; the sign and p-value conventions of the comparison."""
import statistics
import warnings

import numpy as np
import pytest
import torch

import kad_reference as ka
import kd_reference as kr
import mmd_rows_reference as mr

pytestmark = pytest.mark.gpu

EXACT = 1e-12
DEV = "cuda:0"
SIGMA = 10.0
N, NB, M, D = 300, 260, 785, 100


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    audio_metrics_amd._lib.load()
    return audio_metrics_amd


def data_of(am, rows, steps=(97, 31, 150)):
    """an AudioMetricsData filled in batches of uneven size"""
    s = am.AudioMetricsData(True, device=DEV)
    k, i = 0, 0
    while k < len(rows):
        s.add(torch.as_tensor(np.ascontiguousarray(rows[k:k + steps[i % len(steps)]])).to(DEV))
        k += steps[i % len(steps)]
        i += 1
    return s


@pytest.fixture(scope="module")
def sets():
    rng = np.random.default_rng(5700)
    a, b, y = kr.rbf_rows(rng, N, D, SIGMA), kr.rbf_rows(rng, NB, D, SIGMA), kr.rbf_rows(rng, M, D, SIGMA)
    p = ka.pair_values(y)
    median_bw2 = float(ka.as_key(p[ka.lower_median_rank(len(p))]))
    out = dict(a=a, b=b, y=y, median_bw2=median_bw2)
    for name, bw2 in (("fixed", SIGMA * SIGMA), ("median", median_bw2)):
        out[name] = dict(bw2=bw2, a=mr.row_sums(a, y, 0.5 / bw2), b=mr.row_sums(b, y, 0.5 / bw2))
    return out


def bandwidth_of(which):
    return SIGMA if which == "fixed" else None


@pytest.mark.parametrize("which", ["fixed", "median"])
def test_with_error_against_the_oracle(am, sets, which, monkeypatch):
    want = sets[which]["a"]
    scale = want["scale"]
    want_mmd2, want_se = mr.standard_error(want["w"], want["c"], want["v"], want["r"])
    seen = []
    real = am.hip_ops.mmd_rbf_row_sums

    def counting(*a, **k):
        seen.append(k.get("blocks", 7))
        return real(*a, **k)
    monkeypatch.setattr(am.hip_ops, "mmd_rbf_row_sums", counting)
    plain = am.kernel_audio_distance(data_of(am, sets["a"]), data_of(am, sets["y"]), bandwidth=bandwidth_of(which), scale=1000.0)
    cand, ref = data_of(am, sets["a"]), data_of(am, sets["y"])
    got = am.kernel_audio_distance_with_error(cand, ref, bandwidth=bandwidth_of(which), scale=1000.0)
    assert list(got) == ["kad", "kad_mmd2", "kad_bandwidth", "kad_std_error", "kad_ci_low", "kad_ci_high"]
    print(f"{which}: kad {got['kad']!r} / {plain['kad']!r}, se {got['kad_std_error'] / 1000.0!r} / {want_se!r}, scale {scale:.3e}")
    assert got["kad_bandwidth"] == plain["kad_bandwidth"] == np.sqrt(sets[which]["bw2"])
    assert abs(got["kad"] - plain["kad"]) <= EXACT * scale * 1000.0
    assert abs(got["kad_mmd2"] - want_mmd2) <= 4 * EXACT * scale and got["kad"] == 1000.0 * got["kad_mmd2"]
    # each influence value is off by at most 2 EXACT scale; the sample standard deviation is 1-Lipschitz in the max error up to
    # sqrt(n / (n - 1)); 2 (1 / sqrt(n) + 1 / sqrt(m)) <= 2 sqrt(2)
    assert want_se > 0.0 and abs(got["kad_std_error"] / 1000.0 - want_se) <= 8 * EXACT * scale
    # the interval: symmetric about the value, the normal quantile of the confidence wide, proportional to the scale
    q95 = statistics.NormalDist().inv_cdf(0.975)
    assert abs((got["kad_ci_high"] - got["kad"]) - (got["kad"] - got["kad_ci_low"])) <= 1e-12 * abs(got["kad"])
    assert got["kad_ci_high"] - got["kad"] == pytest.approx(q95 * got["kad_std_error"], rel=1e-12)
    # the reference's row sums are cached: the second call carries XX | XY only and returns the same bits
    assert seen == [7]
    assert not getattr(ref, "_kad_cache").syy                          # ... and Syy is left to kernel_audio_distance
    again = am.kernel_audio_distance_with_error(cand, ref, bandwidth=bandwidth_of(which), scale=1000.0)
    assert seen == [7, 5] and again == got
    unit = am.kernel_audio_distance_with_error(cand, ref, bandwidth=bandwidth_of(which), scale=1.0, confidence=0.5)
    assert seen == [7, 5, 5] and unit["kad"] == unit["kad_mmd2"] == got["kad_mmd2"] and 1000.0 * unit["kad_std_error"] == got["kad_std_error"]
    assert unit["kad_ci_high"] - unit["kad"] == pytest.approx(statistics.NormalDist().inv_cdf(0.75) * unit["kad_std_error"], rel=1e-9)
    # kernel_audio_distance on the same reference afterwards: the bits of a reference that never saw the new path
    assert am.kernel_audio_distance(cand, ref, bandwidth=bandwidth_of(which), scale=1000.0) == plain
    # another bandwidth has its own row sums
    am.kernel_audio_distance_with_error(cand, ref, bandwidth=7.0)
    assert seen == [7, 5, 5, 7]


@pytest.mark.parametrize("which", ["fixed", "median"])
def test_compare_against_the_oracle(am, sets, which):
    wa, wb = sets[which]["a"], sets[which]["b"]
    scale = max(wa["scale"], wb["scale"])
    diff, se, z, p, p2 = mr.difference_test(wa["w"], wa["c"], wa["r"], wb["w"], wb["c"], wb["r"])
    a, b, ref = data_of(am, sets["a"]), data_of(am, sets["b"]), data_of(am, sets["y"])
    got = am.kernel_audio_distance_compare(a, b, ref, bandwidth=bandwidth_of(which), scale=1000.0)
    assert list(got) == ["kad_a", "kad_b", "kad_difference", "kad_difference_std_error", "kad_z", "kad_p_value", "kad_p_value_two_sided",
                         "kad_bandwidth"]
    fresh = data_of(am, sets["y"])
    kad_a = am.kernel_audio_distance(a, fresh, bandwidth=bandwidth_of(which), scale=1000.0)
    kad_b = am.kernel_audio_distance(b, fresh, bandwidth=bandwidth_of(which), scale=1000.0)
    print(f"{which}: kad_a {got['kad_a']!r} / {kad_a['kad']!r} kad_b {got['kad_b']!r} / {kad_b['kad']!r} z {got['kad_z']!r} / {z!r} "
          f"se {got['kad_difference_std_error'] / 1000.0!r} / {se!r}")
    assert got["kad_bandwidth"] == kad_a["kad_bandwidth"]
    assert abs(got["kad_a"] - kad_a["kad"]) <= EXACT * scale * 1000.0 and abs(got["kad_b"] - kad_b["kad"]) <= EXACT * scale * 1000.0
    # three terms, each within the standard-error bound 8 EXACT scale
    assert se > 0.0 and abs(got["kad_difference_std_error"] / 1000.0 - se) <= 3 * 8 * EXACT * scale
    # diff is four normalised sums (two of them doubled): 6 EXACT scale;  z = diff / se: |dz| <= |d diff| / se + |z| |d se| / se
    assert abs(got["kad_difference"] / 1000.0 - diff) <= 6 * EXACT * scale
    assert abs(got["kad_z"] - z) <= (6 + 24 * abs(z)) * EXACT * scale / se
    assert got["kad_p_value"] == pytest.approx(p, abs=1e-9) and got["kad_p_value_two_sided"] == pytest.approx(p2, abs=1e-9)
    assert got["kad_difference"] == pytest.approx(got["kad_a"] - got["kad_b"], abs=1e-9 * abs(got["kad_a"]))
    # A and B swapped: the sign of z flips, p -> 1 - p, the two-sided value stays
    back = am.kernel_audio_distance_compare(b, a, ref, bandwidth=bandwidth_of(which), scale=1000.0)
    assert back["kad_z"] == pytest.approx(-got["kad_z"], abs=1e-12) and back["kad_p_value"] == pytest.approx(1.0 - got["kad_p_value"], abs=1e-12)
    assert back["kad_p_value_two_sided"] == pytest.approx(got["kad_p_value_two_sided"], abs=1e-12)
    assert back["kad_a"] == got["kad_b"] and back["kad_b"] == got["kad_a"]


def test_compare_detects_the_closer_model_and_refuses_identical_sets(am):
    """Standard normal rows in 8 dimensions, candidates shifted by 0.4 and by 0.6 per coordinate, bandwidth 4 (gamma = 0.5 /
    (2 d)): the shapes at which the host-side calibration rejects in every one of 300 draws."""
    rng = np.random.default_rng(5800)
    a = (rng.standard_normal((200, 8)) + 0.4).astype(np.float32)
    b = (rng.standard_normal((200, 8)) + 0.6).astype(np.float32)
    y = rng.standard_normal((300, 8)).astype(np.float32)
    sa, sb, ref = data_of(am, a), data_of(am, b), data_of(am, y)
    got = am.kernel_audio_distance_compare(sa, sb, ref, bandwidth=4.0)
    print(got)
    assert got["kad_a"] < got["kad_b"] and got["kad_z"] < -1.645 and got["kad_p_value"] < 0.05
    worse = am.kernel_audio_distance_compare(sb, sa, ref, bandwidth=4.0)
    assert worse["kad_p_value"] > 0.95 and worse["kad_p_value_two_sided"] == pytest.approx(got["kad_p_value_two_sided"], abs=1e-12)
    # A = B: no z, one warning
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        same = am.kernel_audio_distance_compare(sa, data_of(am, a), ref, bandwidth=4.0)
    mine = [r for r in rec if issubclass(r.category, RuntimeWarning)]
    assert len(mine) == 1 and "kernel_audio_distance_compare" in str(mine[0].message), [str(r.message) for r in rec]
    assert same["kad_difference"] == 0.0 and same["kad_a"] == same["kad_b"]
    assert np.isnan(same["kad_z"]) and np.isnan(same["kad_p_value"]) and np.isnan(same["kad_p_value_two_sided"])
