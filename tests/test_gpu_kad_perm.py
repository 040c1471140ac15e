"""kernel_audio_distance_permutation_test end to end on the device, against the relabel-and-recompute oracle of
tests/mmd_cells_reference.py: exact data, 785 candidate rows against 300 reference rows, D = 32, a fixed bandwidth; the
observed value against kernel_audio_distance, the null and the p-value against the oracle, a shifted candidate set, the label
path and the reference-side cache.

SEED = 4 was picked on the host, among the seeds 0 .. 4: with it no value of the oracle's null lies within 1e-9 of the
observed statistic (the nearest is 2.4e-05 away; the observed value lies inside the null, p = 0.175), so the p-values must
agree exactly."""
import numpy as np
import pytest
import torch

import kd_reference as kr
import mmd_cells_reference as mc

pytestmark = pytest.mark.gpu

EXACT = 1e-12
DEV = "cuda:0"
SIGMA = 10.0
GAMMA = 1.0 / (2.0 * SIGMA * SIGMA)
N, M, D = 785, 300, 32
PERMS, SEED = 199, 4


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


def make_sets():
    rng = np.random.default_rng(6700)
    return kr.rbf_rows(rng, N, D, SIGMA), kr.rbf_rows(rng, M, D, SIGMA)


@pytest.fixture(scope="module")
def sets():
    x, y = make_sets()
    K = mc.pooled_gram(x, y, GAMMA)
    unit = np.concatenate([mc.run_units(N, 32), mc.run_units(M, 32, 25)])
    t_obs, null, p = mc.permutation_null(K, unit, 25, PERMS, SEED)
    return dict(x=x, y=y, K=K, t_obs=t_obs, null=null, p=p, scale=float(np.abs(K).mean()))


def test_against_the_oracle(am, sets):
    cand, ref = data_of(am, sets["x"]), data_of(am, sets["y"])
    plain = am.kernel_audio_distance(cand, data_of(am, sets["y"]), bandwidth=SIGMA)
    got = am.kernel_audio_distance_permutation_test(cand, ref, n_permutations=PERMS, seed=SEED, bandwidth=SIGMA, return_null=True)
    gap = float(np.abs(sets["null"] - sets["t_obs"]).min())
    print(f"mmd2 {got['kad_mmd2']!r} / {plain['kad_mmd2']!r} oracle {sets['t_obs']!r}; p {got['kad_p_value']!r} / {sets['p']!r}; "
          f"nearest null value {gap:.3e}; max null |err| {np.abs(got['kad_null'] - sets['null']).max():.3e}")
    assert gap > 1e-9                                                   # the choice of SEED
    assert got["kad_units"] == (25, 10) and got["kad_n_permutations"] == PERMS and got["kad_bandwidth"] == SIGMA
    assert abs(got["kad_mmd2"] - plain["kad_mmd2"]) <= EXACT * sets["scale"]
    assert abs(got["kad_mmd2"] - sets["t_obs"]) <= 4 * EXACT * sets["scale"] and got["kad"] == 100.0 * got["kad_mmd2"]
    assert got["kad_null"].shape == (PERMS,) and np.abs(got["kad_null"] - sets["null"]).max() <= 1e-10
    assert got["kad_p_value"] == sets["p"]
    np.testing.assert_allclose([got["kad_null_mean"], got["kad_null_std"], got["kad_null_q95"]],
                               [100.0 * sets["null"].mean(), 100.0 * sets["null"].std(ddof=1), 100.0 * np.quantile(sets["null"], 0.95)],
                               rtol=1e-6, atol=1e-8)


def test_a_shifted_candidate_set_gets_the_smallest_p(am, sets):
    shifted = (sets["x"] * np.float32(1.5)).astype(np.float32)         # another scale of the same rows: exact data still
    got = am.kernel_audio_distance_permutation_test(data_of(am, shifted), data_of(am, sets["y"]), n_permutations=PERMS, seed=SEED,
                                                    bandwidth=SIGMA)
    assert got["kad_p_value"] == 1.0 / (PERMS + 1) and got["kad"] > got["kad_null_q95"]


def test_labels_in_shuffled_stored_order(am, sets, monkeypatch):
    """15 songs of 50 rows.  Stored song by song, and stored interleaved (every song's rows in their own order, the songs
    mixed): the position lists name the same rows in the same order, so the pooled matrix has the same bits."""
    from audio_metrics_amd.metrics import kad_perm
    seen = []
    real = kad_perm.mmd_permutation_null

    def recording(G, *a, **k):
        seen.append(G.clone())
        return real(G, *a, **k)
    monkeypatch.setattr(kad_perm, "mmd_permutation_null", recording)
    x = sets["x"][:750]
    ordered_labels = np.repeat(np.arange(15), 50)
    rng = np.random.default_rng(6800)
    mixed_labels = rng.permutation(ordered_labels)
    mixed = np.empty_like(x)
    for s in range(15):
        mixed[mixed_labels == s] = x[ordered_labels == s]
    ref = data_of(am, sets["y"])
    kw = dict(n_permutations=PERMS, seed=SEED, bandwidth=SIGMA, return_null=True)
    a = am.kernel_audio_distance_permutation_test(data_of(am, x), ref, x_groups=ordered_labels * 7 + 3, **kw)
    b = am.kernel_audio_distance_permutation_test(data_of(am, mixed), ref, x_groups=torch.as_tensor(mixed_labels), **kw)
    assert a["kad_units"] == b["kad_units"] == (15, 10) and tuple(seen[0].shape) == (25, 25)
    assert torch.equal(seen[0], seen[1]) and not torch.isnan(seen[0]).any()
    assert a["kad_mmd2"] == b["kad_mmd2"] and np.array_equal(a["kad_null"], b["kad_null"]) and a["kad_p_value"] == b["kad_p_value"]
    # against the oracle, songs as units
    K = mc.pooled_gram(x, sets["y"], GAMMA)
    t_obs, null, p = mc.permutation_null(K, np.concatenate([ordered_labels, mc.run_units(M, 32, 15)]), 15, PERMS, SEED)
    assert abs(a["kad_mmd2"] - t_obs) <= 4 * EXACT * sets["scale"] and np.abs(a["kad_null"] - null).max() <= 1e-10


def test_reference_side_cache(am, sets, monkeypatch):
    from audio_metrics_amd.metrics import kad
    seen = []
    real = am.hip_ops.mmd_rbf_cell_sums

    def counting(*a, **k):
        seen.append(k.get("blocks", 7))
        return real(*a, **k)
    monkeypatch.setattr(am.hip_ops, "mmd_rbf_cell_sums", counting)
    cand, ref = data_of(am, sets["x"]), data_of(am, sets["y"][:250])
    kw = dict(n_permutations=PERMS, seed=SEED, bandwidth=SIGMA, return_null=True)
    first = am.kernel_audio_distance_permutation_test(cand, ref, **kw)
    cache = kad.reference_cache(ref)
    assert list(cache.cells) == [(kad._gamma_bits(GAMMA), 32)] and tuple(cache.cells[(kad._gamma_bits(GAMMA), 32)].shape) == (8, 8)
    assert cache.syy == {} and cache.vrow == {}
    second = am.kernel_audio_distance_permutation_test(cand, ref, **kw)
    assert seen == [7, 5]
    assert second["kad_mmd2"] == first["kad_mmd2"] and np.array_equal(second["kad_null"], first["kad_null"])
    # an append: the entry goes with the rest of the reference side, and the result is that of a fresh reference
    ref.add(torch.as_tensor(np.ascontiguousarray(sets["y"][250:])).to(DEV))
    assert kad.reference_cache(ref).cells == {}
    grown = am.kernel_audio_distance_permutation_test(cand, ref, **kw)
    fresh = am.kernel_audio_distance_permutation_test(cand, data_of(am, sets["y"]), **kw)
    assert seen == [7, 5, 7, 7] and grown["kad_units"] == (25, 10)
    assert grown["kad_mmd2"] == fresh["kad_mmd2"] and np.array_equal(grown["kad_null"], fresh["kad_null"])
    assert grown["kad_mmd2"] != first["kad_mmd2"]
