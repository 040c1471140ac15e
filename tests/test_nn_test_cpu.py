"""The nearest-neighbour two-sample test, the part that needs no GPU: nn_permutation_null against the dense reference of
tests/nn_test_reference.py (exact), and the calibration of the test on seeded draws - the graph from the float64 brute-force
reference, the null from the product.

Calibration: 300 draws, 199 relabellings, d = 8, one-sided 5 % level.  A rejection rate of 5 % measured on 300 draws has a
binomial standard deviation of sqrt(0.05 * 0.95 / 300) = 1.26 %; the band 5 % +- 3 of them is [1.2 %, 8.8 %]."""
import numpy as np
import pytest

import nn_test_reference as ref

DRAWS, PERMS, D = 300, 199, 8
BAND = (0.012, 0.088)


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    return audio_metrics_amd


# ---------------------------------------------------------------------------------------------------- the null, exactly
def random_graph(rng, sizes, k, missing):
    """a random graph on units of the given sizes: no neighbour inside the row's own unit, a share of the edges missing"""
    unit = np.repeat(np.arange(len(sizes)), sizes)
    rows = len(unit)
    graph = np.full((rows, k), -1, dtype=np.int64)
    for i in range(rows):
        others = np.flatnonzero(unit != unit[i])
        pick = rng.choice(others, size=k, replace=False)
        pick[rng.random(k) < missing] = -1
        graph[i] = pick
    return unit, np.where(graph >= 0, unit[np.maximum(graph, 0)], -1)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("missing", [0.0, 0.3])
def test_null_equals_the_dense_reference(am, k, missing):
    rng = np.random.default_rng(100 * k + int(10 * missing))
    for sizes, n_x_units in (([1] * 30, 12), ([16] * 9, 5), ([1, 7, 2, 16, 3, 3, 1, 9, 4, 5, 1, 2], 5)):
        unit, neighbor_unit = random_graph(rng, sizes, k, missing)
        for seed in (0, 7):
            want = ref.dense_null(unit, neighbor_unit, n_x_units, 60, seed)
            got = am.nn_permutation_null(unit, neighbor_unit, n_x_units, 60, seed)
            assert got[0] == want[0] and got[2] == want[2], (sizes, got[0], want[0], got[2], want[2])
            assert np.array_equal(got[1], want[1], equal_nan=True)
            assert got[1].dtype == np.float64 and got[1].shape == (60,)


def test_null_in_blocks_of_relabellings(am, monkeypatch):
    from audio_metrics_amd.metrics import nn_test
    rng = np.random.default_rng(3)
    unit, neighbor_unit = random_graph(rng, [4] * 12, 3, 0.1)
    whole = am.nn_permutation_null(unit, neighbor_unit, 5, 50, 1)
    monkeypatch.setattr(nn_test, "PAIR_BLOCK", 7 * 40)                       # a few relabellings per pass, a ragged last block
    parts = am.nn_permutation_null(unit, neighbor_unit, 5, 50, 1)
    assert whole[0] == parts[0] and whole[2] == parts[2] and np.array_equal(whole[1], parts[1])


def test_a_side_without_edges_is_nan_and_exceeds(am):
    # units 0, 1 | 2, 3: only the rows of unit 0 have a neighbour, so every labelling in which unit 0 is not alone on its side ...
    unit = np.array([0, 0, 1, 2, 3])
    neighbor_unit = np.array([[1], [2], [-1], [-1], [-1]])
    t_obs, null, p = am.nn_permutation_null(unit, neighbor_unit, 2, 40, 0)
    assert np.isnan(t_obs) and np.isnan(null).all() and p == 1.0            # one side never has an edge
    want = ref.dense_null(unit, neighbor_unit, 2, 40, 0)
    assert np.isnan(want[0]) and want[2] == 1.0


def test_null_validation(am):
    unit, nb = np.array([0, 0, 1, 2]), np.array([[1], [2], [0], [0]])
    for bad_units in (0, 3, 4):
        with pytest.raises(ValueError, match="n_x_units"):
            am.nn_permutation_null(unit, nb, bad_units)
    with pytest.raises(ValueError, match="n_permutations"):
        am.nn_permutation_null(unit, nb, 1, 0)
    with pytest.raises(ValueError, match="neighbor_unit"):
        am.nn_permutation_null(unit, nb[:3], 1)
    with pytest.raises(ValueError, match="no row belongs to"):
        am.nn_permutation_null(unit, np.array([[1], [2], [0], [3]]), 1)
    with pytest.raises(ValueError, match="unit_of_row"):
        am.nn_permutation_null(unit.astype(np.float64), nb, 1)


# ---------------------------------------------------------------------------------------------------- calibration
def song_rows(rng, songs, windows=16, spread=0.3, shift=0.0):
    """windows of songs: song centres N(shift, I_d), windows N(centre, spread^2 I_d); the label of every row"""
    centres = rng.standard_normal((songs, D)) + shift
    rows = np.repeat(centres, windows, axis=0) + spread * rng.standard_normal((songs * windows, D))
    return rows, np.repeat(np.arange(songs), windows)


def run_draws(am, make, exclusion_by_row=False):
    """(rejection rate at the 5 % level, mean accuracy) over DRAWS seeded draws of make(rng) -> (x, y, groups, ref_groups)"""
    rejected, accuracy = 0, 0.0
    for draw in range(DRAWS):
        x, y, gx, gy = make(np.random.default_rng(1000 + draw))
        unit, n_x_units = ref.pooled_units(len(x), len(y), gx, gy)
        graph, _ = ref.pooled_graph(x, y, 1, np.arange(len(unit)) if exclusion_by_row else unit)
        t_obs, _, p = am.nn_permutation_null(unit, np.where(graph >= 0, unit[np.maximum(graph, 0)], -1), n_x_units, PERMS, draw)
        rejected += p <= 0.05
        accuracy += t_obs
    return rejected / DRAWS, accuracy / DRAWS


def songs_one_law(rng, shift=0.0):
    x, gx = song_rows(rng, 48, shift=shift)
    y, gy = song_rows(rng, 40)
    return x, y, gx, gy


def test_level_on_songs_with_labels(am):
    rate, accuracy = run_draws(am, songs_one_law)
    print("songs, one law, own song excluded: rejection rate %.4f, mean accuracy %.4f" % (rate, accuracy))
    assert BAND[0] <= rate <= BAND[1], rate
    assert abs(accuracy - 0.5) <= 0.02, accuracy


def test_level_on_independent_rows(am):
    def make(rng):
        return rng.standard_normal((400, D)), rng.standard_normal((500, D)), None, None
    rate, accuracy = run_draws(am, make)
    print("independent rows 400 / 500, one law: rejection rate %.4f, mean accuracy %.4f" % (rate, accuracy))
    assert BAND[0] <= rate <= BAND[1], rate


def test_without_the_song_exclusion_the_accuracy_says_nothing(am):
    """the same song data, every row its own unit FOR THE EXCLUSION ONLY (songs are still what is relabelled): a window's
    nearest neighbour is a sibling window, and the accuracy is near 1 for two samples of one law - why labels matter"""
    rate, accuracy = run_draws(am, songs_one_law, exclusion_by_row=True)
    print("songs, one law, only the row excluded: rejection rate %.4f, mean accuracy %.4f" % (rate, accuracy))
    assert accuracy > 0.95, accuracy


def test_power_on_shifted_songs(am):
    rate, accuracy = run_draws(am, lambda rng: songs_one_law(rng, shift=0.5))
    print("songs, candidate mean shifted by 0.5 in every coordinate: rejection rate %.4f, mean accuracy %.4f" % (rate, accuracy))
    assert rate >= 0.6, rate
