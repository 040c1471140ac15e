"""Numpy-float32 restatement of the leave-group-out PRDC, per-sample scores and authenticity (csrc/sample_scores.hip,
metrics/prdc_groups.py): the oracle of tests/test_gpu_sample_scores_groups.py and tests/test_prdc_groups_cpu.py.  Nothing here
imports the package.

Every function takes f32 matrices of squared distances (exact on lattice rows: fidelity_reference.exact_d2) and integer
labels.  A pair of equal labels is no pair: its squared distance is set to +inf, which makes it no member (nothing is
below a threshold at +inf ... a threshold of +inf included: inf < inf is false), gives it the ratio 0 (r^2 / inf = 0,
inf / inf = NaN -> 0) and takes it out of every minimum."""
import numpy as np

import fidelity_reference as fr

F32 = np.float32


def same_label(gx, gy):
    return np.asarray(gx)[:, None] == np.asarray(gy)[None, :]


def lso_radii(d2_self, g, k):
    """Leave-group-out radii from a self-distance matrix: same-label entries (the row itself among them) set to +inf,
    sorted, column k - 1, sqrt in f32; +inf where fewer than k rows carry another label."""
    d2 = np.where(same_label(g, g), F32(np.inf), np.asarray(d2_self, dtype=F32)).astype(F32)
    if d2.shape[1] < k:
        return np.full(d2.shape[0], np.inf, dtype=F32)
    return np.sqrt(np.sort(d2, axis=1)[:, k - 1].astype(F32))


def scores_groups_from_d2(d2, r, gx, gy):
    """The five outputs of sample_scores_groups: fidelity_reference.scores_from_d2 on the admissible pairs."""
    return fr.scores_from_d2(np.where(same_label(gx, gy), F32(np.inf), np.asarray(d2, dtype=F32)).astype(F32), r)


def nearest_admissible(d2, gx, gy):
    """(sqrt of the smallest admissible d2 of every row in f32, its first column; (+inf, -1) where there is none)."""
    masked = np.where(same_label(gx, gy), F32(np.inf), np.asarray(d2, dtype=F32)).astype(F32)
    masked[np.isnan(masked)] = np.inf
    idx = masked.argmin(axis=1)
    best = masked[np.arange(len(masked)), idx]
    return np.sqrt(best).astype(F32), np.where(np.isfinite(best), idx, -1).astype(np.int64)


def prdc_from_counts(count_cand, recalled, covered, k):
    """The expressions of metrics/prdc.py on integers."""
    n, m = len(count_cand), len(recalled)
    return dict(precision=int((count_cand > 0).sum()) / n, recall=int(recalled.sum()) / m,
                density=(1.0 / float(k)) * (int(count_cand.astype(np.int64).sum()) / n), coverage=int(covered.sum()) / m)


def prdc_plain(d2_rr, d2_cc, d2_cr, k):
    """PRDC with the ordinary k-NN radii (row-only exclusion); d2_cr is [candidate, reference]."""
    r_ref, r_cand = fr.radii_of_d2(d2_rr, k), fr.radii_of_d2(d2_cc, k)
    return _prdc(d2_cr, r_ref, r_cand, None, None, k)


def prdc_leave_group_out(d2_rr, d2_cc, d2_cr, g_ref, g_cand, k, match_across_sets=True, rows=False):
    """PRDC with leave-group-out radii; match_across_sets also skips the cross-set pairs of equal labels."""
    r_ref, r_cand = lso_radii(d2_rr, g_ref, k), lso_radii(d2_cc, g_cand, k)
    if match_across_sets:
        return _prdc(d2_cr, r_ref, r_cand, g_cand, g_ref, k, rows)
    return _prdc(d2_cr, r_ref, r_cand, None, None, k, rows)


def _prdc(d2_cr, r_ref, r_cand, g_cand, g_ref, k, rows=False):
    n, m = d2_cr.shape
    if g_cand is None:
        g_cand, g_ref = np.zeros(n, dtype=np.int64), np.ones(m, dtype=np.int64)          # every pair is admissible
    count = scores_groups_from_d2(d2_cr, r_ref, g_cand, g_ref)[2]
    recalled = scores_groups_from_d2(d2_cr.T, r_cand, g_ref, g_cand)[2] > 0
    nearest, _ = nearest_admissible(d2_cr.T, g_ref, g_cand)
    covered = nearest < r_ref
    out = prdc_from_counts(count, recalled, covered, k)
    if rows:
        out.update(candidate_ball_count=count.astype(np.int32), reference_recalled=recalled, reference_covered=covered)
    return out


def authenticity(d2_gt, d2_tt, g_train=None, g_gen=None):
    """(fraction, authentic bool [M], nearest training row int64 [M]) from d2_gt [generated, training] and the training
    set's self-distances.  Without labels: the nearest training row and that row's nearest OTHER training row (by index).
    With g_train the training row's neighbour carries another label; with g_gen too, so does the generated row's."""
    m, n = d2_gt.shape
    if g_train is None:
        radii = fr.radii_of_d2(d2_tt, 1)
    else:
        radii = lso_radii(d2_tt, g_train, 1)
    if g_gen is None or g_train is None:
        dist, idx = nearest_admissible(d2_gt, np.zeros(m, dtype=np.int64), np.ones(n, dtype=np.int64))
    else:
        dist, idx = nearest_admissible(d2_gt, g_gen, g_train)
    authentic = (idx >= 0) & (dist > radii[np.maximum(idx, 0)])
    return float(authentic.astype(np.int64).mean()), authentic, idx


def song_windows(seed, songs, d, windows=16, spread=0.3):
    """Windowed rows (tests/test_gpu_knn_groups.py: song_windows): `songs` centres ~ N(0, I), `windows` rows each at
    centre + spread * N(0, I); (rows f32, the song of every row)."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((songs, d))
    rows = np.repeat(centres, windows, axis=0) + spread * rng.standard_normal((songs * windows, d))
    return rows.astype(F32), np.repeat(np.arange(songs), windows)


def d2_f64(x, y):
    """Squared distances of real-valued rows in float64 (the demonstration of test_prdc_groups_cpu.py; not bit-exact)."""
    x, y = x.astype(np.float64), y.astype(np.float64)
    return np.maximum((x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2.0 * x @ y.T, 0.0)


def lattice_labels(n, m, d):
    """Labels of a fidelity_reference lattice case: seven values (any int32 values) on both sides, and every second
    near-manifold sample carries the label of the manifold row it was made from."""
    rng = np.random.default_rng(1000 + d + n)
    gy = rng.integers(0, 7, m) * 1000 - 3000
    gx = rng.integers(0, 7, n) * 1000 - 3000
    third = n // 3
    src = (100 + np.arange(third)) % m
    gx[:third:2] = gy[src[::2]]
    return gx, gy


def lattice_oracle(n, m, d, k, duplicates, seed=7):
    """Everything a test needs of one labelled lattice case: rows, labels, leave-group-out radii, the five expected outputs,
    and what keeps the case meaningful - (excluded member pairs, rows whose count changes, realism indices that change,
    rarity indices that change) against the same radii without labels, the share of rows inside some ball, the exact ties."""
    x, y = fr.lattice_case(n, m, d, seed, duplicates)
    gx, gy = lattice_labels(n, m, d)
    r = lso_radii(fr.exact_d2(y, y), gy, k)
    d2 = fr.exact_d2(x, y)
    want, plain = scores_groups_from_d2(d2, r, gx, gy), fr.scores_from_d2(d2, r)
    thr = np.array([fr.threshold_of_radius(v) for v in r], dtype=F32)
    same = same_label(gx, gy)
    effect = (int(((d2 < thr[None, :]) & same).sum()), int((want[2] != plain[2]).sum()), int((want[1] != plain[1]).sum()),
              int((want[4] != plain[4]).sum()))
    ties = fr.tie_counts(np.where(same, F32(np.inf), d2).astype(F32), r)
    return {"x": x, "y": y, "gx": gx, "gy": gy, "r": r, "d2": d2, "want": want, "plain": plain, "effect": effect,
            "inside": float((want[2] > 0).mean()), "ties": ties, "tie_heavy": duplicates}


def check_lattice_is_not_degenerate(case):
    """The preconditions under which a kernel that ignores the labels cannot pass and the tie rule is exercised."""
    pairs, counts, realism_idx, rarity_idx = case["effect"]
    assert pairs >= 50 and counts >= 30 and realism_idx >= 20 and rarity_idx >= 15, case["effect"]
    assert 0.4 < case["inside"] < 0.9, case["inside"]
    assert np.isfinite(case["r"]).all() and (case["r"] > 0).all()
    if case["tie_heavy"]:
        assert case["ties"][0] >= 5 and case["ties"][1] >= 3, case["ties"]
    return case["effect"], case["inside"], case["ties"]


def integer_songs(seed_centres=90, seed_windows=91, songs=10, d=8, windows=8):
    """The exact integer-song recipe of the front-end tests: the same `songs` centres for every seed_windows (the same
    songs on both sides), other windows; labels arange(songs).repeat(windows) * 3 + 100."""
    centres = np.random.default_rng(seed_centres).integers(-3, 4, (songs, d))
    rows = np.repeat(centres, windows, axis=0) + np.random.default_rng(seed_windows).integers(-1, 2, (songs * windows, d))
    return rows.astype(F32), np.arange(songs).repeat(windows) * 3 + 100
