"""Per-sample fidelity, the part that needs no GPU: fidelity_by_group against a plain Python loop, the argument checks of
sample_fidelity / sample_fidelity_per_group / hip_ops.sample_scores before any device call, the new names in header /
signature table / package, the entry point's error paths and workspace query, and the oracle's own invariants on the
lattice cases of tests/test_gpu_sample_scores.py."""
import ctypes
import math
import os
import re
import statistics

import numpy as np
import pytest
import torch

import fidelity_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -4
FAKE = ctypes.c_void_p(0x10000)                       # 16-byte aligned, never dereferenced: the calls stop at validation
NAMES = ("am_sample_scores_workspace_bytes", "am_sample_scores_chunks", "am_sample_scores_f32")


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    return audio_metrics_amd


@pytest.fixture(scope="module")
def lib(am):
    return am._lib.load()


def host_set(am, rows):
    s = am.AudioMetricsData(True)
    s._embeddings = rows
    return s


# ---------------------------------------------------------------------------------------------------- host aggregation
def loop_by_group(labels, realism, ball_count, rarity, k):
    out = {}
    for g in sorted(set(int(v) for v in labels)):
        rows = [i for i, v in enumerate(labels) if int(v) == g]
        inside = [i for i in rows if ball_count[i] > 0]
        out[g] = (len(rows), len(inside) / len(rows), (1.0 / k) * (sum(int(ball_count[i]) for i in rows) / len(rows)),
                  statistics.median(float(realism[i]) for i in rows),
                  statistics.median(float(rarity[i]) for i in inside) if inside else math.nan)
    return out


def test_fidelity_by_group_matches_a_plain_loop(am):
    rng = np.random.default_rng(5)
    n, k = 500, 5
    labels = rng.integers(-4, 9, size=n) * 7                               # unsorted, negative labels, uneven sizes
    labels[labels == 14] = 21                                              # a label that does not occur
    ball_count = rng.integers(0, 4, size=n).astype(np.int32) * rng.integers(0, 2, size=n).astype(np.int32)
    ball_count[labels == -7] = 0                                           # a group with no in-manifold row
    realism = rng.gamma(2.0, 0.5, size=n).astype(np.float32)
    realism[rng.integers(0, n, size=40)] = np.inf                          # samples that sit on a manifold row
    realism[labels == 35] = np.inf                                         # a group whose median is +inf
    rarity = np.where(ball_count > 0, rng.gamma(2.0, 1.0, size=n), 0.0).astype(np.float32)
    got = am.fidelity_by_group(labels, realism, ball_count, rarity, k)
    want = loop_by_group(labels, realism, ball_count, rarity, k)
    assert list(got["group_labels"]) == sorted(want) and got["group_labels"].dtype == np.int64
    assert -7 in want and math.isnan(want[-7][4]) and math.isinf(want[35][3]) and 14 not in want
    assert got["group_sizes"].sum() == n and got["group_sizes"].dtype == np.int64
    for j, g in enumerate(got["group_labels"]):
        size, prec, dens, real_med, rare_med = want[int(g)]
        assert got["group_sizes"][j] == size
        assert got["precision_per_group"][j] == prec and got["density_per_group"][j] == dens
        assert got["realism_median_per_group"][j] == real_med
        if math.isnan(rare_med):
            assert math.isnan(got["rarity_median_per_group"][j])
        else:
            assert got["rarity_median_per_group"][j] == rare_med
    for name in ("precision_per_group", "density_per_group", "realism_median_per_group", "rarity_median_per_group"):
        assert got[name].dtype == np.float64, name
    # deterministic, and independent of the order the rows come in
    perm = rng.permutation(n)
    again = am.fidelity_by_group(labels[perm], realism[perm], ball_count[perm], rarity[perm], k)
    for name, v in got.items():
        assert np.array_equal(again[name], v, equal_nan=True), name
    # one group, one row
    one = am.fidelity_by_group([3], [np.inf], [2], [0.5], 2)
    assert one["group_labels"].tolist() == [3] and one["precision_per_group"].tolist() == [1.0]
    assert one["density_per_group"].tolist() == [1.0] and one["realism_median_per_group"].tolist() == [np.inf]
    assert one["rarity_median_per_group"].tolist() == [0.5]
    with pytest.raises(ValueError, match="one value per row"):
        am.fidelity_by_group(labels, realism[:-1], ball_count, rarity, k)
    with pytest.raises(ValueError, match="integers"):
        am.fidelity_by_group(labels.astype(np.float64), realism, ball_count, rarity, k)
    with pytest.raises(ValueError, match="at least 1"):
        am.fidelity_by_group(labels, realism, ball_count, rarity, 0)
    with pytest.raises(ValueError, match="not empty"):
        am.fidelity_by_group(np.zeros(0, dtype=np.int64), [], [], [], k)


# ---------------------------------------------------------------------------------------------------- validation
def test_validation_happens_before_any_device_call(am, monkeypatch):
    from audio_metrics_amd import hip_ops

    def forbidden(*a, **k):
        raise AssertionError("device call before validation")
    for name in ("as_matrix", "_call", "_workspace"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    x, y, r = torch.zeros((10, 8)), torch.zeros((12, 8)), torch.zeros(12)
    with pytest.raises(NotImplementedError, match=r"sample_scores takes float32 rows \(the float64 matrix-core form is not implemented\)"):
        hip_ops.sample_scores(x.double(), y, r)
    with pytest.raises(NotImplementedError, match="float32 rows"):
        hip_ops.sample_scores(x, y.double(), r)
    with pytest.raises(ValueError, match="feature widths"):
        hip_ops.sample_scores(x, torch.zeros((12, 12)), r)
    with pytest.raises(ValueError, match="2-D"):
        hip_ops.sample_scores(torch.zeros(8), y, r)
    with pytest.raises(ValueError, match="rows on both sides"):
        hip_ops.sample_scores(x, torch.zeros((0, 8)), torch.zeros(0))
    with pytest.raises(ValueError, match="one radius per row"):
        hip_ops.sample_scores(x, y, r[:11])
    with pytest.raises(ValueError, match="one radius per row"):
        hip_ops.sample_scores(x, y, r.to(torch.float16))
    # the front ends: with the operations they use forbidden too
    for name in ("sample_scores", "knn_radii", "prdc_counts"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    ok, other = host_set(am, x), host_set(am, y)
    groups = np.arange(10) % 3
    calls = (lambda a, b, **kw: am.sample_fidelity(a, b, **kw),
             lambda a, b, **kw: am.sample_fidelity_per_group(a, b, groups[:a.embeddings.shape[0]] if a.embeddings is not None else groups, **kw))
    for call in calls:
        for a, b in ((host_set(am, x.double()), other), (ok, host_set(am, y.double())), (host_set(am, x.double()), host_set(am, y.double()))):
            with pytest.raises(NotImplementedError, match=r"float64 rows; sample_scores takes float32 rows \(the float64 matrix-core form is not implemented\)"):
                call(a, b)
        with pytest.raises(ValueError, match="feature widths"):
            call(ok, host_set(am, torch.zeros((12, 12))))
        with pytest.raises(ValueError, match="keeps none"):
            call(ok, am.AudioMetricsData(False))
        with pytest.raises(ValueError, match="keeps none"):
            call(am.AudioMetricsData(False), other)
        for bad in (0, -3):
            with pytest.raises(ValueError, match="at least 1"):
                call(ok, other, nearest_k=bad)
    with pytest.raises(ValueError, match="one label per row"):
        am.sample_fidelity_per_group(ok, other, np.arange(9))
    with pytest.raises(ValueError, match="integer labels"):
        am.sample_fidelity_per_group(ok, other, np.linspace(0, 1, 10))
    # past the checks the front ends reach the device operations
    with pytest.raises(AssertionError, match="device call before validation"):
        am.sample_fidelity(ok, other)


# ---------------------------------------------------------------------------------------------------- names
def test_header_signature_table_and_package_agree(am, lib):
    with open(os.path.join(ROOT, "include", "audio_metrics_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in am._lib.SIGNATURES and hasattr(lib, name), name
    assert len(am._lib.SIGNATURES["am_sample_scores_f32"][1]) == 16
    from audio_metrics_amd.metrics import fidelity
    assert am.sample_fidelity is fidelity.sample_fidelity and am.sample_fidelity_per_group is fidelity.sample_fidelity_per_group
    assert am.fidelity_by_group is fidelity.fidelity_by_group and am.metrics.fidelity is fidelity
    assert callable(am.hip_ops.sample_scores) and callable(am.hip_ops.sample_scores_chunks)


# ---------------------------------------------------------------------------------------------------- entry point
def test_entry_point_error_paths_and_workspace(lib):
    n, m, d, ld = 130, 300, 40, 40
    nb = lib.am_sample_scores_workspace_bytes(n, m, d)
    assert nb > 0

    def call(x=FAKE, n=n, ldx=ld, y=FAKE, m=m, ldy=ld, d=d, r=FAKE, o1=FAKE, o2=FAKE, o3=FAKE, o4=FAKE, o5=FAKE, ws=FAKE, nb=nb):
        return lib.am_sample_scores_f32(x, n, ldx, y, m, ldy, d, r, o1, o2, o3, o4, o5, ws, nb, None)
    for null in ("x", "y", "r", "o1", "o2", "o3", "o4", "o5"):
        assert call(**{null: None}) == BAD_ARG, null
    assert call(x=ctypes.c_void_p(0x10004)) == BAD_ARG and call(y=ctypes.c_void_p(0x10008)) == BAD_ARG      # alignment
    assert call(ldx=42) == BAD_ARG and call(ldy=36) == BAD_ARG                                              # ld % 4, ld >= D
    assert call(n=0) == BAD_SHAPE and call(m=0) == BAD_SHAPE and call(d=0, ldx=0, ldy=0) == BAD_SHAPE
    assert call(m=2 ** 32 - 1) == BAD_SHAPE
    assert call(nb=nb - 1) == WORKSPACE and call(ws=None) == WORKSPACE
    for bad in ((0, 5, 8), (5, 0, 8), (5, 5, 0), (5, 2 ** 32 - 1, 8)):
        assert lib.am_sample_scores_workspace_bytes(*bad) == 0 and lib.am_sample_scores_chunks(*bad) == 0, bad
    # the plan of the search and the assign
    for shape in ((130, 300, 40), (130, 4000, 40), (100_000, 100_000, 512), (1000, 5, 64)):
        assert lib.am_sample_scores_chunks(*shape) == lib.am_knn_search_chunks(*shape, 1), shape
    assert lib.am_sample_scores_chunks(130, 300, 40) == 3 and lib.am_sample_scores_chunks(130, 4000, 40) == 32
    # row norms, two floats per column, (8 + 8 + 4) bytes per row and chunk - plus alignment
    for n_, m_ in ((130, 300), (1000, 100_000), (100_000, 1000)):
        need = 4 * n_ + 12 * m_ + 20 * n_ * lib.am_sample_scores_chunks(n_, m_, 64)
        got = lib.am_sample_scores_workspace_bytes(n_, m_, 64)
        assert need <= got <= need + 7 * 256, (n_, m_, need, got)


# ---------------------------------------------------------------------------------------------------- the oracle itself
@pytest.mark.parametrize("case", fr.LATTICE_CASES)
def test_the_lattice_cases_are_not_degenerate(case):
    n, m, d, k, duplicates = case
    o = fr.lattice_oracle(*case)
    inside, realism_ties, rarity_ties = fr.check_lattice_is_not_degenerate(o, duplicates)
    print(case, inside, realism_ties, rarity_ties)
    assert 0.5 < inside < 0.9
    realism, realism_index, count, rarity, rarity_index = o["want"]
    assert realism.dtype == np.float32 and rarity.dtype == np.float32 and count.dtype == np.int32
    # the definitions, restated per row in float64 where f32 rounding cannot change the outcome
    r64, d64 = o["r"].astype(np.float64), o["d2"].astype(np.float64)
    assert np.array_equal(count, (np.sqrt(o["d2"]) < o["r"][None, :]).sum(axis=1))          # sqrt_rn(d2) < r, both f32
    assert np.array_equal(count > 0, rarity > 0) and np.array_equal(count > 0, rarity_index >= 0)
    with np.errstate(divide="ignore"):
        ratio = r64[None, :] / np.sqrt(d64)
    assert np.allclose(realism, ratio.max(axis=1), rtol=1e-6)
    rows = np.arange(n)
    assert (realism_index >= 0).all() and np.allclose(ratio[rows, realism_index], ratio.max(axis=1), rtol=1e-6)
    inside_rows = rows[count > 0]
    assert (np.sqrt(o["d2"])[inside_rows, rarity_index[inside_rows]] < o["r"][rarity_index[inside_rows]]).all()
    assert np.array_equal(rarity[inside_rows], o["r"][rarity_index[inside_rows]])
    # a sample inside a ball has realism > 1 towards it; one outside every ball has realism <= 1
    assert (realism[count > 0] > 1).all() and (realism[count == 0] <= 1).all()


def test_the_threshold_is_the_strict_sqrt_test():
    rng = np.random.default_rng(9)
    radii = np.concatenate([rng.gamma(2.0, 2.0, size=300), [1.0, 2.0, 3.0, 1e-3, 1e3, np.sqrt(2.0)]]).astype(np.float32)
    for r in radii:
        t = fr.threshold_of_radius(r)
        below = np.nextafter(t, np.float32(-np.inf))
        assert np.sqrt(t) >= r and np.sqrt(below) < r, (r, t)
    assert fr.threshold_of_radius(np.float32(0)) == 0 and fr.threshold_of_radius(np.float32(-1)) == 0
    assert fr.threshold_of_radius(np.float32(np.nan)) == 0 and np.isposinf(fr.threshold_of_radius(np.float32(np.inf)))
