"""Leave-group-out PRDC and per-sample fidelity, the part that needs no GPU: the oracle's own identities
(tests/prdc_groups_reference.py), every error that is raised before a device call, the new names in header / signature
table / package, the C entry's error codes and workspace query, and the demonstration that motivates the feature - in numpy
float64 on windowed rows, what the plain k-NN manifold, leave-group-out radii alone and radii plus matched pairs report."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import fidelity_reference as fr
import prdc_groups_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -4
FAKE = ctypes.c_void_p(0x10000)                       # 16-byte aligned, never dereferenced: the calls stop at validation
NAMES = ("am_sample_scores_groups_workspace_bytes", "am_sample_scores_groups_f32")


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


def forbidden(*a, **k):
    raise AssertionError("device call before validation")


# ---------------------------------------------------------------------------------------------------- the oracle's identities
def test_oracle_identities():
    n, m, d, k = 130, 300, 40, 5
    x, y = fr.lattice_case(n, m, d, 7)
    d2_self, d2 = fr.exact_d2(y, y), fr.exact_d2(x, y)
    # one label per row: the row itself is left out and nothing else
    for kk in (1, 3, 5):
        assert np.array_equal(pr.lso_radii(d2_self, np.arange(m) * 3 - 50, kk), fr.radii_of_d2(d2_self, kk))
    # disjoint labels: nothing is left out
    r = fr.radii_of_d2(d2_self, k)
    got, want = pr.scores_groups_from_d2(d2, r, np.arange(n) % 9, 100 + np.arange(m) % 11), fr.scores_from_d2(d2, r)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    # one label on everything: nothing is left
    got = pr.scores_groups_from_d2(d2, r, np.zeros(n, dtype=int), np.zeros(m, dtype=int))
    assert not got[0].any() and (got[1] == -1).all() and not got[2].any() and not got[3].any() and (got[4] == -1).all()
    # a label that leaves fewer than k rows outside it has no radius
    g = np.zeros(m, dtype=int)
    g[:3] = 1
    assert np.isposinf(pr.lso_radii(d2_self, g, 5)[3:]).all() and np.isfinite(pr.lso_radii(d2_self, g, 5)[:3]).all()
    # PRDC: disjoint label values make the two settings one, and unmatched is the plain definition on the same radii
    ref, g_ref = pr.integer_songs(90, 91)
    cand, _ = pr.integer_songs(90, 92)
    rr, cc, cr = fr.exact_d2(ref, ref), fr.exact_d2(cand, cand), fr.exact_d2(cand, ref)
    assert pr.prdc_leave_group_out(rr, cc, cr, g_ref, g_ref + 10000, 3, True) == pr.prdc_leave_group_out(rr, cc, cr, g_ref, g_ref, 3, False)
    own = np.arange(80)
    assert pr.prdc_leave_group_out(rr, cc, cr, own, own + 1000, 3, True) == pr.prdc_plain(rr, cc, cr, 3)


def test_labelled_lattice_cases_are_not_degenerate():
    """The figures the GPU test's preconditions stand on, without a GPU."""
    want = {(130, 300, 40): (106, 63, 38, 22), (130, 300, 64): (81, 49, 40, 26), (257, 130, 40): (217, 116, 74, 29),
            (130, 4000, 40): (135, 65, 36, 24)}
    for c in fr.LATTICE_CASES:
        case = pr.lattice_oracle(*c)
        effect, inside, ties = pr.check_lattice_is_not_degenerate(case)
        assert effect == want[c[:3]] and 0.57 < inside < 0.77, (c, effect, inside)
        if c[4]:
            assert ties == (9, 5)


# ---------------------------------------------------------------------------------------------------- validation
def test_raw_op_validates_before_any_device_call(monkeypatch):
    from audio_metrics_amd import hip_ops
    for name in ("as_matrix", "_call", "_workspace"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    x, y, r = torch.zeros((10, 8)), torch.zeros((12, 8)), torch.zeros(12)
    gx, gy = torch.zeros(10, dtype=torch.int32), torch.zeros(12, dtype=torch.int32)
    f = hip_ops.sample_scores_groups
    with pytest.raises(NotImplementedError, match=r"sample_scores_groups takes float32 rows"):
        f(x.double(), y, r, gx, gy)
    with pytest.raises(NotImplementedError, match="float32 rows"):
        f(x, y, r.double(), gx, gy)
    with pytest.raises(ValueError, match="2-D"):
        f(x[0], y, r, gx, gy)
    with pytest.raises(ValueError, match="feature widths"):
        f(x, torch.zeros((12, 12)), r, gx, gy)
    with pytest.raises(ValueError, match="rows on both sides"):
        f(x[:0], y, r, gx[:0], gy)
    with pytest.raises(ValueError, match="one radius per row of y"):
        f(x, y, r[:11], gx, gy)
    with pytest.raises(ValueError, match="x_group must be an int32 tensor"):
        f(x, y, r, gx.long(), gy)
    with pytest.raises(ValueError, match="y_group must be an int32 tensor"):
        f(x, y, r, gx, np.zeros(12, dtype=np.int32))
    with pytest.raises(ValueError, match="x_group must hold one label per row"):
        f(x, y, r, gx[:9], gy)
    with pytest.raises(ValueError, match="y_group must hold one label per row"):
        f(x, y, r, gx, gy.reshape(12, 1))
    with pytest.raises(ValueError, match="x_group lives on"):
        f(x, y, r, gx.to("meta"), gy)


def test_front_ends_validate_before_any_device_call(am, monkeypatch):
    from audio_metrics_amd import hip_ops
    for name in ("as_matrix", "_call", "_workspace", "knn_search", "knn_search_groups", "sample_scores", "sample_scores_groups",
                 "prdc_counts", "knn_radii", "upload_host_array"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    ok, other = host_set(am, torch.zeros((10, 8))), host_set(am, torch.zeros((12, 8)))
    f64 = host_set(am, torch.zeros((12, 8), dtype=torch.float64))
    g10, g12 = np.arange(10) // 2, np.arange(12) // 3
    # leave_group_out_radii
    radii = am.leave_group_out_radii
    with pytest.raises(ValueError, match="12 labels for 10 stored rows"):
        radii(ok, g12, 1)
    with pytest.raises(ValueError, match="integer labels"):
        radii(ok, g10.astype(np.float32), 1)
    with pytest.raises(ValueError, match="1-D"):
        radii(ok, g10.reshape(5, 2), 1)
    with pytest.raises(ValueError, match="keeps none"):
        radii(am.AudioMetricsData(False), g10, 1)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="nearest_k=%d" % bad):
            radii(ok, g10, bad)
    with pytest.raises(NotImplementedError, match="float64"):
        radii(f64, g12, 1)
    with pytest.raises(ValueError, match="leaves 2 outside it, fewer than nearest_k=3"):
        radii(ok, np.array([0] * 8 + [1, 2]), 3)
    with pytest.raises(ValueError, match="fewer than nearest_k=1"):
        radii(ok, torch.zeros(10, dtype=torch.int16), 1)               # one song: nobody has a neighbour
    # prdc_leave_group_out
    prdc = am.prdc_leave_group_out
    with pytest.raises(ValueError, match="labels of both sets"):
        prdc(other, ok, 1, None, g10)
    with pytest.raises(ValueError, match="labels of both sets"):
        prdc(other, ok, 1, g12, None)
    with pytest.raises(ValueError, match="10 labels for 12 stored rows"):
        prdc(other, ok, 1, g10, g10)
    with pytest.raises(ValueError, match="12 labels for 10 stored rows"):
        prdc(other, ok, 1, g12, g12)
    with pytest.raises(ValueError, match="integer labels"):
        prdc(other, ok, 1, g12.astype(np.float64), g10)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="nearest_k=%d" % bad):
            prdc(other, ok, bad, g12, g10)
    with pytest.raises(NotImplementedError, match="float64"):
        prdc(f64, ok, 1, g12, g10)
    with pytest.raises(NotImplementedError, match="float64"):
        prdc(ok, f64, 1, g10, g12)
    with pytest.raises(ValueError, match="feature widths"):
        prdc(host_set(am, torch.zeros((12, 12))), ok, 1, g12, g10)
    with pytest.raises(ValueError, match="its reference set holds 9 of its 12 rows and leaves 3 outside it, fewer than nearest_k=4"):
        prdc(other, ok, 4, np.array([0] * 9 + [1, 2, 3]), g10)
    with pytest.raises(ValueError, match="its candidate set .* fewer than nearest_k=4"):
        prdc(other, ok, 4, g12, np.array([5] * 7 + [1, 2, 3]))
    with pytest.raises(ValueError, match="ref_radii must be a float32 tensor"):
        prdc(other, ok, 1, g12, g10, ref_radii=torch.zeros(10))
    with pytest.raises(ValueError, match="cand_radii must be a float32 tensor"):
        prdc(other, ok, 1, g12, g10, cand_radii=np.zeros(10, dtype=np.float32))
    # sample_fidelity / sample_fidelity_per_group
    with pytest.raises(ValueError, match="groups without manifold_groups"):
        am.sample_fidelity(ok, other, nearest_k=1, groups=g10)
    with pytest.raises(ValueError, match="12 labels for 10 stored rows"):
        am.sample_fidelity(ok, other, nearest_k=1, groups=g12, manifold_groups=g12)
    with pytest.raises(ValueError, match="10 labels for 12 stored rows"):
        am.sample_fidelity(ok, other, nearest_k=1, manifold_groups=g10)
    with pytest.raises(ValueError, match="nearest_k=33"):
        am.sample_fidelity(ok, other, nearest_k=33, manifold_groups=g12)
    with pytest.raises(ValueError, match="its manifold set .* fewer than nearest_k=5"):
        am.sample_fidelity(ok, other, nearest_k=5, groups=g10, manifold_groups=np.array([0] * 8 + [1, 2, 3, 4]))
    with pytest.raises(ValueError, match="fewer than nearest_k=9"):
        am.sample_fidelity(ok, ok, nearest_k=9, groups=g10)               # samples is manifold: manifold_groups = groups
    with pytest.raises(NotImplementedError, match="float64"):
        am.sample_fidelity(ok, f64, nearest_k=1, groups=g10, manifold_groups=g12)
    with pytest.raises(ValueError, match="integer labels"):
        am.sample_fidelity_per_group(ok, other, g10, nearest_k=1, manifold_groups=g12.astype(np.float32))
    with pytest.raises(ValueError, match="10 labels for 12 stored rows"):
        am.sample_fidelity_per_group(ok, other, g10, nearest_k=1, manifold_groups=g10)
    # authenticity_score
    with pytest.raises(ValueError, match="groups without train_groups"):
        am.authenticity_score(ok, other, groups=g10)
    with pytest.raises(ValueError, match="10 labels for 12 stored rows"):
        am.authenticity_score(ok, other, train_groups=g10)
    with pytest.raises(ValueError, match="12 labels for 10 stored rows"):
        am.authenticity_score(ok, other, train_groups=g12, groups=g12)
    with pytest.raises(ValueError, match="its training set .* fewer than nearest_k=1"):
        am.authenticity_score(ok, other, train_groups=np.zeros(12, dtype=np.int64))
    with pytest.raises(NotImplementedError, match="float64"):
        am.authenticity_score(ok, f64, train_groups=g12)


def test_plain_paths_are_untouched(am, monkeypatch):
    """without the new keywords the calls that reach hip_ops are today's"""
    from audio_metrics_amd import hip_ops
    seen = []

    def fake_scores(x, y, r_y):
        seen.append(("sample_scores", x is y, r_y))
        n = x.shape[0]
        return (torch.zeros(n), torch.zeros(n, dtype=torch.int64), torch.zeros(n, dtype=torch.int32), torch.zeros(n),
                torch.zeros(n, dtype=torch.int64))

    def fake_search(x, y, k, self_offset=None, squared=False):
        seen.append(("knn_search", k, self_offset, squared))
        return torch.ones((x.shape[0], k)), torch.zeros((x.shape[0], k), dtype=torch.int64)
    monkeypatch.setattr(hip_ops, "sample_scores", fake_scores)
    monkeypatch.setattr(hip_ops, "knn_search", fake_search)
    for name in ("sample_scores_groups", "knn_search_groups"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    ok, other = host_set(am, torch.zeros((10, 8))), host_set(am, torch.zeros((12, 8)))
    marker = torch.full((12,), 0.5)
    other.radii["radii_5"] = marker
    other.radii["radii_1"] = marker
    am.sample_fidelity(ok, other)
    am.sample_fidelity_per_group(ok, other, np.arange(10) // 2)
    am.authenticity_score(ok, other)
    assert [s[0] for s in seen] == ["sample_scores", "sample_scores", "knn_search"]
    assert seen[0][2] is marker and seen[1][2] is marker and seen[2][1:] == (1, None, False)


# ---------------------------------------------------------------------------------------------------- names and the C entry
def test_header_exports_signature_table_and_package_agree(am, lib):
    with open(os.path.join(ROOT, "include", "audio_metrics_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in am._lib.SIGNATURES and hasattr(lib, name), name
    assert len(am._lib.SIGNATURES["am_sample_scores_groups_f32"][1]) == 18
    from audio_metrics_amd.metrics import prdc_groups
    assert am.prdc_leave_group_out is prdc_groups.prdc_leave_group_out
    assert am.leave_group_out_radii is prdc_groups.leave_group_out_radii
    assert callable(am.hip_ops.sample_scores_groups)
    assert list(inspect.signature(am.prdc_leave_group_out).parameters) == \
        ["reference", "candidate", "nearest_k", "ref_groups", "groups", "match_across_sets", "ref_radii", "cand_radii", "return_rows"]
    assert list(inspect.signature(am.leave_group_out_radii).parameters) == ["data", "groups", "nearest_k"]
    # new keywords at the end, defaults that keep today's path
    assert list(inspect.signature(am.sample_fidelity).parameters) == \
        ["samples", "manifold", "nearest_k", "groups", "manifold_groups", "match_across_sets"]
    assert list(inspect.signature(am.sample_fidelity_per_group).parameters) == \
        ["samples", "manifold", "groups", "nearest_k", "return_rows", "manifold_groups", "match_across_sets"]
    assert list(inspect.signature(am.authenticity_score).parameters) == ["gen", "train", "return_rows", "train_groups", "groups"]
    for f, names in ((am.sample_fidelity, ("groups", "manifold_groups")), (am.authenticity_score, ("train_groups", "groups"))):
        assert all(inspect.signature(f).parameters[n].default is None for n in names)
    assert "prdc_leave_group_out" not in am.AudioMetrics.__dict__


def test_entry_point_error_paths(lib):
    n, m, d = 1000, 3000, 64
    nb = lib.am_sample_scores_groups_workspace_bytes(n, m, d)

    def call(x=FAKE, n=n, ldx=d, gx=FAKE, y=FAKE, m=m, ldy=d, gy=FAKE, d=d, r=FAKE, o1=FAKE, o2=FAKE, o3=FAKE, o4=FAKE, o5=FAKE,
             ws=FAKE, nb=nb):
        return lib.am_sample_scores_groups_f32(x, n, ldx, gx, y, m, ldy, gy, d, r, o1, o2, o3, o4, o5, ws, nb, None)
    assert call(x=None) == BAD_ARG and call(y=None) == BAD_ARG
    assert call(gx=None) == BAD_ARG and "x_group is null" in lib.am_last_error().decode()
    assert call(gy=None) == BAD_ARG and "y_group is null" in lib.am_last_error().decode()
    assert call(r=None) == BAD_ARG and "r_y is null" in lib.am_last_error().decode()
    for out, name in (("o1", "out_realism"), ("o2", "out_realism_idx"), ("o3", "out_count"), ("o4", "out_rarity"), ("o5", "out_rarity_idx")):
        assert call(**{out: None}) == BAD_ARG and name + " is null" in lib.am_last_error().decode()
    assert call(n=0) == BAD_SHAPE and call(m=0) == BAD_SHAPE and call(d=0) == BAD_SHAPE
    assert call(ldx=d - 4) == BAD_ARG and call(ldy=d + 1) == BAD_ARG and call(x=ctypes.c_void_p(0x10004)) == BAD_ARG
    assert call(m=1 << 32) == BAD_SHAPE                                 # a column takes 32 bits of a key
    assert call(nb=nb - 1) == WORKSPACE and str(nb) in lib.am_last_error().decode()
    assert "am_sample_scores_groups_workspace_bytes" in lib.am_last_error().decode()
    assert call(ws=None) == WORKSPACE and call(nb=0) == WORKSPACE


def test_workspace_query(lib):
    for bad in ((0, 10, 8), (10, 0, 8), (10, 10, 0), (10, 1 << 32, 8)):
        assert lib.am_sample_scores_groups_workspace_bytes(*bad) == 0, bad
    for n, m, d in ((1000, 5000, 64), (130, 4000, 40), (3, 2, 8), (100000, 100000, 512)):
        nb = lib.am_sample_scores_groups_workspace_bytes(n, m, d)
        assert nb > 0 and nb == lib.am_sample_scores_workspace_bytes(n, m, d)      # the labels are the caller's: nothing more to hold


# ---------------------------------------------------------------------------------------------------- why: the demonstration
def windowed_prdc(seed, d, shared, k=5, songs_ref=40, songs_cand=48):
    """PRDC in its three forms on song_windows rows (16 windows per song, spread 0.3) drawn from ONE distribution, numpy
    float64 distances: different songs on the two sides, or (shared) the same 40 songs with other windows."""
    ref, g_ref = pr.song_windows(seed, songs_ref, d)
    if shared:
        centres = np.random.default_rng(seed).standard_normal((songs_ref, d))      # the centres song_windows(seed) drew first
        rng = np.random.default_rng(seed + 100)
        cand = (np.repeat(centres, 16, axis=0) + 0.3 * rng.standard_normal((songs_ref * 16, d))).astype(np.float32)
        g_cand = g_ref.copy()
    else:
        cand, g_cand = pr.song_windows(seed + 100, songs_cand, d)
        g_cand = g_cand + 1000
    rr, cc, cr = (pr.d2_f64(a, b).astype(np.float32) for a, b in ((ref, ref), (cand, cand), (cand, ref)))
    return (pr.prdc_plain(rr, cc, cr, k), pr.prdc_leave_group_out(rr, cc, cr, g_ref, g_cand, k, False),
            pr.prdc_leave_group_out(rr, cc, cr, g_ref, g_cand, k, True))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_plain_manifold_of_windowed_rows_is_song_sized_specks(seed):
    """The bounds are conditions of the input recipe with a wide margin around the measured values (README), not tolerances
    of any code under test."""
    plain, radii_only, matched = windowed_prdc(seed, 64, shared=False)
    print(seed, plain, radii_only)
    assert plain["precision"] < 0.05 and plain["recall"] < 0.05                  # one distribution, and PRDC says "disjoint"
    assert radii_only["precision"] > 0.5 and radii_only["recall"] > 0.5
    assert matched == radii_only                                                # different songs: nothing to match
    plain, radii_only, matched = windowed_prdc(seed, 64, shared=True)
    print(seed, plain, radii_only, matched)
    assert radii_only["precision"] == 1.0 and radii_only["density"] > 3          # saturated: inside the siblings' wider balls
    assert matched["precision"] < 0.8
