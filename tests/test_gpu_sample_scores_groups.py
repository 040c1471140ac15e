"""Leave-group-out per-sample scores on the device (hip_ops.sample_scores_groups) and what stands on them
(leave_group_out_radii, prdc_leave_group_out, sample_fidelity / sample_fidelity_per_group / authenticity_score with labels).

  1  lattice rows with labels: all five outputs bit for bit against the numpy-f32 oracle (tests/prdc_groups_reference.py),
     through one and through more than one column chunk, exact ties included, contiguous rows and padded row views;
  2  equivalences with the plain kernel, bit for bit;  3  real-valued windowed rows at D = 512 against the plain kernel on
     column subsets, no tolerance;  4  independence of the stored order;  5  non-finite rows, special radii, determinism;
  6  the front ends against the oracle's floats.

The shapes are the smallest that cross the edges: 128 + 2 rows, 2 x 128 + 1 rows, a partial third column tile, D with and
without the inner-dimension tail, 4000 columns for the cross-chunk merge."""
import numpy as np
import pytest
import torch

import fidelity_reference as fr
import prdc_groups_reference as pr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ("realism", "realism_index", "ball_count", "rarity", "rarity_index")


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    audio_metrics_amd._lib.load()
    return audio_metrics_amd


@pytest.fixture(scope="module")
def ops(am):
    return am.hip_ops


@pytest.fixture(scope="module")
def lattice():
    """The oracle of every labelled lattice case, computed once and left unchanged."""
    return {c[:3]: pr.lattice_oracle(*c) for c in fr.LATTICE_CASES}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def labels(a):
    return dev(np.asarray(a, dtype=np.int32))


def as_bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32) if v.dtype == np.float32 else v


def host(out, n):
    assert [t.dtype for t in out] == [torch.float32, torch.int64, torch.int32, torch.float32, torch.int64]
    assert all(t.is_cuda and tuple(t.shape) == (n,) for t in out)
    return tuple(t.cpu().numpy() for t in out)


def scores(ops, x, y, r, gx, gy):
    return host(ops.sample_scores_groups(x, y, r, gx, gy), x.shape[0])


def plain(ops, x, y, r):
    return host(ops.sample_scores(x, y, r), x.shape[0])


def assert_same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        bad = np.flatnonzero(as_bits(g) != as_bits(w))
        assert bad.size == 0, (what, name, bad[:8], g[bad[:8]], w[bad[:8]])


def padded(a, extra, fill):
    """The same rows as a view of a wider buffer whose padding must never be read as data."""
    buf = torch.full((a.shape[0], a.shape[1] + extra), fill, dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = dev(a)
    view = buf[:, :a.shape[1]]
    assert view.stride(0) == a.shape[1] + extra
    return view


NOTHING = (0.0, -1, 0, 0.0, -1)


def assert_nothing(got, rows):
    for i in rows:
        assert tuple(g[i] for g in got) == NOTHING, (i, [g[i] for g in got])


# ---------------------------------------------------------------------------------------------------- 1. lattice, bit-exact
@pytest.mark.parametrize("n,m,d,k,duplicates", fr.LATTICE_CASES)
def test_lattice_rows_match_the_oracle_bit_for_bit(ops, lattice, n, m, d, k, duplicates):
    case = lattice[(n, m, d)]
    print(pr.check_lattice_is_not_degenerate(case))            # a kernel that ignores the labels cannot pass
    if m == 4000:
        assert ops.sample_scores_chunks(n, m, d) > 1            # the cross-chunk merge, ties across chunks
    x, y, r, gx, gy = dev(case["x"]), dev(case["y"]), dev(case["r"]), labels(case["gx"]), labels(case["gy"])
    assert_same(scores(ops, x, y, r, gx, gy), case["want"], (n, m, d))
    # the same radii without labels give the plain oracle: the difference asserted above is the labels' doing
    assert_same(plain(ops, x, y, r), case["plain"], (n, m, d, "plain"))


@pytest.mark.parametrize("n,m,d,k,duplicates", fr.LATTICE_CASES)
def test_padded_views_give_the_bits_of_contiguous_rows(ops, lattice, n, m, d, k, duplicates):
    case = lattice[(n, m, d)]
    got = scores(ops, padded(case["x"], 8, 1e30), padded(case["y"], 24, 1e30), dev(case["r"]), labels(case["gx"]), labels(case["gy"]))
    assert_same(got, case["want"], (n, m, d))


# ---------------------------------------------------------------------------------------------------- 2. equivalences
def test_equivalences_with_the_plain_kernel(ops, lattice):
    case = lattice[(130, 4000, 40)]
    n, m = 130, 4000
    x, y, r = dev(case["x"]), dev(case["y"]), dev(case["r"])
    # disjoint label values: nothing is skipped
    got = scores(ops, x, y, r, labels(np.arange(n) % 9), labels(100 + np.arange(m) % 11))
    assert_same(got, plain(ops, x, y, r), "disjoint")
    assert (got[2] > 0).any()
    # one label on everything: nobody has a reference row
    got = scores(ops, x, y, r, labels(np.full(n, -5)), labels(np.full(m, -5)))
    assert_nothing(got, range(n))
    # x is y, every row its own label: the row itself is skipped and nothing else
    case = lattice[(130, 300, 40)]
    y, m = case["y"], 300
    own = np.arange(m) * 7 - 1000
    d2 = fr.exact_d2(y, y)
    r = fr.radii_of_d2(d2, 5)
    yt = dev(y)
    got = scores(ops, yt, yt, dev(r), labels(own), labels(own))
    assert_same(got, pr.scores_groups_from_d2(d2, r, own, own), "x is y")
    assert np.isfinite(got[0]).all() and (got[1] != np.arange(m)).all()
    assert np.isposinf(plain(ops, yt, yt, dev(r))[0]).all()


# ---------------------------------------------------------------------------------------------------- 3. real-valued rows
def test_windowed_rows_at_512_columns_against_the_plain_kernel_on_column_subsets(ops):
    """The d2 of a pair does not depend on which other columns are present, so for the rows of label L the grouped count
    is the plain count over all of y minus the plain count over the columns of label L, and the grouped realism has the
    bits of the maximum of the plain realism over the other labels' column subsets.  No tolerance."""
    d, k = 512, 5
    y, gy = pr.song_windows(62, 63, d)
    y, gy = y[:1000], gy[:1000] % 5                               # 5 label values, each spread over many songs
    rng = np.random.default_rng(63)
    gx = np.repeat(np.arange(19), 16)[:300]
    centres = np.stack([y[np.arange(1000) // 16 == s].mean(axis=0) for s in range(19)])
    x = (centres[gx] + 0.3 * rng.standard_normal((300, d))).astype(np.float32)     # further windows of the first 19 songs
    gx = gx % 5
    xt, yt, gxt, gyt = dev(x), dev(y), labels(gx), labels(gy)
    r = ops.knn_search_groups(yt, yt, k, gyt, gyt)[0][:, k - 1].contiguous()
    assert torch.isfinite(r).all()
    got = scores(ops, xt, yt, r, gxt, gyt)
    whole = plain(ops, xt, yt, r)
    per_label = {}
    for lab in range(5):
        cols = np.flatnonzero(gy == lab)
        per_label[lab] = plain(ops, xt, dev(y[cols]), r[torch.as_tensor(cols, device=DEV)].contiguous())
    excluded = 0
    for lab in range(5):
        rows = np.flatnonzero(gx == lab)
        assert np.array_equal(got[2][rows], whole[2][rows] - per_label[lab][2][rows]), lab
        excluded += int(per_label[lab][2][rows].sum())
        others = np.stack([per_label[o][0][rows] for o in range(5) if o != lab])
        assert np.array_equal(as_bits(got[0][rows]), as_bits(others.max(axis=0))), lab
    assert excluded > 300 and 0 < (got[2] > 0).sum()              # the samples sit in their own songs' balls: plenty to exclude


# ---------------------------------------------------------------------------------------------------- 4. stored order
def test_stored_order_does_not_matter(ops):
    d, k = 64, 5
    y, gy = pr.song_windows(51, 20, d)
    x, gx = pr.song_windows(52, 12, d)
    x = (x + y[:len(x)]) * 0.5                                     # between its own song and a manifold song of the same label
    yt, gyt = dev(y), labels(gy)
    r = ops.knn_search_groups(yt, yt, k, gyt, gyt)[0][:, k - 1].contiguous()
    run = scores(ops, dev(x), yt, r, labels(gx), gyt)
    assert 0 < (run[2] > 0).sum() and (run[1] >= 0).all()
    px, py = np.random.default_rng(53).permutation(len(x)), np.random.default_rng(54).permutation(len(y))
    mix = scores(ops, dev(x[px]), dev(y[py]), r[torch.as_tensor(py, device=DEV)].contiguous(), labels(gx[px]), labels(gy[py]))
    for i in (0, 2, 3):
        assert np.array_equal(as_bits(mix[i]), as_bits(run[i][px])), NAMES[i]
    for i in (1, 4):
        assert np.array_equal(np.where(mix[i] >= 0, py[np.maximum(mix[i], 0)], -1), run[i][px]), NAMES[i]


# ---------------------------------------------------------------------------------------------------- 5. degenerate values
def test_non_finite_rows_special_radii_and_determinism(ops):
    n, m, d, k = 257, 300, 40, 5
    rng = np.random.default_rng(11)
    x, y = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((m, d)).astype(np.float32)
    x[:60] = y[:60] + 0.05 * rng.standard_normal((60, d)).astype(np.float32)
    gx, gy = rng.integers(0, 9, n), rng.integers(0, 9, m)
    gx[:60:2] = gy[:60:2]
    gxt, gyt, yt = labels(gx), labels(gy), dev(y)
    r = ops.knn_search_groups(yt, yt, k, gyt, gyt)[0][:, k - 1].contiguous()
    clean = scores(ops, dev(x), yt, r, gxt, gyt)
    assert (clean[2] > 0).sum() >= 30
    # a NaN / inf row of x scores nothing; the others are untouched
    xb = x.copy()
    xb[130, 3], xb[200, 0], xb[5, 39] = np.nan, np.inf, -np.inf
    got = scores(ops, dev(xb), yt, r, gxt, gyt)
    assert_nothing(got, (5, 130, 200))
    keep = np.setdiff1d(np.arange(n), (5, 130, 200))
    assert_same([g[keep] for g in got], [c[keep] for c in clean])
    # a NaN row of y and radii of 0, negative, NaN are nobody's ball: the set without those rows
    drop = np.array([1, 7, 129, 299])
    yb = y.copy()
    yb[1, 2] = np.nan
    r_cut = r.clone()
    r_cut[torch.as_tensor(drop[1:], device=DEV)] = torch.tensor([0.0, -1.0, float("nan")], device=DEV)
    got = scores(ops, dev(x), dev(yb), r_cut, gxt, gyt)
    cols = np.setdiff1d(np.arange(m), drop)
    sub = scores(ops, dev(x), dev(y[cols]), r[torch.as_tensor(cols, device=DEV)].contiguous(), gxt, labels(gy[cols]))
    for i in (0, 2, 3):
        assert np.array_equal(as_bits(got[i]), as_bits(sub[i])), NAMES[i]
    for i in (1, 4):
        assert np.array_equal(got[i], np.where(sub[i] >= 0, cols[np.maximum(sub[i], 0)], -1)), NAMES[i]
    # a radius of +inf holds every admissible finite row, and no other
    r_inf = torch.zeros(m, device=DEV)
    r_inf[17] = float("inf")
    got = scores(ops, dev(xb), yt, r_inf, gxt, gyt)
    admissible = (gx != gy[17]) & np.isfinite(xb).all(axis=1)
    assert np.array_equal(got[2], admissible.astype(np.int32)) and np.array_equal(got[4], np.where(admissible, 17, -1))
    assert np.isposinf(got[0][admissible]).all() and np.isposinf(got[3][admissible]).all() and (got[0][~admissible] == 0).all()
    # two calls give equal tensors
    a, b = ops.sample_scores_groups(dev(x), yt, r, gxt, gyt), ops.sample_scores_groups(dev(x), yt, r, gxt, gyt)
    assert all(torch.equal(s.view(torch.int32) if s.dtype == torch.float32 else s, t.view(torch.int32) if t.dtype == torch.float32 else t)
               for s, t in zip(a, b))


# ---------------------------------------------------------------------------------------------------- 6. front ends
def stored(am, rows):
    s = am.AudioMetricsData(True)
    for lo in range(0, len(rows), 32):                             # 32-row adds, like the embedding pipeline
        s.add(dev(rows[lo:lo + 32]))
    return s


@pytest.fixture(scope="module")
def songs():
    """The same 10 integer songs on both sides, other windows, and the oracle's PRDC in its three forms at k = 1 and 3."""
    ref, g = pr.integer_songs(90, 91)
    cand, _ = pr.integer_songs(90, 92)
    rr, cc, cr = fr.exact_d2(ref, ref), fr.exact_d2(cand, cand), fr.exact_d2(cand, ref)
    forms = {k: (pr.prdc_plain(rr, cc, cr, k), pr.prdc_leave_group_out(rr, cc, cr, g, g, k, False, rows=True),
                 pr.prdc_leave_group_out(rr, cc, cr, g, g, k, True, rows=True)) for k in (1, 3)}
    return {"ref": ref, "cand": cand, "g": g, "rr": rr, "cc": cc, "cr": cr, "forms": forms}


VALUES = ("precision", "recall", "density", "coverage")
# the oracle's values as the issue states them (density at k = 3, plain: 0.7792 rounded)
STATED = {1: ((0.6625, 0.575, 0.8125, 0.4125), (1.0, 1.0, 8.0625, 0.9875), (0.2625, 0.3, 0.6875, 0.3875)),
          3: ((0.975, 0.9125, 0.7792, 0.825), (1.0, 1.0, 3.525, 1.0), (0.65, 0.6, 0.95, 0.85))}


@pytest.mark.parametrize("k", [1, 3])
def test_prdc_leave_group_out_equals_the_oracle(am, songs, k):
    ref, cand, g = stored(am, songs["ref"]), stored(am, songs["cand"]), songs["g"]
    plain_form, radii_only, matched = songs["forms"][k]
    for form, stated in zip((plain_form, radii_only, matched), STATED[k]):
        assert all(abs(form[v] - s) < 5e-5 for v, s in zip(VALUES, stated)), (form, stated)
    for v in VALUES:                                               # all three forms are pairwise different in every value
        assert len({plain_form[v], radii_only[v], matched[v]}) == 3, v
    assert am.prdc(ref, cand, k) == plain_form
    for match, want in ((True, matched), (False, radii_only)):
        got = am.prdc_leave_group_out(ref, cand, k, g, g, match_across_sets=match, return_rows=True)
        assert sorted(got) == sorted([*VALUES, "nearest_k", "shared_labels", "candidate_ball_count", "reference_recalled",
                                      "reference_covered"])
        assert all(type(got[v]) is float and got[v] == want[v] for v in VALUES), (match, got, want)
        assert got["nearest_k"] == k and got["shared_labels"] == 10
        assert got["candidate_ball_count"].dtype == np.int32 and got["candidate_ball_count"].shape == (80,)
        assert got["reference_recalled"].dtype == bool and got["reference_covered"].dtype == bool
        assert got["reference_recalled"].shape == got["reference_covered"].shape == (80,)
        for name in ("candidate_ball_count", "reference_recalled", "reference_covered"):
            assert np.array_equal(got[name], want[name]), (match, name)
        short = am.prdc_leave_group_out(ref, cand, k, g, g, match_across_sets=match)
        assert sorted(short) == sorted([*VALUES, "nearest_k", "shared_labels"]) and all(short[v] == want[v] for v in VALUES)
    # disjoint label values: the two settings agree, and it is the radii-only form
    far = g + 10000
    a = am.prdc_leave_group_out(ref, cand, k, g, far, match_across_sets=True, return_rows=True)
    b = am.prdc_leave_group_out(ref, cand, k, g, far, match_across_sets=False, return_rows=True)
    assert a["shared_labels"] == b["shared_labels"] == 0
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    assert all(a[v] == radii_only[v] for v in VALUES)
    # host and device labels, any integer dtype; radii handed in
    r_ref, r_cand = am.leave_group_out_radii(ref, g, k), am.leave_group_out_radii(cand, dev(g.astype(np.int16)), k)
    assert r_ref.is_cuda and r_ref.dtype == torch.float32 and tuple(r_ref.shape) == (80,)
    assert np.array_equal(as_bits(r_ref.cpu().numpy()), as_bits(pr.lso_radii(songs["rr"], g, k)))
    again = am.prdc_leave_group_out(ref, cand, k, dev(g), dev(g.astype(np.int32)), ref_radii=r_ref, cand_radii=r_cand)
    assert all(again[v] == matched[v] for v in VALUES) and again["shared_labels"] == 10


@pytest.mark.parametrize("k", [1, 3])
def test_sample_fidelity_with_labels_equals_the_oracle(am, songs, k):
    ref, cand, g = stored(am, songs["ref"]), stored(am, songs["cand"]), songs["g"]
    r = pr.lso_radii(songs["rr"], g, k)
    want = pr.scores_groups_from_d2(songs["cr"], r, g, g)
    prdc = am.prdc_leave_group_out(ref, cand, k, g, g)
    for labels_of in (lambda a: a, dev):                           # host and device labels give the same result
        res = am.sample_fidelity(cand, ref, nearest_k=k, groups=labels_of(g), manifold_groups=labels_of(g))
        assert sorted(res) == sorted([*NAMES, "in_manifold", "nearest_k", "precision", "density"])
        assert_same([res[name] for name in NAMES], want, k)
        assert res["precision"] == prdc["precision"] and res["density"] == prdc["density"]        # no tolerance
        per = am.sample_fidelity_per_group(cand, ref, labels_of(g), nearest_k=k, return_rows=True, manifold_groups=labels_of(g))
        assert_same([per[name] for name in NAMES], want, k)
        by_group = am.fidelity_by_group(g, want[0], want[2], want[3], k)
        for name, v in by_group.items():
            assert np.array_equal(per[name], v, equal_nan=True), name
    # radii only: the manifold's labels alone, or matching switched off
    radii_only = fr.scores_from_d2(songs["cr"], r)
    assert_same([am.sample_fidelity(cand, ref, nearest_k=k, manifold_groups=g)[name] for name in NAMES], radii_only, "radii only")
    res = am.sample_fidelity(cand, ref, nearest_k=k, groups=g, manifold_groups=g, match_across_sets=False)
    assert_same([res[name] for name in NAMES], radii_only, "unmatched")
    unmatched = am.prdc_leave_group_out(ref, cand, k, g, g, match_across_sets=False)
    assert res["precision"] == unmatched["precision"] and res["density"] == unmatched["density"]
    # a set against itself: every row against the OTHER songs, no +inf realism
    own = am.sample_fidelity(ref, ref, nearest_k=k, groups=g)
    assert_same([own[name] for name in NAMES], pr.scores_groups_from_d2(songs["rr"], r, g, g), "own")
    assert np.isfinite(own["realism"]).all() and (g[own["realism_index"]] != g).all()
    assert np.isposinf(am.sample_fidelity(ref, ref, nearest_k=k)["realism"]).all()               # the plain path is untouched


def test_radii_with_one_label_per_row_are_get_radii(am, songs):
    ref = stored(am, songs["ref"])
    for k in (1, 3, 5):
        got = am.leave_group_out_radii(ref, np.arange(80) * 5 - 7, k)
        assert torch.equal(got.view(torch.int32), ref.get_radii(k).view(torch.int32)), k
    x, _ = pr.song_windows(71, 20, 40)
    s = stored(am, x[:257])
    assert torch.equal(am.leave_group_out_radii(s, np.arange(257), 5).view(torch.int32), s.get_radii(5).view(torch.int32))


def test_authenticity_with_labels_equals_the_oracle(am, songs):
    train, gen, g = stored(am, songs["ref"]), stored(am, songs["cand"]), songs["g"]
    want = {"plain": pr.authenticity(songs["cr"], songs["rr"]), "train": pr.authenticity(songs["cr"], songs["rr"], g),
            "both": pr.authenticity(songs["cr"], songs["rr"], g, g)}
    assert len({w[0] for w in want.values()}) == 3                 # the three forms differ on this recipe
    for key, kw in (("plain", {}), ("train", dict(train_groups=g)), ("both", dict(train_groups=dev(g), groups=g))):
        got = am.authenticity_score(gen, train, return_rows=True, **kw)
        frac, authentic, nearest = want[key]
        assert got["authenticity"] == frac and np.array_equal(got["authentic"], authentic), key
        assert np.array_equal(got["authenticity_nearest_train"], nearest), key
        # without rows the fraction is the device's f64 mean of the same 0 / 1 flags, as on the plain path: one rounding of
        # its own (the sum times a rounded 1 / M, against the host's sum / M), each below 2^-52 relative
        short = am.authenticity_score(gen, train, **kw)
        assert list(short) == ["authenticity"] and abs(short["authenticity"] - frac) <= 4 * 2.0 ** -52 * frac, key
    assert (g[want["both"][2]] != g).all()
