"""Retrieval ranks on the device (hip_ops.retrieval_ranks, retrieval_scores).

  1  lattice rows: better, tied, positive, n_pos and the bits of the score against the numpy-f32 oracle
     (tests/retrieval_reference.py), both similarities, both policies, paired and labelled positives, tie-heavy;
  2  random rows: the f64 sandwich lo <= better <= better + tied <= hi, and better == lo wherever lo == hi;
  3  groups: the counts of the no-group call on the gallery without the row's own-group columns;
  4  padded views and degenerate values;  5  determinism;  6  the front end.

The shapes are the smallest that cross the edges: 128 + 2 rows, a partial third column tile, one column, D with and
without the inner-dimension tail, 4000 columns for the cross-chunk merge."""
import warnings

import numpy as np
import pytest
import torch

import retrieval_reference as rr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ("better", "tied", "score", "positive", "n_pos", "n_pos_own_group")
DTYPES = [torch.int32, torch.int32, torch.float32, torch.int64, torch.int32, torch.int32]


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    audio_metrics_amd._lib.load()
    return audio_metrics_amd


@pytest.fixture(scope="module")
def ops(am):
    return am.hip_ops


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def as_bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32) if v.dtype == np.float32 else v


def ranks(ops, q, g, positives, cosine, groups=None, segs=None):
    """One call from host arrays (or device views) -> the six outputs as numpy arrays."""
    start, count, cols = segs if segs is not None else rr.segments(positives)
    q = q if torch.is_tensor(q) else dev(q)
    g = g if torch.is_tensor(g) else dev(g)
    out = ops.retrieval_ranks(q, g, dev(start), dev(count), dev(cols), cosine=cosine,
                              groups=None if groups is None else tuple(dev(v) for v in groups))
    assert [t.dtype for t in out] == DTYPES
    assert all(t.is_cuda and tuple(t.shape) == (q.shape[0],) for t in out)
    return tuple(t.cpu().numpy() for t in out)


def assert_oracle(got, want, what=""):
    """Bit for bit; the score of an unranked row is NaN on both sides (any payload)."""
    for name, g in zip(NAMES, got):
        w = want[name]
        if name == "score":
            assert np.array_equal(np.isnan(g), np.isnan(w)), (what, name)
            g, w = np.where(np.isnan(g), np.float32(0), g), np.where(np.isnan(w), np.float32(0), w)
        bad = np.flatnonzero(as_bits(g) != as_bits(w.astype(g.dtype)))
        assert bad.size == 0, (what, name, bad[:8], g[bad[:8]], w[bad[:8]])


def assert_same(a, b, what=""):
    for name, x, y in zip(NAMES, a, b):
        if name == "score":
            assert np.array_equal(np.isnan(x), np.isnan(y)), (what, name)
            x, y = np.where(np.isnan(x), np.float32(0), x), np.where(np.isnan(y), np.float32(0), y)
        bad = np.flatnonzero(as_bits(x) != as_bits(y))
        assert bad.size == 0, (what, name, bad[:8], x[bad[:8]], y[bad[:8]])


def lattice_case(n, m, d, labelled):
    """Lattice rows with structure: a third of the paired columns equal their query (rank 1 unless a longer duplicate
    direction wins under dot), a few are the NEGATED query (a negative threshold: every real column beats it, a padded one
    must not), the rest are unrelated.  Labelled: several positives per row, duplicated gallery rows under one label (tied
    positives: the smallest column is reported), query labels that no gallery row carries."""
    q, g = rr.lattice_rows(n + m + d, n, d), rr.lattice_rows(n + m + d + 1, m, d)
    p = min(n, m)
    idx = np.arange(p)
    g[idx[idx % 3 == 0]] = q[idx[idx % 3 == 0]]
    g[idx[idx % 7 == 1]] = -q[idx[idx % 7 == 1]]
    song_q, song_g = (np.arange(n) // 5).astype(np.int32), (np.arange(m) // 5).astype(np.int32)      # five windows per song, paired
    if not labelled:
        return q, g, rr.paired_positives(n) if n == m else None, (song_q, song_g)
    n_labels = max(2, min(n, m) // 2)
    q_labels = np.arange(n) % (n_labels + 3)                                 # the last three labels: no gallery row
    g_labels = (np.arange(m) * 7) % n_labels
    if m >= 2 * n_labels:
        g[n_labels:2 * n_labels] = g[:n_labels]                             # columns j and j + n_labels: one label, equal rows
    for i in range(0, min(n, n_labels), 3):                                 # every third label: its first column is the query itself
        g[np.flatnonzero(g_labels == q_labels[i])[0]] = q[i]
    return q, g, rr.label_positives(q_labels, g_labels), (song_q, song_g)


# ---------------------------------------------------------------------------------------------------- 1. lattice, bit-exact
@pytest.mark.parametrize("n,m,d", rr.SHAPES)
def test_lattice_rows_match_the_oracle_bit_for_bit(ops, n, m, d):
    if m == 4000:
        assert ops.retrieval_chunks(n, m, d) > 1                            # the cross-chunk merge is on the path
    q, g, positives, groups = lattice_case(n, m, d, labelled=True)
    seen_tied = seen_better = seen_first = seen_neg_thr = False
    for cosine in (False, True):
        for grp in (None, groups):
            want = rr.lattice_oracle(q, g, positives, cosine, *(grp or ()))
            got = ranks(ops, q, g, positives, cosine, grp)
            assert_oracle(got, want, (cosine, grp is not None))
            ranked = want["positive"] >= 0
            if m > 1:
                assert ranked.any() and (~ranked).any()                     # rows with positives and rows with none
                assert (want["n_pos"] > 1).any()
            if not cosine:
                seen_tied |= bool(want["tied"][ranked].sum() > 0)
                seen_better |= bool((want["better"][ranked] > 0).any())
                seen_first |= bool((want["better"][ranked] == 0).any())
                seen_neg_thr |= bool((want["t"][ranked] < 0).any())
    if m > 1:
        assert seen_tied and seen_better and seen_first                     # tie-heavy under dot, ranks neither all first nor all late
        if m == 300:
            assert seen_neg_thr


@pytest.mark.parametrize("n,m,d", [(130, 130, 40), (257, 257, 64)])
def test_paired_lattice_rows_with_negative_thresholds_and_a_partial_last_tile(ops, n, m, d):
    """Paired positives; every seventh column is the negated query, so t_i = -|q_i|^2 < 0 and nearly every real column beats
    it: a padded column of the partial last tile (u = 0 > t_i if it counted) would show as better > negatives."""
    q, g, positives, groups = lattice_case(n, m, d, labelled=False)
    for cosine in (False, True):
        for grp in (None, groups):
            want = rr.lattice_oracle(q, g, positives, cosine, *(grp or ()))
            got = ranks(ops, q, g, positives, cosine, grp)
            assert_oracle(got, want, (cosine, grp is not None))
            neg_thr = np.flatnonzero(want["t"] < 0)
            assert neg_thr.size >= n // 8
            assert (want["better"][neg_thr] + want["tied"][neg_thr] <= want["negatives"][neg_thr]).all()
            assert (got[0][neg_thr] >= want["negatives"][neg_thr] - 8).any()  # rows that (nearly) every real negative beats
            if grp is not None:
                assert (want["n_pos_own_group"] == 1).all()                 # the positive sits in the row's own song and stays the positive
    want = rr.lattice_oracle(q, g, positives, False)
    assert want["tied"].sum() > 0 and (want["better"] > 0).any() and (want["better"] == 0).any()


# ---------------------------------------------------------------------------------------------------- 2. random rows, f64 sandwich
@pytest.mark.parametrize("cosine", [True, False])
@pytest.mark.parametrize("n,m,d", rr.SHAPES)
def test_random_rows_lie_inside_the_f64_sandwich(ops, n, m, d, cosine):
    q, g, q_labels, g_labels = rr.sandwich_rows(n, m, d)
    positives = rr.label_positives(q_labels, g_labels)
    lo, hi, ranked = rr.sandwich(q, g, positives, cosine)
    better, tied, score, positive, n_pos, _ = ranks(ops, q, g, positives, cosine)
    p = min(n, m)
    assert ranked.sum() == p and np.array_equal(positive >= 0, ranked) and np.array_equal(n_pos, ranked.astype(np.int32))
    assert np.array_equal(positive[ranked], np.arange(p))
    assert (better[~ranked] == -1).all() and (tied[~ranked] == -1).all() and np.isnan(score[~ranked]).all()
    b, t = better[ranked].astype(np.int64), tied[ranked].astype(np.int64)
    print(f"{n}x{m}x{d} cosine={cosine}: decided {np.mean(lo[ranked] == hi[ranked]):.3f}, better quartiles "
          f"{np.percentile(b, [25, 50, 75, 100])}, ties {t.sum()}")
    assert (lo[ranked] <= b).all() and (t >= 0).all() and (b + t <= hi[ranked]).all()
    decided = lo[ranked] == hi[ranked]
    assert np.array_equal(b[decided], lo[ranked][decided])
    assert decided.mean() >= 0.85                                           # the sandwich is not vacuous
    # the score itself: the cosine (or the dot product) of the pair, inside the same bound
    s, eps = rr.scores_f64(q, g, cosine)
    i = np.flatnonzero(ranked)
    want = s[i, i] / (np.linalg.norm(q[i].astype(np.float64), axis=1) if cosine else 1.0)
    assert np.all(np.abs(score[ranked] - want) <= 2.0 * eps[i, i] / (np.linalg.norm(q[i].astype(np.float64), axis=1) if cosine else 1.0) + 1e-7)


# ---------------------------------------------------------------------------------------------------- 3. groups
def test_groups_equal_the_plain_call_without_the_rows_own_group(ops):
    """Queries: label = song (the windows of a song share their positives).  Gallery: a song and a label per row, so that a
    query's positives lie inside AND outside its own song.  For every song c the grouped counts of its rows equal the
    plain call on the gallery that keeps the columns of the other songs and the positives of c."""
    n, m, d, songs = 40, 300, 40, 6
    rng = np.random.default_rng(11)
    q, g = rr.lattice_rows(21, n, d), rr.lattice_rows(22, m, d)
    q_song = (np.arange(n) % songs).astype(np.int32)
    g_song = rng.integers(0, songs, m).astype(np.int32)
    g_label = rng.integers(0, songs + 2, m)
    g[:songs] = q[:songs]                                                   # some positives that win
    g_label[:songs], g_song[:songs] = np.arange(songs), np.arange(songs)
    positives = rr.label_positives(q_song, g_label)
    for cosine in (True, False):
        want = rr.lattice_oracle(q, g, positives, cosine, q_song, g_song)
        full = ranks(ops, q, g, positives, cosine, (q_song, g_song))
        assert_oracle(full, want, cosine)
        assert (want["n_pos_own_group"] > 0).all() and (want["n_pos_own_group"] < want["n_pos"]).all()
        plain = ranks(ops, q, g, positives, cosine)
        assert (plain[0] >= full[0]).all() and (plain[0] > full[0]).any()   # the own song held better-scoring columns
        for c in range(songs):
            rows = np.flatnonzero(q_song == c)
            keep = np.flatnonzero((g_song != c) | (g_label == c))           # ascending: the tie order of the columns is kept
            sub_pos = [np.flatnonzero(g_label[keep] == c) for _ in rows]
            sub = ranks(ops, q[rows], g[keep], sub_pos, cosine)
            assert np.array_equal(sub[0], full[0][rows]) and np.array_equal(sub[1], full[1][rows]), (cosine, c)
            assert np.array_equal(as_bits(sub[2]), as_bits(full[2][rows])) and np.array_equal(keep[sub[3]], full[3][rows])
            assert np.array_equal(sub[4], full[4][rows])
            assert np.array_equal(want["negatives"][rows], len(keep) - sub[4])


def test_front_end_counts_the_negatives_of_grouped_rows_directly(am):
    n, m, d = 130, 300, 40
    q, g = rr.lattice_rows(31, n, d), rr.lattice_rows(32, m, d)
    q_labels, g_labels = np.arange(n) % 50, np.arange(m) % 60
    q_song, g_song = np.arange(n) // 4 + 100, np.arange(m) // 6 + 100         # any integer values, joint across the sets
    positives = rr.label_positives(q_labels, g_labels)
    want = rr.lattice_oracle(q, g, positives, True, q_song, g_song)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = am.retrieval_scores(dev(q), dev(g), query_labels=q_labels, gallery_labels=dev(g_labels), groups=dev(q_song),
                                  gallery_groups=g_song, return_rows=True)
    direct = np.array([np.count_nonzero((g_labels != q_labels[i]) & (g_song != q_song[i])) for i in range(n)])
    assert np.array_equal(got["negatives"], direct) and np.array_equal(got["negatives"], want["negatives"])
    assert np.array_equal(got["ranks"], np.where(want["better"] >= 0, want["better"] + 1, -1))
    assert np.array_equal(got["tied"], want["tied"]) and np.array_equal(got["positive_index"], want["positive"])
    ref = rr.summary(got["ranks"], got["tied"], negatives=direct, units=q_song)
    for k, w in ref.items():
        assert got[k] == pytest.approx(w, rel=1e-12), k


# ---------------------------------------------------------------------------------------------------- 4. views, degenerate values
@pytest.mark.parametrize("cosine", [True, False])
def test_padded_views_give_the_bits_of_the_contiguous_call(ops, cosine):
    n, m, d = 130, 300, 40
    q, g, positives, groups = lattice_case(n, m, d, labelled=True)

    def padded(a, extra):
        buf = torch.full((a.shape[0], a.shape[1] + extra), float("nan"), dtype=torch.float32, device=DEV)
        buf[:, :a.shape[1]] = dev(a)
        view = buf[:, :a.shape[1]]
        assert view.stride(0) == a.shape[1] + extra
        return view
    base = ranks(ops, q, g, positives, cosine, groups)
    assert_same(ranks(ops, padded(q, 4), padded(g, 12), positives, cosine, groups), base)
    rq, rg, lq, lg = rr.sandwich_rows(n, m, d)
    pos = rr.label_positives(lq, lg)
    assert_same(ranks(ops, padded(rq, 8), padded(rg, 4), pos, cosine), ranks(ops, rq, rg, pos, cosine))


def test_degenerate_values_give_the_documented_outputs(ops):
    n, m, d = 130, 300, 40
    q, g = rr.lattice_rows(41, n, d), rr.lattice_rows(42, m, d)
    g[7] = 0.0                          # a zero-norm gallery row: no score under cosine (0 * inf), the score 0 under dot
    g[9, 3] = np.nan                    # a non-finite gallery row: no score
    q[5, 0] = np.nan                    # a NaN query row: nothing in its row has a score
    positives = rr.paired_positives(n)
    positives[20] = np.array([7, 9])    # its only positives are unscored under cosine
    positives[21] = np.array([7, 21])
    positives[22] = np.array([], np.int64)
    for cosine in (True, False):
        want = rr.lattice_oracle(q, g, positives, cosine)
        got = ranks(ops, q, g, positives, cosine)
        assert_oracle(got, want, cosine)
        better, tied, score, positive, n_pos, n_own = got
        for i in (5, 9, 22) + ((7, 20) if cosine else ()):
            assert (better[i], tied[i], positive[i]) == (-1, -1, -1) and np.isnan(score[i]), (cosine, i)
        assert n_pos[20] == 2 and n_pos[22] == 0 and n_pos[5] == 1 and (n_own == 0).all()
        if not cosine:
            assert positive[20] == 7 and score[20] == 0.0 and positive[7] == 7 and score[7] == 0.0
        if cosine:
            assert positive[21] == 21
        ok = np.setdiff1d(np.arange(n), [5, 7, 9, 20, 21, 22])
        assert (positive[ok] == ok).all()
    # one column
    q1, g1 = rr.lattice_rows(43, n, d), rr.lattice_rows(44, 1, d)
    pos1 = [np.array([0]) if i % 2 else np.array([], np.int64) for i in range(n)]
    for cosine in (True, False):
        got = ranks(ops, q1, g1, pos1, cosine)
        assert_oracle(got, rr.lattice_oracle(q1, g1, pos1, cosine), cosine)
        assert (got[0][1::2] == 0).all() and (got[1][1::2] == 0).all() and (got[0][0::2] == -1).all()


def test_a_positive_column_out_of_range_is_never_read_and_leaves_the_row_unranked(ops):
    n, m, d = 130, 300, 40
    q, g = rr.lattice_rows(51, n, d), rr.lattice_rows(52, m, d)
    positives = rr.paired_positives(n)
    want = rr.lattice_oracle(q, g, positives, True)
    start, count, cols = rr.segments(positives)
    cols = cols.copy()
    cols[3], cols[4] = m, -1                              # one past the end, and negative
    cols = np.concatenate([cols, [17, 1 << 40]])          # row 6: two entries, one far outside
    start, count = start.copy(), count.copy()
    start[6], count[6] = n, 2
    start[8], count[8] = n + 1, 5                         # a segment that leaves pos_columns
    start[10], count[10] = -3, 1
    got = ranks(ops, q, g, None, True, segs=(start, count, cols))
    bad = [3, 4, 6, 8, 10]
    for i in bad:
        assert (got[0][i], got[1][i], got[3][i]) == (-1, -1, -1) and np.isnan(got[2][i]), i
    assert got[4][3] == 0 and got[4][4] == 0 and got[4][6] == 1 and got[4][8] == 0 and got[4][10] == 0
    ok = np.setdiff1d(np.arange(n), bad)
    for k, name in enumerate(NAMES):
        w = want[name][ok]
        assert np.array_equal(as_bits(got[k][ok]), as_bits(w.astype(got[k].dtype))), name


# ---------------------------------------------------------------------------------------------------- 5. determinism
def test_two_calls_give_the_same_bits_and_the_order_inside_a_segment_does_not_matter(ops):
    n, m, d = 130, 4000, 40
    q, g, positives, groups = lattice_case(n, m, d, labelled=True)
    rq, rg, lq, lg = rr.sandwich_rows(n, m, d)
    rng = np.random.default_rng(9)
    for cosine in (True, False):
        a = ranks(ops, q, g, positives, cosine, groups)
        assert_same(ranks(ops, q, g, positives, cosine, groups), a)
        shuffled = [rng.permutation(p) for p in positives]
        assert any(len(p) > 1 and not np.array_equal(p, s) for p, s in zip(positives, shuffled))
        assert_same(ranks(ops, q, g, shuffled, cosine, groups), a)
        pos = rr.label_positives(lq, lg)
        assert_same(ranks(ops, rq, rg, pos, cosine), ranks(ops, rq, rg, pos, cosine))


# ---------------------------------------------------------------------------------------------------- 6. front end
def test_front_end_on_paired_unit_norm_rows_agrees_with_the_summary_of_the_oracles_ranks(am):
    n, d = 257, 40
    q, g = rr.unit_lattice_rows(61, n, d), rr.unit_lattice_rows(62, n, d)
    g[::2] = q[::2]
    want = rr.lattice_oracle(q, g, rr.paired_positives(n), True)
    assert want["tied"].sum() > 0 and (want["better"] > 0).any()
    oracle_ranks = want["better"].astype(np.int64) + 1
    for ties in ("optimistic", "pessimistic", "mean"):
        got = am.retrieval_scores(dev(q), dev(g), ties=ties, ks=(1, 5, 10, 50), return_rows=True)
        assert np.array_equal(got["ranks"], oracle_ranks) and np.array_equal(got["tied"], want["tied"])
        assert np.array_equal(as_bits(got["positive_score"]), as_bits(want["score"]))
        assert np.array_equal(got["positive_index"], np.arange(n)) and (got["negatives"] == n - 1).all()
        ref = am.retrieval_summary(oracle_ranks, want["tied"], ks=(1, 5, 10, 50), ties=ties, negatives=np.full(n, n - 1))
        direct = rr.summary(oracle_ranks, want["tied"], ks=(1, 5, 10, 50), ties=ties, negatives=np.full(n, n - 1))
        for k, w in ref.items():
            assert got[k] == w, (ties, k)
            assert w == pytest.approx(direct[k], rel=1e-12), (ties, k)
        assert got["retrieval_similarity"] == "cosine" and isinstance(got["recall_at_1"], float)
    data_q, data_g = am.AudioMetricsData(True), am.AudioMetricsData(True)
    data_q.add(dev(q))
    data_g.add(dev(g))
    stored = am.retrieval_scores(data_q, data_g, similarity="dot", return_rows=True)
    assert stored["retrieval_similarity"] == "dot" and np.array_equal(stored["ranks"], oracle_ranks)     # unit norms: one order


def test_front_end_identical_rows_unranked_rows_and_a_shuffled_gallery(am):
    rng = np.random.default_rng(71)
    n, d = 300, 64
    x = rng.standard_normal((n, d)).astype(np.float32)
    same = am.retrieval_scores(dev(x), dev(x))
    assert same["recall_at_1"] == 1.0 and same["median_rank"] == 1.0 and same["mrr"] == 1.0 and same["retrieval_rows_unranked"] == 0.0
    # five captions per clip, shuffled: the ranks of the unshuffled call, the positive's index mapped
    clips = 60
    audio = rng.standard_normal((clips, d)).astype(np.float32)
    text = (np.repeat(audio, 5, axis=0) + 4.0 * rng.standard_normal((5 * clips, d))).astype(np.float32)
    text_labels, audio_labels = np.repeat(np.arange(clips), 5), np.arange(clips)
    a2t = am.retrieval_scores(dev(audio), dev(text), query_labels=audio_labels, gallery_labels=text_labels, return_rows=True)
    perm = rng.permutation(5 * clips)
    shuffled = am.retrieval_scores(dev(audio), dev(text[perm]), query_labels=audio_labels, gallery_labels=text_labels[perm],
                                   return_rows=True)
    assert np.array_equal(shuffled["ranks"], a2t["ranks"]) and np.array_equal(shuffled["tied"], a2t["tied"])
    assert np.array_equal(perm[shuffled["positive_index"]], a2t["positive_index"])
    assert np.array_equal(as_bits(shuffled["positive_score"]), as_bits(a2t["positive_score"]))
    assert (a2t["negatives"] == 5 * clips - 5).all() and 0.0 < a2t["recall_at_1"] < 1.0 and a2t["recall_at_10"] > a2t["chance_recall_at_10"]
    t2a = am.retrieval_scores(dev(text), dev(audio), query_labels=text_labels, gallery_labels=audio_labels)
    assert t2a["retrieval_rows_ranked"] == 5.0 * clips and 0.0 < t2a["recall_at_1"] < 1.0
    # a zero row has no cosine: unranked, one warning, left out of the means
    y = x.copy()
    y[4] = 0.0
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = am.retrieval_scores(dev(x), dev(y), return_rows=True)
    assert len(caught) == 1 and caught[0].category is RuntimeWarning and "retrieval_scores: 1 of 300" in str(caught[0].message)
    assert got["ranks"][4] == -1 and got["retrieval_rows_unranked"] == 1.0 and got["recall_at_1"] == 1.0
    with pytest.raises(am._lib.HipLibraryError):
        am.retrieval_scores(torch.as_tensor(x), torch.as_tensor(x))           # host rows: no CPU fallback
