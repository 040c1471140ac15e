"""Retrieval ranks, the part that needs no GPU: retrieval_summary on hand-made ranks (the three tie rules, unranked rows,
the mAP@10 cut-off, chance recall, the cluster-robust error against a direct formula), the numpy reference the GPU tests
lean on (tests/retrieval_reference.py) against a direct loop, the argument errors of retrieval_scores that are raised before
any device call, and the host side of am_retrieval_ranks_f32 (workspace and chunk queries, error codes from a fake
pointer)."""
import ctypes
import math
import warnings

import numpy as np
import pytest
import torch

import retrieval_reference as rr

BAD_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -4
FAKE = ctypes.c_void_p(0x10000)                       # 16-byte aligned, never dereferenced: the calls stop at validation


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    return audio_metrics_amd


@pytest.fixture(scope="module")
def lib(am):
    return am._lib.load()


@pytest.fixture(autouse=True)
def feature_present(am):
    """The reference below is only worth its tests beside the feature it checks."""
    assert hasattr(am, "retrieval_scores") and hasattr(am.hip_ops, "retrieval_ranks") and "am_retrieval_ranks_f32" in am._lib.SIGNATURES


# ---------------------------------------------------------------------------------------------------- the summary
RANKS = np.array([1, 3, 1, 12, 6, 2, 10, 11, 1, 40])
TIED = np.array([0, 2, 1, 0, 0, 9, 1, 0, 0, 3])


def test_summary_with_the_three_tie_rules(am):
    opt = am.retrieval_summary(RANKS, TIED)
    assert opt["recall_at_1"] == 0.3 and opt["recall_at_5"] == 0.5 and opt["recall_at_10"] == 0.7
    assert opt["median_rank"] == 4.5 and opt["mean_rank"] == 8.7
    assert opt["mrr"] == pytest.approx(np.mean(1.0 / RANKS), rel=1e-15)
    assert opt["retrieval_ties"] == 16.0 and opt["retrieval_rows_ranked"] == 10.0 and opt["retrieval_rows_unranked"] == 0.0
    pes = am.retrieval_summary(RANKS, TIED, ties="pessimistic")
    assert pes["recall_at_1"] == 0.2 and pes["recall_at_5"] == 0.4 and pes["recall_at_10"] == 0.5      # 1, 5, 2, 12, 6, 11, 11, 11, 1, 43
    assert pes["mean_rank"] == pytest.approx(10.3)
    mean = am.retrieval_summary(RANKS, TIED, ties="mean")
    assert mean["recall_at_1"] == 0.2 and mean["recall_at_5"] == 0.4 and mean["recall_at_10"] == 0.6   # 1, 4, 1.5, 12, 6, 6.5, 10.5, 11, 1, 41.5
    assert mean["median_rank"] == 6.25
    assert am.retrieval_summary(RANKS)["recall_at_1"] == 0.3 and am.retrieval_summary(RANKS)["retrieval_ties"] == 0.0
    for ties in rr_ties():
        got = am.retrieval_summary(RANKS, TIED, ks=(1, 3, 7), ties=ties)
        want = rr.summary(RANKS, TIED, ks=(1, 3, 7), ties=ties)
        assert sorted(got) == sorted(want)
        for k, w in want.items():
            assert got[k] == pytest.approx(w, rel=1e-13), (ties, k)
    with pytest.raises(ValueError, match="needs the tied counts"):
        am.retrieval_summary(RANKS, ties="mean")


def rr_ties():
    return ("optimistic", "pessimistic", "mean")


def test_summary_drops_unranked_rows_and_warns_once(am):
    ranks = np.array([1, -1, 4, -1, 2, 30])
    tied = np.array([0, -1, 1, -1, 0, 0])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = am.retrieval_summary(ranks, tied, negatives=np.full(6, 99))
    assert len(caught) == 1 and caught[0].category is RuntimeWarning and "2 of 6" in str(caught[0].message)
    assert got["retrieval_rows_ranked"] == 4.0 and got["retrieval_rows_unranked"] == 2.0 and got["retrieval_ties"] == 1.0
    assert got["recall_at_1"] == 0.25 and got["recall_at_5"] == 0.75 and got["mean_rank"] == 9.25 and got["median_rank"] == 3.0
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        none = am.retrieval_summary(np.array([-1, -1]), np.array([-1, -1]))
    assert len(caught) == 1 and math.isnan(none["recall_at_1"]) and math.isnan(none["mrr"]) and none["retrieval_rows_ranked"] == 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                    # all ranked: silence
        am.retrieval_summary(RANKS, TIED)


def test_map_at_10_cuts_off_behind_rank_ten(am):
    got = am.retrieval_summary(np.array([1, 10, 11, 2]))
    assert got["map_at_10"] == pytest.approx((1.0 + 0.1 + 0.0 + 0.5) / 4, rel=1e-15)
    assert got["mrr"] == pytest.approx((1.0 + 0.1 + 1.0 / 11 + 0.5) / 4, rel=1e-15)
    assert am.retrieval_summary(np.array([10, 10]), np.array([1, 0]), ties="pessimistic")["map_at_10"] == pytest.approx(0.05)


def test_chance_recall_is_the_mean_of_k_over_the_candidates(am):
    negatives = np.array([0, 3, 9, 99])
    got = am.retrieval_summary(np.array([1, 1, 1, 1]), negatives=negatives)
    assert got["chance_recall_at_1"] == pytest.approx((1 + 1 / 4 + 1 / 10 + 1 / 100) / 4, rel=1e-15)
    assert got["chance_recall_at_5"] == pytest.approx((1 + 1 + 5 / 10 + 5 / 100) / 4, rel=1e-15)
    assert got["chance_recall_at_10"] == pytest.approx((1 + 1 + 1 + 10 / 100) / 4, rel=1e-15)
    assert "chance_recall_at_1" not in am.retrieval_summary(np.array([1, 2]))


def test_standard_errors_by_row_and_cluster_robust_against_a_direct_formula(am):
    rng = np.random.default_rng(3)
    ranks = rng.integers(1, 30, 60)
    ranks[[5, 17]] = -1
    tied = np.where(ranks > 0, rng.integers(0, 3, 60), -1)
    units = np.repeat(np.arange(12), 5) * 7 - 3                           # any integer values
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        by_row = am.retrieval_summary(ranks, tied)
        by_song = am.retrieval_summary(ranks, tied, units=units)
    keep = ranks > 0
    hit = (ranks[keep] <= 5).astype(float)
    assert by_row["recall_at_5_std_error"] == pytest.approx(hit.std(ddof=1) / math.sqrt(len(hit)), rel=1e-13)
    inv = 1.0 / ranks[keep]
    assert by_row["mrr_std_error"] == pytest.approx(inv.std(ddof=1) / math.sqrt(len(inv)), rel=1e-13)
    want = rr.summary(ranks, tied, units=units)
    for key in ("recall_at_1_std_error", "recall_at_5_std_error", "recall_at_10_std_error", "mrr_std_error"):
        assert by_song[key] == pytest.approx(want[key], rel=1e-12), key
        assert by_song[key] != pytest.approx(by_row[key], rel=1e-3), key
    # G / (G - 1) sum_g (sum_{i in g} (h_i - mean))^2 / n^2, written out for one figure
    total = 0.0
    for u in np.unique(units[keep]):
        total += float((hit[units[keep] == u] - hit.mean()).sum()) ** 2
    assert by_song["recall_at_5_std_error"] == pytest.approx(math.sqrt(12 / 11 * total) / len(hit), rel=1e-13)
    assert by_song["recall_at_5"] == by_row["recall_at_5"]
    one = am.retrieval_summary(np.array([1, 2, 3]), units=np.array([4, 4, 4]))
    assert math.isnan(one["mrr_std_error"]) and math.isnan(am.retrieval_summary(np.array([2]))["recall_at_1_std_error"])


def test_summary_argument_errors(am):
    with pytest.raises(ValueError, match="ties='best' is not one of"):
        am.retrieval_summary(RANKS, TIED, ties="best")
    with pytest.raises(ValueError, match="one value per query"):
        am.retrieval_summary(RANKS, TIED[:4])
    with pytest.raises(ValueError, match="ks="):
        am.retrieval_summary(RANKS, ks=(0,))


# ---------------------------------------------------------------------------------------------------- the reference
def test_reference_against_a_direct_loop():
    q, g = rr.lattice_rows(1, 9, 8), rr.lattice_rows(2, 14, 8)
    g[5] = 0.0                                                            # a zero-norm gallery row: no score under cosine
    q_labels = np.array([0, 1, 2, 3, 4, 0, 1, 7, 8])
    g_labels = np.array([0, 0, 1, 2, 2, 3, 9, 9, 4, 4, 4, 1, 0, 9])          # labels 7 and 8: no positive; label 3: column 5 only
    qg, gg = np.arange(9, dtype=np.int32) % 3, np.arange(14, dtype=np.int32) % 3
    for cosine in (True, False):
        u, wq = rr.lattice_scores(q, g, cosine)
        assert np.isnan(u[:, 5]).all() == cosine
        for groups in (None, (qg, gg)):
            got = rr.lattice_oracle(q, g, rr.label_positives(q_labels, g_labels), cosine, *(groups or ()))
            for i in range(9):
                pos = [j for j in range(14) if g_labels[j] == q_labels[i]]
                scored = [j for j in pos if not np.isnan(u[i, j])]
                neg = [j for j in range(14) if j not in pos and (groups is None or gg[j] != qg[i])]
                assert got["n_pos"][i] == len(pos) and got["negatives"][i] == len(neg)
                assert got["n_pos_own_group"][i] == (0 if groups is None else sum(gg[j] == qg[i] for j in pos))
                if not scored:
                    assert (got["better"][i], got["tied"][i], got["positive"][i]) == (-1, -1, -1) and np.isnan(got["score"][i])
                    continue
                t = max(u[i, j] for j in scored)
                assert got["positive"][i] == min(j for j in scored if u[i, j] == t)
                assert got["better"][i] == sum(u[i, j] > t for j in neg) and got["tied"][i] == sum(u[i, j] == t for j in neg)
                assert got["score"][i] == (t * wq[i] if cosine else t)
            assert (got["positive"][[7, 8]] == -1).all() and (got["positive"][3] == -1) == cosine


def test_f64_scores_and_their_error_bound_hold_for_the_f32_bits_of_lattice_rows():
    q, g = rr.lattice_rows(3, 20, 40), rr.lattice_rows(4, 30, 40)
    for cosine in (True, False):
        s, eps = rr.scores_f64(q, g, cosine)
        u, _ = rr.lattice_scores(q, g, cosine)
        assert np.all(np.abs(u.astype(np.float64) - s) <= eps)
    a, b = np.array([[3.0, 4.0]], np.float32), np.array([[6.0, 8.0], [4.0, -3.0]], np.float32)
    np.testing.assert_allclose(rr.scores_f64(a, b, True)[0], [[5.0, 0.0]], atol=1e-15)
    np.testing.assert_allclose(rr.scores_f64(a, b, False)[0], [[50.0, 0.0]], atol=1e-15)


def test_segments_list_every_row_once():
    starts, counts, cols = rr.segments([np.array([3, 1]), np.array([], np.int64), np.array([7])])
    assert starts.tolist() == [0, 2, 2] and counts.tolist() == [2, 0, 1] and cols.tolist() == [3, 1, 7]
    assert [p.tolist() for p in rr.label_positives([5, 6], [6, 5, 5])] == [[1, 2], [0]]


# ---------------------------------------------------------------------------------------------------- front end, before any device call
def test_front_end_argument_errors_need_no_device(am):
    q, g = torch.zeros(6, 8), torch.zeros(5, 8)
    with pytest.raises(ValueError, match="paired row by row, but queries holds 6 rows and gallery 5"):
        am.retrieval_scores(q, g)
    with pytest.raises(ValueError, match="query_labels holds 5 labels for 6 rows"):
        am.retrieval_scores(q, g, query_labels=np.arange(5), gallery_labels=np.arange(5))
    with pytest.raises(ValueError, match="groups without gallery_groups"):
        am.retrieval_scores(q, q, groups=np.arange(6))
    with pytest.raises(ValueError, match="gallery_groups without groups"):
        am.retrieval_scores(q, q, gallery_groups=np.arange(6))
    with pytest.raises(ValueError, match="query_labels without gallery_labels"):
        am.retrieval_scores(q, g, query_labels=np.arange(6))
    with pytest.raises(ValueError, match="gallery_labels must hold integer labels"):
        am.retrieval_scores(q, g, query_labels=np.arange(6), gallery_labels=np.arange(5) * 0.5)
    with pytest.raises(ValueError, match="groups must hold integer labels"):
        am.retrieval_scores(q, q, groups=torch.zeros(6), gallery_groups=np.arange(6))
    with pytest.raises(ValueError, match="similarity='euclid' is not one of"):
        am.retrieval_scores(q, q, similarity="euclid")
    with pytest.raises(ValueError, match="ties='best' is not one of"):
        am.retrieval_scores(q, q, ties="best")
    with pytest.raises(ValueError, match="feature widths differ"):
        am.retrieval_scores(q, torch.zeros(6, 4))
    with pytest.raises(NotImplementedError, match="float32 rows"):
        am.retrieval_scores(q.double(), q.double())
    with pytest.raises(ValueError, match="keeps none"):
        am.retrieval_scores(am.AudioMetricsData(False), q)
    with pytest.raises(NotImplementedError, match="float32 rows"):
        am.hip_ops.retrieval_ranks(q.double(), q.double(), None, None, None)
    assert "retrieval_scores" not in am.AudioMetrics.__dict__                 # a function of two paired sets, no metric name


# ---------------------------------------------------------------------------------------------------- host side of the C ABI
def test_workspace_and_chunk_queries_are_host_calls(am, lib):
    assert lib.am_retrieval_workspace_bytes(100000, 100000, 512) > 0
    assert lib.am_retrieval_workspace_bytes(100000, 100000, 512) >= 2 * 4 * 100000 * lib.am_retrieval_chunks(100000, 100000, 512)
    assert lib.am_retrieval_chunks(100000, 100000, 512) >= 8 and am.hip_ops.retrieval_chunks(130, 4000, 40) > 1
    assert am.hip_ops.retrieval_chunks(130, 300, 40) == lib.am_sample_scores_chunks(130, 300, 40)      # one plan
    for shape in ((0, 10, 8), (10, 0, 8), (10, 10, 0), (10, 1 << 31, 8)):
        assert lib.am_retrieval_workspace_bytes(*shape) == 0 and lib.am_retrieval_chunks(*shape) == 0, shape
    assert lib.am_retrieval_workspace_bytes(10, (1 << 31) - 1, 8) > 0


def call(lib, n=130, m=300, d=40, ld=40, **kw):
    a = dict(Q=FAKE, G=FAKE, pos_start=FAKE, pos_count=FAKE, pos_columns=FAKE, n_pos_columns=n, q_group=None, g_group=None,
             out_better=FAKE, out_tied=FAKE, out_score=FAKE, out_positive=FAKE, out_n_pos=FAKE, out_n_pos_own_group=FAKE,
             ws=FAKE, ws_bytes=0)
    a.update(kw)
    rc = lib.am_retrieval_ranks_f32(a["Q"], n, ld, a["G"], m, ld, d, 1, a["pos_start"], a["pos_count"], a["pos_columns"],
                                    a["n_pos_columns"], a["q_group"], a["g_group"], a["out_better"], a["out_tied"], a["out_score"],
                                    a["out_positive"], a["out_n_pos"], a["out_n_pos_own_group"], a["ws"], a["ws_bytes"], None)
    return rc, lib.am_last_error().decode()


def test_entry_point_validates_before_any_device_work(lib):
    rc, msg = call(lib)
    assert rc == WORKSPACE and "am_retrieval_workspace_bytes" in msg and str(lib.am_retrieval_workspace_bytes(130, 300, 40)) in msg, msg
    for name in ("Q", "G", "pos_start", "pos_count", "pos_columns", "out_better", "out_tied", "out_score", "out_positive", "out_n_pos",
                 "out_n_pos_own_group"):
        rc, msg = call(lib, **{name: None})
        assert rc == BAD_ARG and msg.startswith(name + " is null"), (name, rc, msg)
    # group ids go with both sides or neither
    rc, msg = call(lib, q_group=FAKE)
    assert rc == BAD_ARG and "g_group is null" in msg, msg
    rc, msg = call(lib, g_group=FAKE)
    assert rc == BAD_ARG and "q_group is null" in msg, msg
    assert call(lib, q_group=FAKE, g_group=FAKE)[0] == WORKSPACE
    assert call(lib, n_pos_columns=-1)[0] == BAD_ARG
    assert call(lib, n_pos_columns=0, pos_columns=None)[0] == WORKSPACE        # no entries: nothing to point at
    assert call(lib, ld=42)[0] == BAD_ARG and call(lib, d=44)[0] == BAD_ARG     # ld % 4, ld >= D
    assert call(lib, n=0)[0] == BAD_SHAPE
    rc, msg = call(lib, m=1 << 31)
    assert rc == BAD_SHAPE and "M < 2^31" in msg, msg
