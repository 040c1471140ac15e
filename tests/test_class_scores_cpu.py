"""The classifier-output scores (Inception Score, paired KL, paired cosine), the part that needs no GPU: the float64 oracle of
tests/class_scores_reference.py against closed forms and scipy, the host helpers of metrics/classifier.py, validation before
any device call in both layers, the new names in header / signature table / package, the entry points' error paths and
workspace queries through the loaded library, and the front end's logic with the two device operations replaced by host
functions that call the oracle."""
import ctypes
import inspect
import math
import os
import re
import warnings

import numpy as np
import pytest
import torch

import class_scores_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -4
FAKE = ctypes.c_void_p(0x10000)                       # 16-byte aligned, never dereferenced: the calls stop at validation
NAMES = ("am_class_groups_workspace_bytes", "am_class_groups_f32", "am_class_groups_f64", "am_row_pairs_workspace_bytes",
         "am_row_pairs_f32", "am_row_pairs_f64")


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


# ---------------------------------------------------------------------------------------------------- the oracle itself
def test_the_oracle_closed_forms_of_the_inception_score():
    for c, n in ((7, 12), (527, 5)):
        got = ref.class_groups(np.full((n, c), 3.25), [range(n)])
        assert abs(got["log_is"][0]) <= 4 * 2.0 ** -53 * math.log(c) and got["mean_h"][0] == pytest.approx(-math.log(c), rel=1e-15)
        assert ref.pair_value(np.full(c, 3.25), np.full(c, -1.5), "kl_softmax")[0] == 0.0          # constant rows: both uniform
    for c in (2, 5, 40):
        prev = 1.0
        for t in (0.5, 2.0, 8.0, 30.0, 60.0):
            logits = t * np.eye(c)
            a, b = math.exp(t) / (math.exp(t) + c - 1), 1.0 / (math.exp(t) + c - 1)
            want = math.exp(math.log(c) + a * math.log(a) + (c - 1) * b * math.log(b))
            got = math.exp(ref.class_groups(logits, [range(c)])["log_is"][0])
            assert got == pytest.approx(want, rel=1e-13) and prev < got <= c * (1 + 1e-15), (c, t, got, want)
            prev = got
        assert prev == pytest.approx(c, rel=1e-12)                                                 # IS -> C as t grows
    rng = np.random.default_rng(0)
    for n, c in ((1, 9), (3, 50), (40, 4), (25, 25)):
        logits = rng.standard_normal((n, c)) * 6
        got = ref.inception(logits, splits=1)
        assert 1.0 - 1e-12 <= got["inception_score"] <= min(c, n) * (1 + 1e-12), (n, c, got["inception_score"])
        assert got["inception_marginal_entropy"] - got["inception_conditional_entropy"] == pytest.approx(
            math.log(got["inception_score"]), abs=1e-13)
        assert np.all(got["row_entropy"] >= 0) and np.all(got["row_entropy"] <= math.log(c) * (1 + 1e-15))


def test_the_oracle_edge_rules():
    h, p, _ = ref.row_quantities([0.0, -np.inf, 0.0])                     # a masked class
    assert h == pytest.approx(-math.log(2), rel=1e-15) and float(p[1]) == 0.0 and float(p[0]) == 0.5
    h, p, _ = ref.row_quantities([-np.inf, 2.5, -np.inf])                 # all but one class masked: a point mass
    assert h == 0.0 and float(p[1]) == 1.0
    for bad in ([0.0, np.nan], [np.inf, 0.0], [-np.inf, -np.inf]):
        assert math.isnan(ref.row_quantities(bad)[0]) and not ref.row_is_finite(bad)
    g = ref.class_groups(np.array([[0.0, 1.0], [np.nan, 0.0], [1.0, 0.0]]), [[0, 2], [1, 2]])
    assert g["nonfinite"].tolist() == [0, 1] and math.isnan(g["log_is"][1]) and math.isfinite(g["log_is"][0])
    assert math.isnan(g["h"][1][0]) and math.isfinite(g["h"][1][1])
    assert ref.row_quantities(np.array([1e3, -1e3, 0.0]) * 1e3)[0] == 0.0                       # far underflow: a point mass
    # kl_softmax: p^r_c = 0 drops the term, a masked candidate class under p^r_c > 0 gives +inf
    assert ref.pair_value([0.0, -np.inf], [0.0, -np.inf], "kl_softmax")[0] == 0.0
    assert ref.pair_value([0.0, -np.inf], [0.0, 0.0], "kl_softmax")[0] == math.inf
    assert ref.pair_value([0.0, 0.0], [0.0, -np.inf], "kl_softmax")[0] == pytest.approx(math.log(2), rel=1e-15)
    assert ref.pair_value([5e5, 0.0], [-5e5, 0.0], "kl_softmax")[0] == pytest.approx(5e5, rel=1e-15)   # finite however far


def test_the_oracle_paired_values():
    rng = np.random.default_rng(1)
    scipy_stats = pytest.importorskip("scipy.stats")
    for c in (1, 3, 64, 527):
        r, q = rng.standard_normal(c) * 3, rng.standard_normal(c) * 3
        p_r, p_q = np.exp(r - r.max()), np.exp(q - q.max())
        want = scipy_stats.entropy(p_r / p_r.sum(), p_q / p_q.sum())
        got, scale = ref.pair_value(q, r, "kl_softmax")
        assert abs(got - want) <= (c + 16) * 2.0 ** -52 * scale, (c, got, want)
        eps = 1e-3
        with_eps = ref.pair_value(q, r, "kl_softmax", eps)[0]
        direct = float(np.sum(p_r / p_r.sum() * (np.log(p_r / p_r.sum()) - np.log(p_q / p_q.sum() + eps))))
        assert with_eps == pytest.approx(direct, abs=1e-13) and with_eps < got + 1e-15
        assert ref.pair_value(r, r, "kl_softmax")[0] == 0.0 and ref.pair_value(r, r, "kl_softmax", eps)[0] <= 0.0
        bern = ref.pair_value(q, r, "kl_bernoulli")[0]
        s, t = 1 / (1 + np.exp(-r)), 1 / (1 + np.exp(-q))
        assert bern >= 0.0 and bern == pytest.approx(float(np.sum(s * np.log(s / t) + (1 - s) * np.log((1 - s) / (1 - t)))), rel=1e-12)
        assert ref.pair_value(q, r, "kl_sigmoid")[0] == pytest.approx(float(np.sum(s * np.log(s / t))), rel=1e-12, abs=1e-14)
        assert ref.pair_value(r, r, "kl_bernoulli")[0] == 0.0 and ref.pair_value(r, r, "kl_sigmoid")[0] == 0.0
        assert ref.pair_value(r, r, "cosine")[0] == pytest.approx(1.0, abs=2.0 ** -52)
        assert ref.pair_value(r, -r, "cosine")[0] == pytest.approx(-1.0, abs=2.0 ** -52)
    # the one-term sigmoid form is not a divergence: a candidate surer than the reference makes it negative
    neg = ref.pair_value(np.full(4, 9.0), np.zeros(4), "kl_sigmoid")[0]
    assert neg < 0 and neg == pytest.approx(4 * 0.5 * (math.log(0.5) - math.log(1 / (1 + math.exp(-9.0)))), rel=1e-14)
    assert ref.pair_value(np.full(4, 9.0), np.zeros(4), "kl_bernoulli")[0] > 0
    assert ref.pair_value([800.0, -800.0], [-800.0, 800.0], "kl_bernoulli")[0] == pytest.approx(1600.0, rel=1e-15)   # stable forms
    for mode in ref.MODES:
        assert math.isnan(ref.pair_value([0.0, np.nan], [0.0, 1.0], mode)[0]), mode
    assert math.isnan(ref.pair_value([0.0, 0.0], [1.0, 2.0], "cosine")[0])


# ---------------------------------------------------------------------------------------------------- host helpers
def test_split_offsets(am):
    from audio_metrics_amd.metrics.classifier import split_offsets
    for n, splits in ((10, 10), (10, 3), (103, 10), (7, 1), (1, 1), (100_000, 10), (65, 64)):
        offs = split_offsets(n, splits)
        assert offs == [k * n // splits for k in range(splits + 1)] and offs[0] == 0 and offs[-1] == n
        assert all(b > a for a, b in zip(offs, offs[1:])) and max(np.diff(offs)) - min(np.diff(offs)) <= 1
        assert [len(p) for p in ref.split_plan(n, splits)] == np.diff(offs).tolist()
    for n, splits in ((5, 0), (5, 6), (5, -1), (0, 1)):
        with pytest.raises(ValueError, match="splits="):
            split_offsets(n, splits)


def test_inception_summary_and_paired_summary(am):
    from audio_metrics_amd.metrics.classifier import inception_summary, paired_summary, rows_by_group
    got = inception_summary(np.log([2.0, 4.0, 3.0]), [10, 10, 20], [-0.5, -0.25, -1.0], [-1.5, -2.0, -2.5])
    assert got["inception_score"] == pytest.approx(3.0, rel=1e-15) and got["inception_n_splits"] == 3
    assert got["inception_score_std"] == pytest.approx(math.sqrt(2.0 / 3.0), rel=1e-15)               # ddof = 0
    assert np.allclose(got["inception_score_per_split"], [2.0, 4.0, 3.0], rtol=1e-15)
    assert got["inception_conditional_entropy"] == pytest.approx((5.0 + 2.5 + 20.0) / 40, rel=1e-15)
    assert got["inception_marginal_entropy"] == pytest.approx((15.0 + 20.0 + 50.0) / 40, rel=1e-15)
    one = inception_summary([math.log(2.5)], [7], [-0.1], [-1.0])
    assert one["inception_score"] == pytest.approx(2.5, rel=1e-15) and one["inception_score_std"] == 0.0
    nan = inception_summary([0.5, math.nan], [3, 3], [-0.1, math.nan], [-1.0, math.nan])
    assert math.isnan(nan["inception_score"]) and math.isnan(nan["inception_score_std"]) and nan["inception_score_per_split"][0] == pytest.approx(math.exp(0.5), rel=1e-15)
    with pytest.raises(ValueError):
        inception_summary([], [], [], [])

    v = np.array([1.0, 2.0, 4.0, 9.0])
    mean, se, used, left = paired_summary([v.sum(), (v * v).sum(), 4, 2])
    assert (mean, used, left) == (4.0, 4, 2) and se == pytest.approx(math.sqrt(((v - 4.0) ** 2).sum() / 3 / 4), rel=1e-15)
    assert paired_summary([v.sum(), (v * v).sum(), 4, 2])[:2] == pytest.approx(ref.paired_summary(list(v) + [math.nan, math.inf])[:2], rel=1e-15)
    mean, se, used, left = paired_summary([2.5, 6.25, 1, 0])
    assert mean == 2.5 and math.isnan(se) and (used, left) == (1, 0)                                   # fewer than 2 rows
    mean, se, used, left = paired_summary([0.0, 0.0, 0, 3])
    assert math.isnan(mean) and math.isnan(se) and (used, left) == (0, 3)
    assert paired_summary([3.0, 3.0 - 1e-9, 3, 0])[1] == 0.0                                          # cancellation never goes negative

    labels, sizes, means = rows_by_group([7, 3, 7, 3, 5, 7], [1.0, 2.0, math.nan, 4.0, math.inf, 5.0])
    assert labels.tolist() == [3, 5, 7] and sizes.tolist() == [2, 1, 3] and means[0] == 3.0 and math.isnan(means[1]) and means[2] == 3.0
    with pytest.raises(ValueError):
        rows_by_group([1.5, 2.5], [0.0, 0.0])
    with pytest.raises(ValueError):
        rows_by_group([1, 2], [0.0])


# ---------------------------------------------------------------------------------------------------- validation
def test_validation_happens_before_any_device_call(am, monkeypatch):
    from audio_metrics_amd import hip_ops

    def forbidden(*a, **k):
        raise AssertionError("device call before validation")
    for name in ("as_matrix", "as_matrix64", "_call", "_workspace", "upload_host_array", "_group_index"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    x, y = torch.zeros((10, 8)), torch.zeros((10, 8))
    for bad in (torch.zeros(8), torch.zeros((2, 3, 4)), np.zeros((4, 4))):
        with pytest.raises(ValueError, match="2-D"):
            hip_ops.class_group_scores(bad, None, [0, 1])
        with pytest.raises(ValueError, match="2-D"):
            hip_ops.row_pair_scores(bad, bad, "cosine")
    for bad in (x.to(torch.float16), x.to(torch.int64)):
        with pytest.raises(ValueError, match="float32 or float64"):
            hip_ops.class_group_scores(bad, None, [0, 10])
        with pytest.raises(ValueError, match="float32 or float64"):
            hip_ops.row_pair_scores(bad, bad, "cosine")
    for bad in (torch.zeros((0, 8)), torch.zeros((4, 0)), torch.zeros((1, 2049))):
        with pytest.raises(ValueError, match="1 .. 2048 columns"):
            hip_ops.class_group_scores(bad, None, [0, 1])
    for bad in (torch.zeros((0, 8)), torch.zeros((4, 0)), torch.zeros((1, 8193))):
        with pytest.raises(ValueError, match="1 .. 8192 columns"):
            hip_ops.row_pair_scores(bad, bad, "cosine")
    for offs in ([0], [1, 10], [0, 5, 5, 10], [0, 10, 5]):
        with pytest.raises(ValueError, match="offsets"):
            hip_ops.class_group_scores(x, None, offs)
    with pytest.raises(ValueError, match="no index list"):
        hip_ops.class_group_scores(x, None, [0, 11])
    for a, b in ((x, y.double()), (x.double(), y)):
        with pytest.raises(NotImplementedError, match="one dtype"):
            hip_ops.row_pair_scores(a, b, "kl_softmax")
    for other in (torch.zeros((9, 8)), torch.zeros((10, 12))):
        with pytest.raises(ValueError, match="paired one to one"):
            hip_ops.row_pair_scores(x, other, "cosine")
    for bad in ("softmax", "kl", None, 1):
        with pytest.raises(ValueError, match="mode="):
            hip_ops.row_pair_scores(x, y, bad)
    for bad in (-1e-9, math.inf, math.nan, "tiny", None):
        with pytest.raises(ValueError, match="eps="):
            hip_ops.row_pair_scores(x, y, "kl_softmax", bad)
    for call in (lambda: hip_ops.class_group_scores(x, None, [0, 4, 10]), lambda: hip_ops.class_group_scores(x.double(), None, [0, 10]),
                 lambda: hip_ops.row_pair_scores(x, y, "kl_sigmoid", 1e-6), lambda: hip_ops.row_pair_scores(x.double(), y.double(), "cosine")):
        with pytest.raises(AssertionError, match="device call before validation"):       # past the checks: the device operations
            call()

    # the front end: with the two operations forbidden too
    for name in ("class_group_scores", "row_pair_scores"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    ok, other = host_set(am, torch.randn((10, 8))), host_set(am, torch.randn((10, 8)))
    for empty in (am.AudioMetricsData(False), host_set(am, torch.zeros((0, 8))), torch.zeros(8)):
        for call in (lambda: am.inception_score(empty), lambda: am.inception_score_per_group(empty, [0] * 10),
                     lambda: am.kl_divergence_paired(empty, ok), lambda: am.kl_divergence_paired(ok, empty),
                     lambda: am.paired_cosine_score(empty, ok), lambda: am.paired_cosine_score(ok, empty)):
            with pytest.raises(ValueError, match="keeps none"):
                call()
    for bad in (0, 11, -2):
        with pytest.raises(ValueError, match="splits="):
            am.inception_score(ok, splits=bad)
    with pytest.raises(ValueError, match="1 .. 2048 columns"):
        am.inception_score(torch.zeros((4, 2049)), splits=2)
    with pytest.raises(ValueError, match="1 .. 2048 columns"):
        am.inception_score_per_group(torch.zeros((4, 2049)), [0, 0, 1, 1])
    with pytest.raises(ValueError, match="float32 or float64"):
        am.inception_score(torch.zeros((4, 8), dtype=torch.float16), splits=2)
    with pytest.raises(ValueError, match="one label per row"):
        am.inception_score_per_group(ok, [0] * 9)
    with pytest.raises(ValueError, match="integer labels"):
        am.inception_score_per_group(ok, np.linspace(0, 1, 10))
    for fn in (am.kl_divergence_paired, am.paired_cosine_score):
        with pytest.raises(ValueError, match="paired row by row"):
            fn(ok, host_set(am, torch.randn((9, 8))))
        with pytest.raises(ValueError, match="paired one to one"):
            fn(ok, host_set(am, torch.randn((10, 12))))
        with pytest.raises(NotImplementedError, match="one dtype"):
            fn(ok, host_set(am, torch.randn((10, 8)).double()))
        with pytest.raises(ValueError, match="one label per row"):
            fn(ok, other, groups=[0] * 9)
        with pytest.raises(ValueError, match="1 .. 8192 columns"):
            fn(torch.zeros((2, 8193)), torch.zeros((2, 8193)))
    for bad in ("kl_softmax", "cosine", None):
        with pytest.raises(ValueError, match="mode="):
            am.kl_divergence_paired(ok, other, mode=bad)
    for bad in (-1e-9, math.inf, math.nan):
        with pytest.raises(ValueError, match="eps="):
            am.kl_divergence_paired(ok, other, eps=bad)
    for call in (lambda: am.inception_score(ok), lambda: am.kl_divergence_paired(ok, other), lambda: am.paired_cosine_score(ok, other)):
        with pytest.raises(AssertionError, match="device call before validation"):
            call()


# ---------------------------------------------------------------------------------------------------- the front end on host stand-ins
class HostOps:
    """Host stand-ins of the two device operations, calling the oracle and recording what they were given."""

    def __init__(self):
        self.group_calls, self.pair_calls = [], []

    def install(self, monkeypatch, hip_ops):
        monkeypatch.setattr(hip_ops, "as_matrix", lambda e, name="": e)
        monkeypatch.setattr(hip_ops, "as_matrix64", lambda e, name="": e)
        monkeypatch.setattr(hip_ops, "upload_host_array", lambda a, device: torch.as_tensor(np.ascontiguousarray(a)))
        monkeypatch.setattr(hip_ops, "class_group_scores", self.groups)
        monkeypatch.setattr(hip_ops, "row_pair_scores", self.pairs)

    def groups(self, rows, order, offsets, return_rows=False):
        offs = [int(o) for o in offsets]
        listed = np.arange(offs[-1]) if order is None else order.numpy()
        self.group_calls.append((None if order is None else order.numpy().copy(), offs, return_rows))
        g = ref.class_groups(rows.numpy(), [listed[a:b] for a, b in zip(offs, offs[1:])])
        rec = np.stack([g["mean_h"], g["marginal"], g["log_is"], g["nonfinite"]], axis=1)
        h = torch.as_tensor(np.concatenate(g["h"])) if return_rows else None
        return torch.as_tensor(rec), h, lambda: None

    def pairs(self, a, b, mode, eps=0.0, return_rows=False):
        self.pair_calls.append((mode, eps, return_rows))
        v = ref.pair_rows(a.numpy(), b.numpy(), mode, eps)[0]
        fin = v[np.isfinite(v)]
        sums = torch.tensor([fin.sum(), (fin * fin).sum(), float(fin.size), float(v.size - fin.size)], dtype=torch.float64)
        return sums, (torch.as_tensor(v) if return_rows else None)


def test_inception_front_end_on_host_stand_ins(am, monkeypatch):
    from audio_metrics_amd import hip_ops
    host = HostOps()
    host.install(monkeypatch, hip_ops)
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((53, 9)) * 2).astype(np.float32)
    for data in (host_set(am, torch.as_tensor(x)), torch.as_tensor(x), torch.as_tensor(x).double()):
        host.group_calls.clear()
        got = am.inception_score(data, splits=5, return_rows=True)
        want = ref.inception(x, 5)
        order, offs, _ = host.group_calls[0]
        assert order is None and offs == [k * 53 // 5 for k in range(6)] and len(host.group_calls) == 1
        for key in ("inception_score", "inception_score_std", "inception_conditional_entropy", "inception_marginal_entropy"):
            assert got[key] == pytest.approx(want[key], rel=1e-14), key
        assert np.allclose(got["inception_score_per_split"], want["inception_score_per_split"], rtol=1e-14)
        assert np.array_equal(got["row_entropy"], want["row_entropy"]) and got["inception_n_splits"] == 5
        assert set(got) == {"inception_score", "inception_score_std", "inception_score_per_split", "inception_conditional_entropy",
                            "inception_marginal_entropy", "inception_n_splits", "row_entropy"}
    # a seed: the permutation of numpy's default_rng is the index list, row results come back in stored order
    host.group_calls.clear()
    got = am.inception_score(torch.as_tensor(x), splits=4, seed=3, return_rows=True)
    order, offs, _ = host.group_calls[0]
    assert np.array_equal(order, np.random.default_rng(3).permutation(53)) and order.dtype == np.int64
    want = ref.inception(x, 4, seed=3)
    assert np.allclose(got["inception_score_per_split"], want["inception_score_per_split"], rtol=1e-14)
    assert np.array_equal(got["row_entropy"], want["row_entropy"])
    assert np.array_equal(got["row_entropy"], am.inception_score(torch.as_tensor(x), splits=1, return_rows=True)["row_entropy"])
    assert "row_entropy" not in am.inception_score(torch.as_tensor(x), splits=4, seed=3) and host.group_calls[-1][2] is False
    # groups: any labels in any order; the list is the stable sort by label
    labels = rng.integers(-2, 4, 53) * 10
    got = am.inception_score_per_group(torch.as_tensor(x), labels)
    uniq = np.unique(labels)
    assert got["group_labels"].tolist() == uniq.tolist() and got["group_sizes"].tolist() == [int((labels == u).sum()) for u in uniq]
    want = ref.class_groups(x, [np.flatnonzero(labels == u) for u in uniq])
    assert np.array_equal(host.group_calls[-1][0], np.argsort(labels, kind="stable"))
    assert np.array_equal(got["inception_log_per_group"], want["log_is"])
    assert np.array_equal(got["inception_score_per_group"], np.exp(want["log_is"]))
    assert set(got) == {"inception_score_per_group", "inception_log_per_group", "group_labels", "group_sizes"}


def test_front_end_warnings_fire_once(am, monkeypatch):
    from audio_metrics_amd import hip_ops
    HostOps().install(monkeypatch, hip_ops)
    rng = np.random.default_rng(4)
    x = rng.standard_normal((40, 6)).astype(np.float32)
    x[3, 1], x[4, 0], x[25] = np.nan, np.inf, -np.inf
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = am.inception_score(torch.as_tensor(x), splits=4, return_rows=True)
    assert len(caught) == 1 and issubclass(caught[0].category, RuntimeWarning) and "3 rows" in str(caught[0].message)
    assert np.isnan(got["inception_score_per_split"]).tolist() == [True, False, True, False] and math.isnan(got["inception_score"])
    assert np.flatnonzero(np.isnan(got["row_entropy"])).tolist() == [3, 4, 25]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        per = am.inception_score_per_group(torch.as_tensor(x), np.arange(40) // 5)
    assert len(caught) == 1 and "2 of 8 groups" in str(caught[0].message)
    assert np.flatnonzero(np.isnan(per["inception_score_per_group"])).tolist() == [0, 5]
    y = rng.standard_normal((40, 6)).astype(np.float32)
    for fn, key, words in ((am.kl_divergence_paired, "kl", "3 of 40 row pairs"), (am.paired_cosine_score, "cosine_score", "3 of 40 row pairs")):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            got = fn(torch.as_tensor(y), torch.as_tensor(x), return_rows=True)
        assert len(caught) == 1 and issubclass(caught[0].category, RuntimeWarning) and words in str(caught[0].message), key
        prefix = "kl" if key == "kl" else "cosine"
        assert got[prefix + "_rows_used"] == 37 and got[prefix + "_rows_nonfinite"] == 3 and math.isfinite(got[key])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        am.kl_divergence_paired(torch.as_tensor(y), torch.as_tensor(y + 1))
        am.inception_score(torch.as_tensor(y))
    assert caught == []


def test_paired_front_end_on_host_stand_ins(am, monkeypatch):
    from audio_metrics_amd import hip_ops
    host = HostOps()
    host.install(monkeypatch, hip_ops)
    rng = np.random.default_rng(5)
    c, r = rng.standard_normal((31, 7)).astype(np.float32), rng.standard_normal((31, 7)).astype(np.float32)
    labels = rng.integers(0, 4, 31)
    for mode in ("softmax", "sigmoid", "bernoulli"):
        for eps in (0.0, 1e-6):
            host.pair_calls.clear()
            got = am.kl_divergence_paired(host_set(am, torch.as_tensor(c)), host_set(am, torch.as_tensor(r)), mode=mode, eps=eps)
            assert host.pair_calls == [("kl_" + mode, eps, False)]                             # only the four sums are read back
            v = ref.pair_rows(c, r, "kl_" + mode, eps)[0]
            mean, se, used, left = ref.paired_summary(v)
            assert got["kl"] == pytest.approx(mean, rel=1e-13) and got["kl_std_error"] == pytest.approx(se, rel=1e-9)
            assert (got["kl_mode"], got["kl_eps"], got["kl_rows_used"], got["kl_rows_nonfinite"]) == (mode, eps, 31, 0)
            assert set(got) == {"kl", "kl_std_error", "kl_mode", "kl_eps", "kl_rows_used", "kl_rows_nonfinite"}
    got = am.kl_divergence_paired(torch.as_tensor(c), torch.as_tensor(r), groups=labels, return_rows=True)
    v = ref.pair_rows(c, r, "kl_softmax")[0]
    assert host.pair_calls[-1] == ("kl_softmax", 0.0, True) and np.array_equal(got["kl_rows"], v)
    assert got["group_labels"].tolist() == np.unique(labels).tolist() and got["group_sizes"].sum() == 31
    assert np.allclose(got["kl_per_group"], [v[labels == u].mean() for u in np.unique(labels)], rtol=1e-14)
    only_groups = am.kl_divergence_paired(torch.as_tensor(c), torch.as_tensor(r), groups=torch.as_tensor(labels))
    assert "kl_rows" not in only_groups and np.array_equal(only_groups["kl_per_group"], got["kl_per_group"])
    one = am.kl_divergence_paired(torch.as_tensor(c[:1]), torch.as_tensor(r[:1]))
    assert one["kl"] == pytest.approx(v[0], rel=1e-14) and math.isnan(one["kl_std_error"])              # fewer than 2 rows
    cos = am.paired_cosine_score(torch.as_tensor(c), torch.as_tensor(r), groups=labels, return_rows=True)
    w = ref.pair_rows(c, r, "cosine")[0]
    assert host.pair_calls[-1] == ("cosine", 0.0, True) and np.array_equal(cos["cosine_rows"], w)
    assert cos["cosine_score"] == pytest.approx(w.mean(), rel=1e-13) and cos["cosine_score_std_error"] == pytest.approx(w.std(ddof=1) / math.sqrt(31), rel=1e-9)
    assert set(cos) == {"cosine_score", "cosine_score_std_error", "cosine_rows_used", "cosine_rows_nonfinite", "cosine_score_per_group",
                        "group_labels", "group_sizes", "cosine_rows"}
    assert np.allclose(cos["cosine_score_per_group"], [w[labels == u].mean() for u in np.unique(labels)], rtol=1e-14)


# ---------------------------------------------------------------------------------------------------- names
def test_header_signature_table_and_package_agree(am, lib):
    with open(os.path.join(ROOT, "include", "audio_metrics_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in am._lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"enum am_pair_mode \{ AM_PAIR_COSINE = 0, AM_PAIR_KL_SOFTMAX = 1, AM_PAIR_KL_SIGMOID = 2, AM_PAIR_KL_BERNOULLI = 3 \}", header)
    assert am.hip_ops.PAIR_MODES == {"cosine": 0, "kl_softmax": 1, "kl_sigmoid": 2, "kl_bernoulli": 3}
    from audio_metrics_amd.metrics import classifier
    for name in ("inception_score", "inception_score_per_group", "kl_divergence_paired", "paired_cosine_score"):
        assert getattr(am, name) is getattr(classifier, name), name
    assert am.metrics.classifier is classifier
    assert all(callable(getattr(classifier, n)) for n in ("split_offsets", "inception_summary", "paired_summary", "rows_by_group"))
    assert all(callable(getattr(am.hip_ops, n)) for n in ("class_group_scores", "row_pair_scores"))
    source = inspect.getsource(am.audio_metrics).lower()                    # calls, not metric names of AudioMetrics
    assert "inception" not in source and "cosine_score" not in source and "kl_divergence" not in source


# ---------------------------------------------------------------------------------------------------- entry points
@pytest.mark.parametrize("suffix", ["f32", "f64"])
def test_entry_point_error_paths_and_workspaces(lib, suffix):
    def offsets(*values):
        return ctypes.cast((ctypes.c_int64 * len(values))(*values), ctypes.c_void_p)
    nb = lib.am_class_groups_workspace_bytes(130, 2, 40)
    # the head (flag word, B + 1 offsets, B + 1 segment counts), then (n_total + 63 B) / 64 segments of C + 2 doubles
    assert nb == 256 + (((130 + 63 * 2) // 64) * 42 * 8 + 255) // 256 * 256
    assert lib.am_class_groups_workspace_bytes(100_000, 10, 527) == (8 + 2 * 11 * 8 + 255) // 256 * 256 + (1572 * 529 * 8 + 255) // 256 * 256
    for bad in ((0, 2, 40), (130, 0, 40), (130, 2, 0), (130, 2, 2049)):
        assert lib.am_class_groups_workspace_bytes(*bad) == 0, bad
    assert lib.am_class_groups_workspace_bytes(1, 1, 2048) > 0
    groups_fn = getattr(lib, "am_class_groups_" + suffix)

    def groups(x=FAKE, n=130, ld=40, c=40, idx=None, offs=(0, 70, 130), rec=FAKE, h=None, ws=FAKE, nb=nb):
        return groups_fn(x, n, ld, c, idx, offsets(*offs) if offs is not None else None, len(offs) - 1 if offs else 1, rec, h, ws, nb, None)
    for null in ("x", "rec", "offs"):
        assert groups(**{null: None}) == BAD_ARG, null
    assert groups(c=0) == BAD_SHAPE and groups(c=2049, ld=2052) == BAD_SHAPE and "2048" in lib.am_last_error().decode()
    assert groups(n=0) == BAD_SHAPE
    assert groups(ld=36) == BAD_ARG
    if suffix == "f32":
        assert groups(x=ctypes.c_void_p(0x10004)) == BAD_ARG and groups(ld=42) == BAD_ARG           # misaligned rows
        assert groups(n=1 << 25, ld=64, c=40) == BAD_SHAPE and "32-bit" in lib.am_last_error().decode()
    assert groups(offs=(1, 70, 130)) == BAD_ARG and "offsets[0]" in lib.am_last_error().decode()
    assert groups(offs=(0, 70, 70)) == BAD_SHAPE and groups(offs=(0, 70, 60)) == BAD_SHAPE          # an empty group
    assert groups(offs=(0, 70, 131)) == BAD_SHAPE and "no index list" in lib.am_last_error().decode()
    assert groups(nb=nb - 1) == WORKSPACE and groups(ws=None) == WORKSPACE                          # a short workspace

    nbp = lib.am_row_pairs_workspace_bytes(130)
    assert nbp == 256 and lib.am_row_pairs_workspace_bytes(100_000) == (1563 * 32 + 255) // 256 * 256
    assert lib.am_row_pairs_workspace_bytes(0) == 0 and lib.am_row_pairs_workspace_bytes(-5) == 0
    pairs_fn = getattr(lib, "am_row_pairs_" + suffix)

    def pairs(a=FAKE, lda=40, b=FAKE, ldb=44, n=130, c=40, mode=1, eps=0.0, rows=None, sums=FAKE, ws=FAKE, nb=nbp):
        return pairs_fn(a, lda, b, ldb, n, c, mode, eps, rows, sums, ws, nb, None)
    for null in ("a", "b", "sums"):
        assert pairs(**{null: None}) == BAD_ARG, null
    for bad in (-1, 4, 17):
        assert pairs(mode=bad) == BAD_ARG and "mode=" in lib.am_last_error().decode()
    for bad in (-1e-12, math.inf, math.nan):
        assert pairs(eps=bad) == BAD_ARG and "eps=" in lib.am_last_error().decode()
    assert pairs(c=0) == BAD_SHAPE and pairs(c=8193, lda=8196, ldb=8196) == BAD_SHAPE and pairs(n=0) == BAD_SHAPE
    assert pairs(lda=36) == BAD_ARG and pairs(ldb=36) == BAD_ARG
    if suffix == "f32":
        assert pairs(a=ctypes.c_void_p(0x10004)) == BAD_ARG and pairs(b=ctypes.c_void_p(0x10008)) == BAD_ARG and pairs(ldb=42) == BAD_ARG
    assert pairs(nb=nbp - 1) == WORKSPACE and pairs(ws=None) == WORKSPACE
    assert pairs(c=8192, lda=8192, ldb=8192, nb=nbp - 1) == WORKSPACE                               # the cap itself passes validation
