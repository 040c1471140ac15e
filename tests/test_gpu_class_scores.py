"""The classifier-output scores on the device against the float64 oracle of tests/class_scores_reference.py.

Bounds (derived in DESIGN.md, "Classifier-output scores"; u = 2^-53):
  h_i       |device - oracle| <= (C + 16) u (sum_c p_c |l_c - M| + |log S| + 1)
  log IS_b  the mean of its rows' bounds + (C + n_b + 16) u (sum_c pbar_c |log pbar_c| + 1)
  paired v  (C + 16) u (sum of the absolute values of its terms + 1); cosine: the terms are a_c b_c / (|a| |b|)
and, exactly: float32 rows and their float64 copies, two calls, a group list in stored order / behind a permutation / with
idx == NULL, groups next to non-finite rows, the four sums against the documented fold of the row values, a set against
itself.  Measured on the MI355X (the ratios the tests print): see profiles/class_scores/accuracy.txt."""
import math
import warnings

import numpy as np
import pytest
import torch

import class_scores_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -53
MEASURED = {}
GROUP_C = [1, 3, 4, 5, 63, 64, 65, 255, 257, 527, 1000, 2047, 2048]
PAIR_C = GROUP_C + [8192]
SIZES = [1, 2, 63, 64, 65, 130, 200]                  # segments that cross, single-row groups, a last partial segment
OFFS = np.concatenate([[0], np.cumsum(SIZES)]).tolist()
N_ROWS = [1, 3, 63, 64, 65, 257]
KINDS = ["randn", "times_1e3", "times_1e-3", "masked_column", "point_masses"]


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    audio_metrics_amd._lib.load()
    return audio_metrics_amd


@pytest.fixture(scope="module")
def ops(am):
    return am.hip_ops


@pytest.fixture(scope="module", autouse=True)
def accuracy_record():
    yield
    for section, lines in MEASURED.items():
        ref.record_accuracy(section, lines)


def logits(seed, n, c, kind="randn"):
    x = (np.random.default_rng(seed).standard_normal((n, c)) * 2).astype(np.float32)
    if kind == "times_1e3":
        x *= np.float32(1e3)
    elif kind == "times_1e-3":
        x *= np.float32(1e-3)
    elif kind == "masked_column":
        x[:, c // 2] = -np.inf
    elif kind == "point_masses":                      # every third row -inf in all but one class
        for i in range(0, n, 3):
            keep = x[i, i % c]
            x[i] = -np.inf
            x[i, i % c] = keep
    return x


def padded(a, extra=8, poison=math.nan):
    """The matrix as a device view of a wider one: a row stride of (columns rounded up to 4) + extra, `poison` in the rest."""
    n, c = a.shape
    buf = torch.full((n, (c + 3) // 4 * 4 + extra), poison, dtype=torch.as_tensor(a).dtype, device=DEV)
    buf[:, :c] = torch.as_tensor(a)
    return buf[:, :c]


def groups_call(ops, x_dev, order, offs):
    rec, h, check = ops.class_group_scores(x_dev, order, offs, return_rows=True)
    check()
    return rec.cpu().numpy(), h.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


def check_groups(rec, h, want, c, sizes, tag):
    """The bounds of h and log IS for every group; returns the two largest ratios."""
    worst_h = worst_is = 0.0
    pos = 0
    for b, n_b in enumerate(sizes):
        hb, wb, scale = h[pos:pos + n_b], want["h"][b], want["row_scale"][b]
        pos += n_b
        bound_h = (c + 16) * U * scale
        err = np.abs(hb - wb)
        assert np.all(err <= bound_h), (tag, b, float(np.max(err / bound_h)))
        worst_h = max(worst_h, float(np.max(err / bound_h)))
        bound_is = float(np.mean(bound_h)) + (c + n_b + 16) * U * want["marginal_scale"][b]
        err_is = abs(rec[b, 2] - want["log_is"][b])
        assert err_is <= bound_is, (tag, b, err_is / bound_is)
        worst_is = max(worst_is, err_is / bound_is)
        # the mean of n_b values h <= 0: their bounds, n_b - 1 additions and a division
        assert abs(rec[b, 0] - want["mean_h"][b]) <= float(np.mean(bound_h)) + (n_b + 16) * U * (abs(want["mean_h"][b]) + 1), (tag, b)
        assert rec[b, 3] == 0.0 and rec[b, 2] == rec[b, 0] - rec[b, 1]
    return worst_h, worst_is


# ---------------------------------------------------------------------------------------------------- class groups
@pytest.mark.parametrize("c", GROUP_C)
def test_class_groups_against_the_oracle_and_exact_identities(ops, c):
    n = OFFS[-1]
    x = logits(c, n, c)
    want = ref.class_groups(x, [range(a, b) for a, b in zip(OFFS, OFFS[1:])])
    x_dev = padded(x)                                                     # ld > C: a column slice of a wider matrix
    rec, h = groups_call(ops, x_dev, None, OFFS)
    worst = check_groups(rec, h, want, c, SIZES, c)
    print("C = %d: h %.4f, log IS %.4f" % (c, *worst))
    MEASURED.setdefault("class groups, randn x 2, group sizes 1 2 63 64 65 130 200: largest |device - oracle| / bound of h_i, of log IS_b (bound: 1)",
                        []).append("C = %d: %.4f, %.4f" % (c, *worst))
    # two calls; idx == NULL against the identity list; a contiguous copy; the float64 copy of the rows
    again = groups_call(ops, x_dev, None, OFFS)
    ident = groups_call(ops, x_dev, torch.arange(n, device=DEV), OFFS)
    plain = groups_call(ops, torch.as_tensor(x).to(DEV), None, OFFS)
    wide = groups_call(ops, padded(x.astype(np.float64), extra=3), None, OFFS)
    for other in (again, ident, plain, wide):
        assert same_bits(rec, other[0]) and same_bits(h, other[1])
    # the same groups behind a seeded permutation of the stored rows
    perm = np.random.default_rng(100 + c).permutation(n)
    stored = np.empty_like(x)
    stored[perm] = x
    moved = groups_call(ops, torch.as_tensor(stored).to(DEV), torch.as_tensor(perm).to(DEV), OFFS)
    assert same_bits(rec, moved[0]) and same_bits(h, moved[1])
    # a group's bits do not depend on the other groups of the call: the last group alone
    alone = groups_call(ops, x_dev, torch.arange(OFFS[-2], n, device=DEV), [0, SIZES[-1]])
    assert same_bits(rec[-1], alone[0][0]) and same_bits(h[OFFS[-2]:], alone[1])


@pytest.mark.parametrize("kind", KINDS[1:])
@pytest.mark.parametrize("c", [5, 257, 527])
def test_class_groups_on_scaled_and_masked_logits(ops, c, kind):
    sizes = [1, 2, 65, 3]
    offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    x = logits(7 * c, offs[-1], c, kind)
    want = ref.class_groups(x, [range(a, b) for a, b in zip(offs, offs[1:])])
    assert want["nonfinite"].sum() == 0
    rec, h = groups_call(ops, torch.as_tensor(x).to(DEV), None, offs)
    worst = check_groups(rec, h, want, c, sizes, (c, kind))
    print("C = %d, %s: h %.4f, log IS %.4f" % (c, kind, *worst))
    MEASURED.setdefault("class groups, scaled and masked logits: largest ratio of h_i, of log IS_b (bound: 1)", []).append(
        "C = %d, %s: %.4f, %.4f" % (c, kind, *worst))
    if kind == "point_masses":
        assert np.all(h[0::3] == 0.0)                                    # one live class: the entropy is exactly 0
    wide = groups_call(ops, torch.as_tensor(x.astype(np.float64)).to(DEV), None, offs)
    assert same_bits(rec, wide[0]) and same_bits(h, wide[1])


@pytest.mark.parametrize("n", N_ROWS)
def test_class_groups_row_counts(ops, n):
    for c in (5, 65):
        x = logits(1000 * n + c, n, c)
        want = ref.class_groups(x, [range(n)])
        rec, h = groups_call(ops, torch.as_tensor(x).to(DEV), None, [0, n])
        check_groups(rec, h, want, c, [n], (n, c))
        if n > 1:                                                        # every row its own group (log IS = 0 up to rounding)
            rec1, h1 = groups_call(ops, torch.as_tensor(x).to(DEV), None, list(range(n + 1)))
            check_groups(rec1, h1, ref.class_groups(x, [[i] for i in range(n)]), c, [1] * n, (n, c, "single rows"))
            assert same_bits(h, h1)


def test_class_groups_non_finite_rows(ops):
    c = 37
    x = logits(11, OFFS[-1], c)
    clean = groups_call(ops, torch.as_tensor(x).to(DEV), None, OFFS)
    bad = x.copy()
    rows = {OFFS[2] + 5: "nan", OFFS[4] + 64: "inf", OFFS[6] + 199: "ninf"}            # groups 2, 4 and 6
    bad[OFFS[2] + 5, 3] = np.nan
    bad[OFFS[4] + 64, c - 1] = np.inf
    bad[OFFS[6] + 199] = -np.inf
    bad[OFFS[6] + 7, 0] = np.nan                                                       # a second one in group 6
    rec, h = groups_call(ops, torch.as_tensor(bad).to(DEV), None, OFFS)
    assert rec[:, 3].tolist() == [0, 0, 1, 0, 1, 0, 2]
    assert np.flatnonzero(np.isnan(h)).tolist() == sorted(list(rows) + [OFFS[6] + 7])
    for b in range(7):
        if rec[b, 3]:
            assert np.isnan(rec[b, :3]).all()
        else:
            assert same_bits(rec[b], clean[0][b])                      # untouched groups keep their bits
    keep = ~np.isnan(h)
    assert same_bits(h[keep], clean[1][keep])
    # an index outside [0, N) is flagged, never dereferenced
    idx = torch.arange(OFFS[-1], device=DEV)
    idx[17] = OFFS[-1] + 5
    out, _, check = ops.class_group_scores(torch.as_tensor(x).to(DEV), idx, OFFS)
    with pytest.raises(ValueError, match=r"idx\[17\]"):
        check()


# ---------------------------------------------------------------------------------------------------- row pairs
def fold_of_rows(v):
    """{sum v, sum v^2, finite, non-finite} in the order the device documents: per 64 rows an xor butterfly over the lanes
    (offsets 32 .. 1); the workgroups' partials thread-strided (w = t, t + 256, ...), the same butterfly per wave of 64
    threads, then (wave 0 + wave 1) + (wave 2 + wave 3)."""
    lanes = np.arange(64)

    def butterfly(q):
        q = q.copy()
        for off in (32, 16, 8, 4, 2, 1):
            q = q + q[..., lanes ^ off]
        return q[..., 0]
    n = len(v)
    nwg = (n + 63) // 64
    full = np.zeros(nwg * 64)
    full[:n] = v
    valid = np.arange(nwg * 64) < n
    fin = valid & np.isfinite(full)
    quantities = [np.where(fin, full, 0.0), np.where(fin, full, 0.0) ** 2, fin.astype(np.float64), (valid & ~fin).astype(np.float64)]
    out = []
    for q in quantities:
        partial = butterfly(q.reshape(nwg, 64))
        threads = np.zeros(256)
        for w in range(nwg):
            threads[w % 256] += partial[w]
        waves = butterfly(threads.reshape(4, 64))
        out.append((waves[0] + waves[1]) + (waves[2] + waves[3]))
    return np.array(out)


def pairs_call(ops, a, b, mode, eps):
    sums, rows = ops.row_pair_scores(a, b, mode, eps, return_rows=True)
    return sums.cpu().numpy(), rows.cpu().numpy()


@pytest.mark.parametrize("c", PAIR_C)
def test_row_pairs_against_the_oracle_and_exact_identities(ops, c):
    n = 67                                                                # two workgroups, the second partial
    cand, other = logits(2 * c, n, c), logits(2 * c + 1, n, c)
    a_dev, b_dev = padded(cand), torch.as_tensor(other).to(DEV)
    a64, b64 = torch.as_tensor(cand.astype(np.float64)).to(DEV), padded(other.astype(np.float64), extra=5)
    lines = []
    for mode in ref.MODES:
        for eps in ((0.0,) if mode == "cosine" else (0.0, 1e-6)):
            want, scale = ref.pair_rows(cand, other, mode, eps)
            sums, rows = pairs_call(ops, a_dev, b_dev, mode, eps)
            bound = (c + 16) * U * scale
            assert np.all(np.abs(rows - want) <= bound), (c, mode, eps, float(np.max(np.abs(rows - want) / bound)))
            lines.append("%s%s %.4f" % (mode, "" if eps == 0 else " eps", float(np.max(np.abs(rows - want) / bound))))
            assert same_bits(sums, fold_of_rows(rows)) and sums[2] == n and sums[3] == 0
            again, wide = pairs_call(ops, a_dev, b_dev, mode, eps), pairs_call(ops, a64, b64, mode, eps)
            assert same_bits(sums, again[0]) and same_bits(rows, again[1]) and same_bits(sums, wide[0]) and same_bits(rows, wide[1])
            only_sums, none = ops.row_pair_scores(a_dev, b_dev, mode, eps)
            assert none is None and same_bits(sums, only_sums.cpu().numpy())
    print("C = %d: %s" % (c, ", ".join(lines)))
    MEASURED.setdefault("row pairs, randn x 2, 67 rows: largest |device - oracle| / bound per mode (bound: 1)", []).append(
        "C = %d: %s" % (c, ", ".join(lines)))


@pytest.mark.parametrize("kind", KINDS[1:])
def test_row_pairs_on_scaled_and_masked_logits(ops, kind):
    lines = []
    for c in (5, 257):
        cand, other = logits(3 * c, 66, c, kind), logits(3 * c + 1, 66, c, kind)
        if kind == "masked_column":
            cand[7, 0] = -np.inf                                          # a masked candidate class under p^r > 0: +inf
        for mode in ref.MODES:
            for eps in ((0.0,) if mode == "cosine" else (0.0, 1e-6)):
                want, scale = ref.pair_rows(cand, other, mode, eps)
                sums, rows = pairs_call(ops, torch.as_tensor(cand).to(DEV), torch.as_tensor(other).to(DEV), mode, eps)
                fin = np.isfinite(want)
                assert np.array_equal(np.isnan(rows), np.isnan(want)) and np.array_equal(rows[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
                bound = (c + 16) * U * scale[fin]
                assert np.all(np.abs(rows[fin] - want[fin]) <= bound), (c, kind, mode, eps, float(np.max(np.abs(rows[fin] - want[fin]) / bound)))
                lines.append("C = %d %s%s %.4f" % (c, mode, "" if eps == 0 else " eps", float(np.max(np.abs(rows[fin] - want[fin]) / bound)) if fin.any() else 0.0))
                assert same_bits(sums, fold_of_rows(rows)) and sums[2] == fin.sum() and sums[3] == 66 - fin.sum()
        if kind == "masked_column":
            assert pairs_call(ops, torch.as_tensor(cand).to(DEV), torch.as_tensor(other).to(DEV), "kl_softmax", 0.0)[1][7] == math.inf
    print(kind, "; ".join(lines))
    MEASURED.setdefault("row pairs, scaled and masked logits, 66 rows: largest ratio (bound: 1)", []).append("%s: %s" % (kind, "; ".join(lines)))


@pytest.mark.parametrize("n", N_ROWS + [16_500])
def test_row_pairs_row_counts_and_the_fold(ops, n):
    c = 5 if n > 1000 else 65                                             # 16 500 rows: 258 workgroups, past one stride of the fold
    cand, other = logits(n, n, c), logits(n + 1, n, c)
    if n > 70:
        cand[70, 1], other[3, 2] = np.nan, np.inf
    for mode in ("cosine", "kl_softmax"):
        sums, rows = pairs_call(ops, torch.as_tensor(cand).to(DEV), torch.as_tensor(other).to(DEV), mode, 0.0)
        assert same_bits(sums, fold_of_rows(rows)), (n, mode)
        if n <= 1000:
            want, scale = ref.pair_rows(cand, other, mode)
            fin = np.isfinite(want)
            assert np.array_equal(np.isfinite(rows), fin) and np.all(np.abs(rows[fin] - want[fin]) <= (c + 16) * U * scale[fin])
            assert sums[3] == n - fin.sum() == (2 if n > 70 else 0)


def test_non_finite_pairs_are_counted_and_left_out(am):
    c = 12
    cand, other = logits(1, 40, c), logits(2, 40, c)
    cand[3, 1], other[4, 0], other[25], cand[30] = np.nan, np.inf, -np.inf, 0.0
    a, b = torch.as_tensor(cand).to(DEV), torch.as_tensor(other).to(DEV)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        kl = am.kl_divergence_paired(a, b, return_rows=True)
        cos = am.paired_cosine_score(a, b, return_rows=True)
    assert len(caught) == 2 and all(issubclass(w.category, RuntimeWarning) for w in caught)
    assert np.flatnonzero(np.isnan(kl["kl_rows"])).tolist() == [3, 4, 25] and (kl["kl_rows_used"], kl["kl_rows_nonfinite"]) == (37, 3)
    assert np.flatnonzero(np.isnan(cos["cosine_rows"])).tolist() == [3, 4, 25, 30] and cos["cosine_rows_nonfinite"] == 4     # a zero norm
    want = ref.paired_summary(ref.pair_rows(cand, other, "kl_softmax")[0])
    assert kl["kl"] == pytest.approx(want[0], rel=1e-13) and kl["kl_std_error"] == pytest.approx(want[1], rel=1e-9)


# ---------------------------------------------------------------------------------------------------- a set against itself
def test_a_set_against_itself(am):
    for kind in ("randn", "times_1e3"):
        x = torch.as_tensor(logits(5, 130, 527, kind)).to(DEV)
        for same in (x, x.clone()):
            zero = am.kl_divergence_paired(x, same, return_rows=True)
            assert zero["kl"] == 0.0 and np.all(zero["kl_rows"] == 0.0) and zero["kl_std_error"] == 0.0
            below = am.kl_divergence_paired(x, same, eps=1e-6, return_rows=True)
            assert below["kl"] <= 0.0 and np.all(below["kl_rows"] <= 0.0)
            for mode in ("sigmoid", "bernoulli"):
                assert np.all(am.kl_divergence_paired(x, same, mode=mode, return_rows=True)["kl_rows"] == 0.0)
            one = am.paired_cosine_score(x, same, return_rows=True)
            assert abs(one["cosine_score"] - 1.0) <= 2.0 ** -52 and np.all(np.abs(one["cosine_rows"] - 1.0) <= 2.0 ** -52)
        minus = am.paired_cosine_score(x, -x, return_rows=True)
        assert np.all(np.abs(minus["cosine_rows"] + 1.0) <= 2.0 ** -52)


# ---------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("seed", [None, 3])
def test_inception_score_end_to_end(am, seed):
    n, c, splits = 263, 10, 4
    x = logits(9, n, c)
    x[:, :3] += 2.0
    want = ref.inception(x, splits, seed)
    data = am.AudioMetricsData(True)
    data.add(torch.as_tensor(x).to(DEV))
    got = am.inception_score(data, splits=splits, seed=seed, return_rows=True)
    g = want["groups"]
    for k in range(splits):
        n_k = len(g["h"][k])
        bound = float(np.mean((c + 16) * U * g["row_scale"][k])) + (c + n_k + 16) * U * g["marginal_scale"][k]
        # IS = exp(log IS): the bound of the logarithm, relative, plus the rounding of exp
        assert abs(got["inception_score_per_split"][k] - want["inception_score_per_split"][k]) <= (math.expm1(bound) + 2 * U) * want["inception_score_per_split"][k]
    scale = np.empty(n)
    for rows_k, scale_k in zip(ref.split_plan(n, splits, seed), g["row_scale"]):
        scale[rows_k] = scale_k
    assert np.all(np.abs(got["row_entropy"] - want["row_entropy"]) <= (c + 16) * U * scale)
    for key in ("inception_score", "inception_score_std", "inception_conditional_entropy", "inception_marginal_entropy"):
        assert got[key] == pytest.approx(want[key], rel=1e-12, abs=1e-13), key
    assert got["inception_n_splits"] == splits and got["inception_score"] > 1.0
    tensor = am.inception_score(torch.as_tensor(x).to(DEV).double(), splits=splits, seed=seed, return_rows=True)
    assert same_bits(tensor["inception_score_per_split"], got["inception_score_per_split"]) and same_bits(tensor["row_entropy"], got["row_entropy"])


def test_inception_score_per_group_equals_the_splits(am):
    n, c, splits = 263, 10, 4
    x = torch.as_tensor(logits(9, n, c)).to(DEV)
    offs = [k * n // splits for k in range(splits + 1)]
    labels = np.repeat(np.arange(splits) * 7 - 3, np.diff(offs))
    whole = am.inception_score(x, splits=splits)
    per = am.inception_score_per_group(x, labels)
    assert same_bits(per["inception_score_per_group"], whole["inception_score_per_split"])
    assert per["group_labels"].tolist() == [-3, 4, 11, 18] and per["group_sizes"].tolist() == np.diff(offs).tolist()
    # the rows stored in another order, listed behind the permutation that restores it: the same bits
    perm = np.random.default_rng(0).permutation(n)
    from audio_metrics_amd import hip_ops
    stored = x[torch.as_tensor(perm).to(DEV)]                            # stored[j] = x[perm[j]]: x[i] lies at argsort(perm)[i]
    rec, _, check = hip_ops.class_group_scores(stored, torch.as_tensor(np.argsort(perm)).to(DEV), offs)
    check()
    assert same_bits(np.exp(rec.cpu().numpy()[:, 2]), whole["inception_score_per_split"])
