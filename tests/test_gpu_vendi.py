"""The Vendi score on the device (am_vendi_groups_* / am_vendi_gram_* / am_vendi_moment_*, vendi_score and
vendi_score_per_group) against the numpy float64 oracles of vendi_reference.py.

Group route.  Criterion: eigenvalues within 1e-12 lambda_max of eigvalsh(K / n), the order-1 score within 1e-12 relative,
equal rank, stop code 1, at most 30 sweeps, residual <= 2^-52.  Basis of 1e-12 (tests/test_vendi_cpu.py::test_oracles_agree,
on the CPU): two independent oracles - LAPACK eigvalsh of K / n and the SVD of the normalised rows - differ by at most 3.6e-15
on these inputs at orders 1, 2 and inf (that test measures 3.6e-15 at order 1 and 9.3e-15 at order 0.5; with a second LAPACK
driver in the comparison the spread at order 0.5, where the smallest kept eigenvalues weigh most, reaches 1.1e-12); 1e-12
is the bar per-group FAD holds the same Jacobi to.  Order 0.5 is therefore held to 1e-9 (1000 x the oracles' own spread), order
2 to 1e-12.  Every case rests on the oracle's own condition (vendi_reference.apply_zero_rule): no eigenvalue within a factor
1e3 of the zero threshold.  A family of three tight clusters (spread 0.01) does not meet it under the Gaussian kernel at D = 20,
n >= 127, and is left out.

Whole-set routes.  Eigenvalues within 1e-10 lambda_0 - am_eigh_sym_f64's pinned accuracy (tests/test_gpu_pca.py: E1) - and
|ln VS - ln VS_oracle| <= sum_i 1e-10 lambda_0 (|ln lambda_i| + 1) over the oracle's kept eigenvalues, computed per case from
the oracle alone.

Measured on an MI355X (maxima over the cases of each test, printed by the tests):
  group route       eigenvalues 4.1e-15 lambda_max, order 1 5.8e-15 relative, 9 - 15 sweeps, residual <= 2.1e-16
  Python layer      order 0.5: 8.0e-15, order 1: 3.6e-15, order 2: 5.8e-15 relative
  closed forms      identical rows: 8.9e-16; orthogonal rows: 3.8e-15 relative
  gram route        eigenvalues 5.1e-14 lambda_0, |ln VS - ln oracle| 1.3e-13 (bounds 5.8e-10 .. 4.7e-8)
  moment route      eigenvalues 2.2e-14 lambda_0, |ln VS - ln oracle| 4.7e-14
  median bandwidth  equal bits against the bandwidth it reports; |ln VS - ln oracle| 1.2e-14 (bound 6.3e-8)
  one group of 100  |ln VS(gram) - ln VS(groups)| 8.9e-16 (cosine), 4.9e-15 (Gaussian)"""
import warnings

import numpy as np
import pytest
import torch

import vendi_reference as vr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-12
SIZES = [1, 2, 3, 15, 16, 17, 33, 64, 127, 128]
BW = 0.7                                  # the fixed Gaussian bandwidth, on unit-norm rows
EIGH_TOL = 1e-10                          # whole-set routes: the eigensolver's pinned accuracy and their zero_tol
WHOLE = [(64, 132, "randn"), (129, 20, "randn"), (300, 64, "randn"), (513, 20, "randn"), (700, 64, "song")]
_CACHE = {}


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    audio_metrics_amd._lib.load()
    return audio_metrics_amd


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64).tolist()


def grouped_case(kind, d, dtype, kernel):
    """The ten groups of SIZES as one stored matrix with the groups scattered behind a permutation, and the oracle of every
    group; computed once per case.  Gaussian cases use unit-norm rows.  The oracle sees the values the device sees (the
    float32 rows as float64)."""
    key = (kind, d, np.dtype(dtype).name, kernel)
    if key not in _CACHE:
        rng = np.random.default_rng(100 * d + len(kind))
        groups = []
        for n in SIZES:
            x = vr.family_rows(kind, n, d, rng)
            if kernel == "gaussian":
                x = x / np.linalg.norm(x, axis=1, keepdims=True)
            groups.append(x.astype(dtype))
        offs = offsets_of(SIZES)
        listed = np.concatenate(groups)
        perm = np.random.default_rng(d).permutation(offs[-1])
        stored = np.empty_like(listed)
        stored[perm] = listed                                              # list position p is stored row perm[p]
        labels = np.empty(offs[-1], dtype=np.int64)
        labels[perm] = np.repeat(np.arange(len(SIZES)), SIZES)
        want = [vr.oracle(g.astype(np.float64), kernel, BW, orders=(0.5, 1.0, 2.0)) for g in groups]
        _CACHE[key] = (stored, perm, offs, labels, want)
    return _CACHE[key]


def width(kernel):
    return {"gamma": 1.0 / (2.0 * BW * BW)} if kernel == "gaussian" else {}


def run_groups(am, rows, idx, offs, kernel, **kw):
    rec, evals, check = am.hip_ops.vendi_groups(rows, idx, offs, kernel, **(kw or width(kernel)))
    rec, evals = rec.cpu().numpy(), evals.cpu().numpy()
    check()
    return rec, evals


# ------------------------------------------------------------------ 1. every group size, both row types, three families, both kernels
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["randn", "song", "dups"])
@pytest.mark.parametrize("d", [20, 64, 132])
def test_group_sizes(am, d, kind, dtype):
    for kernel in ("cosine", "gaussian"):
        stored, perm, offs, _, want = grouped_case(kind, d, dtype, kernel)
        rec, evals = run_groups(am, torch.as_tensor(stored).to(DEV), torch.as_tensor(perm).to(DEV), offs, kernel)
        err_l = max(np.abs(evals[offs[g]:offs[g + 1]] - w["lam"]).max() / w["lam"][0] for g, w in enumerate(want))
        err_v = max(abs(rec[g, 0] / w["scores"][1.0] - 1.0) for g, w in enumerate(want))
        err_h = max(abs(rec[g, 1] - w["entropy"]) for g, w in enumerate(want))
        print(kernel, "eigenvalues / lambda_max:", err_l, " vendi rel:", err_v, " entropy abs:", err_h, " sweeps:", rec[:, 4].max(),
              " residual:", rec[:, 5].max())
        assert (rec[:, 6] == 1).all(), rec[:, 6]
        assert (rec[:, 4] <= 30).all() and (rec[:, 5] <= 2.0 ** -52).all(), rec[:, 4:6]
        assert rec[0].tolist() == [1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0]          # one row: vendi 1, entropy 0, rank 1, no sweeps
        assert (rec[:, 2] == [w["rank"] for w in want]).all(), (rec[:, 2], [w["rank"] for w in want])
        assert (rec[:, 3] == [evals[o] for o in offs[:-1]]).all() and (rec[:, 7] == 0).all()
        for g in range(len(SIZES)):
            lam = evals[offs[g]:offs[g + 1]]
            assert (np.diff(lam) <= 0).all() and (lam[int(rec[g, 2]):] == 0.0).all()  # descending, the dropped ones exactly 0
        assert err_l <= TOL and err_v <= TOL, (kernel, err_l, err_v)


@pytest.mark.parametrize("kernel", ["cosine", "gaussian"])
@pytest.mark.parametrize("kind", ["randn", "song", "dups"])
def test_orders_through_the_python_layer(am, kind, kernel):
    worst = {0.5: 0.0, 1.0: 0.0, 2.0: 0.0}
    for d in (20, 132):
        stored, _, _, labels, want = grouped_case(kind, d, np.float64, kernel)
        out = am.vendi_score_per_group(torch.as_tensor(stored).to(DEV), labels, kernel=kernel, orders=(0.5, 1.0, 2.0),
                                       bandwidth=BW if kernel == "gaussian" else None)
        assert out["vendi_per_group"].shape == (3, len(SIZES)) and out["group_sizes"].tolist() == SIZES
        assert out["vendi_rank_per_group"].tolist() == [w["rank"] for w in want]
        assert out["vendi_bandwidth"] == (BW if kernel == "gaussian" else None) and out["vendi_orders"] == (0.5, 1.0, 2.0)
        for i, q in enumerate((0.5, 1.0, 2.0)):
            worst[q] = max(worst[q], max(abs(out["vendi_per_group"][i, g] / w["scores"][q] - 1.0) for g, w in enumerate(want)))
    print(kind, kernel, "relative error per order:", worst)
    assert worst[0.5] <= 1e-9 and worst[1.0] <= TOL and worst[2.0] <= TOL, worst


# ------------------------------------------------------------------ 2. bit-level properties
@pytest.mark.parametrize("kernel", ["cosine", "gaussian"])
def test_bit_level_properties(am, kernel):
    d, sizes = 64, [50, 7, 128, 33, 64, 1, 20, 100, 16, 65]
    rng = np.random.default_rng(5)
    offs = offsets_of(sizes)
    listed = (rng.standard_normal((offs[-1], d)) * 0.1).astype(np.float32)
    perm = rng.permutation(offs[-1])
    stored = np.empty_like(listed)
    stored[perm] = listed
    x32, idx = torch.as_tensor(stored).to(DEV), torch.as_tensor(perm).to(DEV)
    rec, evals = run_groups(am, x32, idx, offs, kernel)
    assert (rec[:, 6] == 1).all()
    again = run_groups(am, x32, idx, offs, kernel)                       # two calls
    assert rec.tobytes() == again[0].tobytes() and evals.tobytes() == again[1].tobytes()
    wide = run_groups(am, x32.to(torch.float64), idx, offs, kernel)      # float32 rows and their float64 conversion
    assert rec.tobytes() == wide[0].tobytes() and evals.tobytes() == wide[1].tobytes()
    in_order = run_groups(am, torch.as_tensor(listed).to(DEV), None, offs, kernel)       # stored order, no index list
    assert rec.tobytes() == in_order[0].tobytes() and evals.tobytes() == in_order[1].tobytes()
    for g in (0, 2, 5):                                                  # alone: B = 1, in stored order and behind idx
        rows = torch.as_tensor(listed[offs[g]:offs[g + 1]].copy()).to(DEV)
        alone = run_groups(am, rows, None, [0, sizes[g]], kernel)
        behind = run_groups(am, x32, idx[offs[g]:offs[g + 1]].clone(), [0, sizes[g]], kernel)
        for r, e in (alone, behind):
            assert r[0].tobytes() == rec[g].tobytes() and e.tobytes() == evals[offs[g]:offs[g + 1]].tobytes(), g
    # an index outside [0, N): check() raises, the row is never read, and the other groups' records keep their bits
    bad = idx.clone()
    bad[offs[3] + 4] = offs[-1] + 5
    r_bad, e_bad, check = am.hip_ops.vendi_groups(x32, bad, offs, kernel, **width(kernel))
    r_bad, e_bad = r_bad.cpu().numpy(), e_bad.cpu().numpy()
    with pytest.raises(ValueError, match=r"idx\[%d\] = %d is outside" % (offs[3] + 4, offs[-1] + 5)):
        check()
    keep = np.arange(len(sizes)) != 3
    assert r_bad[keep].tobytes() == rec[keep].tobytes()
    assert e_bad[:offs[3]].tobytes() == evals[:offs[3]].tobytes() and e_bad[offs[4]:].tobytes() == evals[offs[4]:].tobytes()
    # the device-scalar bandwidth: gamma = 0.5 / (double)bw2, the bits of the host number formed the same way
    if kernel == "gaussian":
        bw2 = torch.tensor(0.37, dtype=torch.float32, device=DEV)
        from_dev = run_groups(am, x32, idx, offs, kernel, gamma_dev=bw2)
        from_host = run_groups(am, x32, idx, offs, kernel, gamma=0.5 / float(np.float32(0.37)))
        assert from_dev[0].tobytes() == from_host[0].tobytes() and from_dev[1].tobytes() == from_host[1].tobytes()


# ------------------------------------------------------------------ 3. closed forms
def test_closed_forms(am):
    rng = np.random.default_rng(11)
    d = 48
    one = rng.standard_normal(d)
    ortho = np.linalg.qr(rng.standard_normal((d, d)))[0]
    sizes = [40, 20, 48, 1]
    rows = np.concatenate([np.tile(one, (40, 1)), ortho[:20] * 3.0, ortho * rng.uniform(0.5, 2.0, (d, 1)), one[None, :]])
    offs = offsets_of(sizes)
    for dtype in (torch.float64, torch.float32):
        x = torch.as_tensor(rows).to(DEV, dtype)
        rec, _ = run_groups(am, x, None, offs, "cosine")
        print(dtype, "identical:", rec[0, 0] - 1.0, " orthonormal:", rec[1, 0] / 20 - 1.0, rec[2, 0] / 48 - 1.0)
        assert abs(rec[0, 0] - 1.0) <= TOL and rec[0, 2] == 1                  # n identical rows: one effective sample
        if dtype == torch.float64:                                             # (rounding the rows to float32 breaks orthogonality)
            assert abs(rec[1, 0] / 20 - 1.0) <= TOL and rec[1, 2] == 20        # n <= D orthogonal rows of any length: n
            assert abs(rec[2, 0] / 48 - 1.0) <= TOL and rec[2, 2] == 48
        assert (rec[:, 6] == 1).all()
        rec, _ = run_groups(am, x, None, offs, "gaussian")
        assert abs(rec[0, 0] - 1.0) <= TOL and rec[0, 2] == 1
        assert rec[3].tolist() == [1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_rows_without_a_similarity_give_nan_for_their_group_alone(am, dtype):
    rng = np.random.default_rng(12)
    sizes = [10, 30, 1, 70, 5]
    offs = offsets_of(sizes)
    rows = rng.standard_normal((offs[-1], 24))
    rows[offs[1] + 3] = 0.0                                               # a zero row in group 1
    rows[offs[3] + 60, 7] = np.nan                                        # a NaN element in group 3
    x = torch.as_tensor(rows).to(DEV, dtype)
    labels = np.repeat(np.arange(len(sizes)), sizes)
    clean = am.vendi_score_per_group(x[:offs[1]], labels[:offs[1]])["vendi_per_group"]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = am.vendi_score_per_group(x, labels, orders=(1.0, 0.5))
    assert len([w for w in caught if issubclass(w.category, RuntimeWarning)]) == 1, [str(w.message) for w in caught]
    from audio_metrics_amd.metrics.vendi import last_info
    assert last_info["stops"] == [1, 4, 1, 4, 1]
    v = out["vendi_per_group"]
    assert np.isnan(v[:, [1, 3]]).all() and np.isfinite(v[:, [0, 2, 4]]).all() and out["vendi_rank_per_group"].tolist()[2] == 1
    assert v[0, 0] == clean[0]                                            # the neighbour's bits do not move
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        gauss = am.vendi_score_per_group(x, labels, kernel="gaussian", bandwidth=3.0)["vendi_per_group"]
    assert len([w for w in caught if issubclass(w.category, RuntimeWarning)]) == 1 and np.isnan(gauss[3]) and np.isfinite(gauss[[0, 1, 2, 4]]).all()      # a zero row is a row like any other there
    for route in ("groups", "gram", "moment"):                            # the whole-set routes flag the row, too
        with pytest.warns(RuntimeWarning, match="zero norm"):
            res = am.vendi_score(x[offs[1]:offs[2]], route=route, return_eigenvalues=True)
        assert np.isnan(res["vendi"]) and res["vendi_rank"] == 0 and np.isnan(res["vendi_eigenvalues"]).all(), route


# ------------------------------------------------------------------ 4. the whole set: gram and moment routes
def whole_case(n, d, kind):
    if ("whole", n, d) not in _CACHE:
        x = vr.family_rows(kind, n, d, np.random.default_rng(n + d))
        want = vr.oracle(x, "cosine", zero_tol=EIGH_TOL)
        dual = vr.apply_zero_rule(vr.svd_eigenvalues(x), EIGH_TOL)
        assert want["rank"] == dual.size == min(n, d) and np.abs(want["kept"] - dual).max() <= 1e-14 * dual[0]
        _CACHE["whole", n, d] = (x, want)
    return _CACHE["whole", n, d]


def test_moment_route_folds_several_chunks(am):
    chunks = {(n, d): am.hip_ops.vendi_moment_chunks(n, d) for n, d, _ in WHOLE}
    print(chunks)
    assert max(chunks.values()) >= 3, chunks


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n,d,kind", WHOLE)
def test_whole_set_routes(am, n, d, kind, dtype):
    x64, want = whole_case(n, d, kind)
    if dtype == torch.float32:                                            # the oracle of the values the device sees
        x64 = x64.astype(np.float32).astype(np.float64)
        want = vr.oracle(x64, "cosine", zero_tol=EIGH_TOL)
    x = torch.as_tensor(x64).to(DEV, dtype)
    bound = vr.log_score_bound(want["kept"], EIGH_TOL)
    routes = (["groups"] if n <= 128 else []) + ["gram", "moment"]
    assert am.vendi_score(x)["vendi_route"] == ("groups" if n <= 128 else "moment" if n > d else "gram")
    for route in routes:
        got = am.vendi_score(x, route=route, orders=(1.0, 2.0, float("inf")), return_eigenvalues=True)
        lam = got["vendi_eigenvalues"]
        m = min(len(lam), n)
        err_l = np.abs(lam[:m] - want["lam"][:m]).max() / want["lam"][0]
        err_v = abs(np.log(got["vendi"]) - np.log(want["scores"][1.0]))
        print(route, "eigenvalues / lambda_0:", err_l, " |ln VS - ln oracle|:", err_v, " bound:", bound, " rank:", got["vendi_rank"])
        assert got["vendi_route"] == route and got["vendi_kernel"] == "cosine" and got["vendi_bandwidth"] is None
        assert err_l <= (TOL if route == "groups" else EIGH_TOL), (route, err_l)
        assert err_v <= bound, (route, err_v, bound)
        assert got["vendi_rank"] == want["rank"] == min(n, d)
        assert got["vendi_per_order"][0] == got["vendi"]
        assert abs(got["vendi_per_order"][2] * lam[0] - 1.0) <= 1e-15
    # the Gram matrix itself: exactly symmetric, diagonal exactly 1 / n, the oracle's K / n
    mat, check = am.hip_ops.vendi_gram(x)
    mat = mat.cpu().numpy()
    assert check() is None
    assert (mat == mat.T).all() and (np.diag(mat) == 1.0 / n).all()
    # (worst case of a d-term dot product in either arithmetic: d 2^-52 of the norms' product, twice, and the normalisation)
    assert np.abs(mat - vr.kernel_matrix(x64, "cosine") / n).max() <= 4 * d * 2.0 ** -52 / n
    sel = torch.arange(n - 1, -1, -3, device=DEV)                         # behind an index list: the same elements
    sub, check = am.hip_ops.vendi_gram(x, sel)
    assert check() is None
    np.testing.assert_allclose(sub.cpu().numpy() * len(sel), mat[np.ix_(sel.cpu().numpy(), sel.cpu().numpy())] * n, rtol=0, atol=4e-16)
    # the moment matrix: exactly symmetric, trace 1, the oracle's S
    s, check = am.hip_ops.vendi_moment(x)
    s = s.cpu().numpy()
    xh = x64 / np.linalg.norm(x64, axis=1, keepdims=True)
    assert check() is None and (s == s.T).all() and abs(np.trace(s) - 1.0) <= 1e-13
    assert np.abs(s - xh.T @ xh / n).max() <= 4 * n * 2.0 ** -52 / d          # n-term sums of products whose mean size is <= 1 / d


def test_gaussian_median_bandwidth_and_the_shared_cache(am, monkeypatch):
    """bandwidth=None is the median pairwise distance of x's own rows through the cache a KAD reference fills: computed
    once, and the score equals the one at the bandwidth it reports.  The two calls form gamma as 0.5 / bw2 and as
    1 / (2 sqrt(bw2)^2), a few 2^-52 apart; gamma d2 stays below 40 where K matters, so K moves by < 1e-14 relative and the
    score with it: 1e-12 is the bar."""
    n, d = 129, 20
    x64 = vr.family_rows("randn", n, d, np.random.default_rng(77))
    data = am.AudioMetricsData(True)
    data._embeddings = torch.as_tensor(x64.astype(np.float32)).to(DEV)
    calls = []
    select = am.hip_ops.pairwise_select_sq
    monkeypatch.setattr(am.hip_ops, "pairwise_select_sq", lambda *a, **k: calls.append(1) or select(*a, **k))
    first = am.vendi_score(data, kernel="gaussian", orders=(1.0, 2.0))
    second = am.vendi_score(data, kernel="gaussian", orders=(1.0, 2.0))
    per_group = am.vendi_score_per_group(data, np.arange(n) % 3, kernel="gaussian")
    assert len(calls) == 1 and first["vendi_route"] == "gram"
    assert first["vendi"] == second["vendi"] and first["vendi_bandwidth"] == second["vendi_bandwidth"] == per_group["vendi_bandwidth"]
    from audio_metrics_amd.metrics.kad import reference_cache
    assert reference_cache(data).bw2_host == pytest.approx(first["vendi_bandwidth"] ** 2, rel=1e-15)
    d2 = np.sort(((x64.astype(np.float32).astype(np.float64)[:, None] - x64.astype(np.float32).astype(np.float64)[None]) ** 2).sum(-1)[np.triu_indices(n, 1)])
    assert first["vendi_bandwidth"] ** 2 == pytest.approx(d2[(len(d2) - 1) // 2], rel=1e-6)       # a float32 rounding of the f64 median
    fixed = am.vendi_score(data, kernel="gaussian", orders=(1.0, 2.0), bandwidth=first["vendi_bandwidth"])
    rel = np.abs(fixed["vendi_per_order"] / first["vendi_per_order"] - 1.0).max()
    want = vr.oracle(x64.astype(np.float32).astype(np.float64), "gaussian", first["vendi_bandwidth"], zero_tol=EIGH_TOL)
    err = abs(np.log(first["vendi"]) - np.log(want["scores"][1.0]))
    print("median bandwidth against the same number:", rel, " |ln VS - ln oracle|:", err, " bound:", vr.log_score_bound(want["kept"], EIGH_TOL))
    assert rel <= TOL and fixed["vendi_rank"] == first["vendi_rank"] == want["rank"]
    assert err <= vr.log_score_bound(want["kept"], EIGH_TOL)
    # a plain tensor has no cache to fill, and gives the same bits
    plain = am.vendi_score(data._embeddings, kernel="gaussian", orders=(1.0, 2.0))
    assert len(calls) == 2 and plain["vendi"] == first["vendi"] and plain["vendi_bandwidth"] == first["vendi_bandwidth"]


# ------------------------------------------------------------------ 5. one group of 100 rows = the set of those rows
@pytest.mark.parametrize("kernel", ["cosine", "gaussian"])
def test_one_group_equals_the_whole_set(am, kernel):
    x64 = vr.family_rows("song", 100, 64, np.random.default_rng(3))
    if kernel == "gaussian":
        x64 /= np.linalg.norm(x64, axis=1, keepdims=True)
    x = torch.as_tensor(x64).to(DEV)
    bw = BW if kernel == "gaussian" else None
    orders = (1.0, 0.5, 2.0, float("inf"))
    per_group = am.vendi_score_per_group(x, np.full(100, 42), kernel=kernel, orders=orders, bandwidth=bw)
    whole = am.vendi_score(x, kernel=kernel, orders=orders, bandwidth=bw)
    assert whole["vendi_route"] == "groups" and per_group["group_labels"].tolist() == [42]
    assert per_group["vendi_per_group"][:, 0].tobytes() == whole["vendi_per_order"].tobytes()          # bit for bit
    assert per_group["vendi_rank_per_group"][0] == whole["vendi_rank"]
    want = vr.oracle(x64, kernel, bw, zero_tol=EIGH_TOL)
    gram = am.vendi_score(x, kernel=kernel, bandwidth=bw, route="gram")
    err = abs(np.log(gram["vendi"]) - np.log(whole["vendi"]))
    print(kernel, "|ln VS(gram) - ln VS(groups)|:", err, " bound:", vr.log_score_bound(want["kept"], EIGH_TOL))
    assert err <= vr.log_score_bound(want["kept"], EIGH_TOL) and gram["vendi_rank"] == whole["vendi_rank"]
