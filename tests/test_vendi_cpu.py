"""The Vendi score, the part that needs no GPU: vendi_from_eigenvalues (host arithmetic), the argument checks of
vendi_score / vendi_score_per_group / hip_ops.vendi_* in front of any device call, the host-side queries and error paths
of the am_vendi_* entry points, and the oracles of vendi_reference.py against each other."""
import ctypes
import math

import numpy as np
import pytest
import torch

import vendi_reference as vr

FAKE = ctypes.c_void_p(0x10000)                       # 16-byte aligned, never dereferenced: the calls stop at validation
BAD_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -4


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


# ------------------------------------------------------------------ vendi_from_eigenvalues
def test_equal_eigenvalues_give_their_number(am):
    for n in (1, 2, 7, 128):
        got = am.vendi_from_eigenvalues(np.full(n, 1.0 / n), orders=(0.5, 1.0, 2.0, float("inf")))
        np.testing.assert_allclose(got, n, rtol=1e-13)
    assert am.vendi_from_eigenvalues([1.0], (1.0,))[0] == 1.0
    assert am.vendi_from_eigenvalues([1.0, 0.0, 0.0], (0.1, 1.0, 3.0, float("inf"))).tolist() == [1.0, 1.0, 1.0, 1.0]


def test_orders_bracket_order_one_and_infinity_is_the_top_eigenvalue(am):
    lam = np.array([0.5, 0.25, 0.125, 0.0625, 0.0625])
    below, one, above, two, inf = am.vendi_from_eigenvalues(lam, (0.999, 1.0, 1.001, 2.0, float("inf")))
    assert below > one > above > two > inf                          # the score falls with the order
    assert below - one < 1e-2 and one - above < 1e-2
    assert inf == 1.0 / 0.5
    assert one == pytest.approx(math.exp(-np.sum(lam * np.log(lam))), rel=1e-15)
    assert two == pytest.approx(1.0 / np.sum(lam ** 2), rel=1e-15)
    # the order of the input does not matter: sums run in descending order
    assert am.vendi_from_eigenvalues(lam[::-1], (0.5, 1.0)).tolist() == am.vendi_from_eigenvalues(lam, (0.5, 1.0)).tolist()


def test_zero_rule_drops_at_the_threshold_and_keeps_just_above(am):
    tol = 1e-10
    at, above = tol * 0.5, tol * 0.5 * (1 + 1e-6)
    base = am.vendi_from_eigenvalues([0.5, 0.5], (0.1, 1.0), tol)
    np.testing.assert_array_equal(am.vendi_from_eigenvalues([0.5, 0.5, at, at / 7, -1e-17], (0.1, 1.0), tol), base)
    kept = am.vendi_from_eigenvalues([0.5, 0.5, above], (0.1, 1.0), tol)
    assert kept[0] > base[0] + 0.1                                  # (5e-11)^0.1 = 0.09 in the sum: why q < 1 needs the rule
    assert kept[1] > base[1] and kept[1] - base[1] < 1e-8
    assert np.isnan(am.vendi_from_eigenvalues([0.5, float("nan")], (1.0,))).all()
    for bad in ((), (0.0,), (-1.0,), (1.0, float("nan"))):
        with pytest.raises(ValueError, match="orders"):
            am.vendi_from_eigenvalues([1.0], bad)


# ------------------------------------------------------------------ argument checks in front of any device call
def test_validation_happens_before_any_device_call(am, monkeypatch):
    from audio_metrics_amd import hip_ops

    def forbidden(*a, **k):
        raise AssertionError("device call before validation")
    for name in ("as_matrix", "as_matrix64", "_call", "_workspace"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    ok = host_set(am, torch.zeros((10, 8)))
    for x in (ok, torch.zeros((10, 8)), torch.zeros((10, 8), dtype=torch.float64)):
        with pytest.raises(ValueError, match="kernel='linear'"):
            am.vendi_score(x, kernel="linear")
        with pytest.raises(ValueError, match="kernel='linear'"):
            am.vendi_score_per_group(x, np.zeros(10, dtype=np.int64), kernel="linear")
        for bad in ((0.0,), (1.0, -2.0), (), (float("nan"),)):
            with pytest.raises(ValueError, match="orders"):
                am.vendi_score(x, orders=bad)
            with pytest.raises(ValueError, match="orders"):
                am.vendi_score_per_group(x, np.zeros(10, dtype=np.int64), orders=bad)
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError, match="bandwidth"):
                am.vendi_score(x, kernel="gaussian", bandwidth=bad)
            with pytest.raises(ValueError, match="bandwidth"):
                am.vendi_score_per_group(x, np.zeros(10, dtype=np.int64), kernel="gaussian", bandwidth=bad)
        with pytest.raises(ValueError, match="route='nystroem'"):
            am.vendi_score(x, route="nystroem")
        with pytest.raises(ValueError, match="9 labels for 10"):
            am.vendi_score_per_group(x, np.zeros(9, dtype=np.int64))
        with pytest.raises(ValueError, match="integer labels"):
            am.vendi_score_per_group(x, np.zeros(10))
    for empty in (am.AudioMetricsData(False), host_set(am, torch.zeros((0, 8))), torch.zeros((0, 8))):
        with pytest.raises(ValueError, match="empty or keeps none"):
            am.vendi_score(empty)
        with pytest.raises(ValueError, match="keeps none"):
            am.vendi_score_per_group(empty, np.zeros(0, dtype=np.int64))
    # a group of 129 rows is named by its label; 128 rows pass this check (and then need the device)
    labels = np.concatenate([np.full(129, 7), np.full(3, -4)])
    with pytest.raises(ValueError, match=r"group 7 holds 129 rows.*at most 128"):
        am.vendi_score_per_group(torch.zeros((132, 8)), labels)
    with pytest.raises(AssertionError, match="device call before validation"):
        am.vendi_score_per_group(torch.zeros((131, 8)), labels[1:])
    # the Gaussian kernel has no route beyond the Gram cap, and says which cap
    with pytest.raises(ValueError, match=r"gaussian kernel on 2049 rows.*2048"):
        am.vendi_score(torch.zeros((2049, 8)), kernel="gaussian", bandwidth=1.0)
    with pytest.raises(ValueError, match="2048"):
        am.vendi_score(torch.zeros((2049, 4000)), route="gram")
    with pytest.raises(ValueError, match="at most 128"):
        am.vendi_score(torch.zeros((129, 8)), route="groups")
    with pytest.raises(ValueError, match="dual form"):
        am.vendi_score(torch.zeros((300, 8)), kernel="gaussian", bandwidth=1.0, route="moment")
    with pytest.raises(ValueError, match="at least 2 rows"):
        am.vendi_score(torch.zeros((1, 8)), kernel="gaussian")
    # hip_ops.vendi_*
    rows = torch.zeros((10, 8))
    with pytest.raises(ValueError, match="kernel='rbf'"):
        hip_ops.vendi_groups(rows, None, [0, 10], "rbf")
    with pytest.raises(ValueError, match="exactly one of"):
        hip_ops.vendi_groups(rows, None, [0, 10], "gaussian")
    with pytest.raises(ValueError, match="gamma"):
        hip_ops.vendi_groups(rows, None, [0, 10], "gaussian", gamma=0.0)
    with pytest.raises(ValueError, match="neither gamma"):
        hip_ops.vendi_gram(rows, None, "cosine", gamma=1.0)
    with pytest.raises(ValueError, match="offsets must start at 0"):
        hip_ops.vendi_groups(rows, None, [0, 5, 5], "cosine")
    with pytest.raises(ValueError, match="1 .. 2048 rows"):
        hip_ops.vendi_gram(torch.zeros((2049, 8)))
    with pytest.raises(ValueError, match="non-empty"):
        hip_ops.vendi_moment(torch.zeros((0, 8)))


def test_route_choice(am):
    from audio_metrics_amd.metrics.vendi import _choose_route
    assert _choose_route(None, "cosine", 128, 20) == "groups" and _choose_route(None, "gaussian", 1, 512) == "groups"
    assert _choose_route(None, "cosine", 129, 128) == "moment" and _choose_route(None, "cosine", 129, 129) == "gram"
    assert _choose_route(None, "gaussian", 129, 20) == "gram" and _choose_route(None, "gaussian", 2048, 20) == "gram"
    assert _choose_route(None, "cosine", 100000, 512) == "moment" and _choose_route(None, "cosine", 3000, 4096) == "moment"
    assert _choose_route("gram", "cosine", 300, 64) == "gram" and _choose_route("moment", "cosine", 64, 132) == "moment"


# ------------------------------------------------------------------ the C entry points: queries and error paths
def test_host_queries(am, lib):
    assert lib.am_vendi_groups_max_rows() == 128 and lib.am_vendi_gram_max_rows() == 2048
    assert am.hip_ops.vendi_groups_max_rows() == 128 and am.hip_ops.vendi_gram_max_rows() == 2048
    assert lib.am_vendi_groups_workspace_bytes(100, 10, 64) >= 8 + 11 * 8
    for bad in ((0, 1, 8), (10, 0, 8), (10, 1, 0)):
        assert lib.am_vendi_groups_workspace_bytes(*bad) == 0
    assert lib.am_vendi_gram_workspace_bytes(2048, 512) >= 2048 * 512 * 8 and lib.am_vendi_gram_workspace_bytes(2049, 512) == 0
    assert lib.am_vendi_moment_chunks(0, 8) == 0 and lib.am_vendi_moment_chunks(8, 0) == 0
    assert lib.am_vendi_moment_chunks(100, 64) == 1 and lib.am_vendi_moment_chunks(700, 64) == 5
    assert lib.am_vendi_moment_chunks(513, 20) == 4 and lib.am_vendi_moment_chunks(300, 64) == 2
    assert lib.am_vendi_moment_chunks(100000, 512) == 29 and lib.am_vendi_moment_chunks(100000, 128) == 256
    for n, d in ((700, 64), (100000, 512)):
        assert lib.am_vendi_moment_workspace_bytes(n, d) >= lib.am_vendi_moment_chunks(n, d) * d * d * 8 + n * 8


def test_entry_point_error_paths(lib):
    offs = (ctypes.c_int64 * 3)(0, 5, 10)
    nb = lib.am_vendi_groups_workspace_bytes(10, 2, 8)

    def groups(x=FAKE, n=10, ld=8, d=8, idx=None, offsets=offs, b=2, kernel=0, gamma=0.0, gdev=None, rec=FAKE, ev=FAKE, ws=FAKE, ws_bytes=nb,
               name="am_vendi_groups_f32"):
        return getattr(lib, name)(x, n, ld, d, idx, ctypes.cast(offsets, ctypes.c_void_p), b, kernel, gamma, gdev, rec, ev, ws, ws_bytes, None)
    assert groups(x=None) == BAD_ARG and groups(rec=None) == BAD_ARG and groups(ev=None) == BAD_ARG
    assert groups(n=0) == BAD_SHAPE and groups(d=0) == BAD_SHAPE
    assert groups(kernel=2) == BAD_ARG and b"kernel=2" in lib.am_last_error()
    assert groups(kernel=1, gamma=0.0) == BAD_ARG and groups(kernel=1, gamma=float("inf")) == BAD_ARG
    assert groups(ld=6) == BAD_ARG                                       # float32 rows: ld % 4
    assert groups(ld=6, name="am_vendi_groups_f64") == BAD_ARG           # ld < D
    assert groups(offsets=(ctypes.c_int64 * 3)(1, 5, 10)) == BAD_ARG
    assert groups(offsets=(ctypes.c_int64 * 3)(0, 5, 5)) == BAD_SHAPE
    big = (ctypes.c_int64 * 3)(0, 129, 130)
    assert groups(n=200, offsets=big) == BAD_SHAPE and b"group 0 has 129 rows" in lib.am_last_error()
    assert groups(n=9) == BAD_SHAPE                                      # no index list: 10 listed rows, 9 stored
    assert groups(ws_bytes=8) == WORKSPACE
    nbg = lib.am_vendi_gram_workspace_bytes(10, 8)
    for name in ("am_vendi_gram_f32", "am_vendi_gram_f64"):
        f = getattr(lib, name)
        assert f(FAKE, 4000, 8, 8, None, 2049, 0, 0.0, None, FAKE, FAKE, 1 << 30, None) == BAD_SHAPE
        assert b"am_vendi_gram_max_rows" in lib.am_last_error()
        assert f(FAKE, 10, 8, 8, None, 10, 0, 0.0, None, None, FAKE, nbg, None) == BAD_ARG
        assert f(FAKE, 10, 8, 8, None, 10, 3, 0.0, None, FAKE, FAKE, nbg, None) == BAD_ARG
        assert f(FAKE, 10, 8, 8, None, 10, 1, -1.0, None, FAKE, FAKE, nbg, None) == BAD_ARG
        assert f(FAKE, 10, 8, 8, None, 11, 0, 0.0, None, FAKE, FAKE, nbg, None) == BAD_SHAPE
        assert f(FAKE, 10, 8, 8, None, 10, 0, 0.0, None, FAKE, FAKE, 16, None) == WORKSPACE
    nbm = lib.am_vendi_moment_workspace_bytes(10, 8)
    for name in ("am_vendi_moment_f32", "am_vendi_moment_f64"):
        f = getattr(lib, name)
        assert f(None, 10, 8, 8, FAKE, FAKE, nbm, None) == BAD_ARG and f(FAKE, 10, 8, 8, None, FAKE, nbm, None) == BAD_ARG
        assert f(FAKE, 0, 8, 8, FAKE, FAKE, nbm, None) == BAD_SHAPE and f(FAKE, 10, 4, 8, FAKE, FAKE, nbm, None) == BAD_ARG
        assert f(FAKE, 10, 8, 8, FAKE, FAKE, 16, None) == WORKSPACE


# ------------------------------------------------------------------ the oracles against each other
@pytest.mark.parametrize("kind", ["randn", "song", "dups"])
def test_oracles_agree(kind):
    """eigvalsh of K / n and the squared singular values of the normalised rows give the same kept eigenvalues and scores:
    the spread that the 1e-12 bar of the device tests stands on (measured here: 3.6e-15 at orders 1, 2 and inf, 9.3e-15 at
    order 0.5; a second LAPACK driver widens order 0.5 to 1.1e-12, which is why the device tests hold it to 1e-9)."""
    worst = {1.0: 0.0, 2.0: 0.0, float("inf"): 0.0, 0.5: 0.0}
    for d in (20, 64, 132):
        for n in (2, 3, 15, 16, 17, 33, 64, 127, 128):
            x = vr.family_rows(kind, n, d, np.random.default_rng(1000 * d + n))
            a = vr.oracle(x, "cosine", orders=tuple(worst))
            kept = vr.apply_zero_rule(vr.svd_eigenvalues(x), vr.group_zero_tol(n), clearance=1e3)
            assert a["rank"] == kept.size
            assert np.abs(a["kept"] - kept).max() <= 1e-14 * kept[0]
            for q in worst:
                worst[q] = max(worst[q], abs(vr.score(kept, q) / a["scores"][q] - 1.0))
            xu = x / np.linalg.norm(x, axis=1, keepdims=True)
            vr.oracle(xu, "gaussian", 0.7)                       # the clearance condition holds for the Gaussian cases too
    print(kind, worst)
    assert worst[1.0] <= 1e-13 and worst[2.0] <= 1e-13 and worst[float("inf")] <= 1e-13 and worst[0.5] <= 1e-11
