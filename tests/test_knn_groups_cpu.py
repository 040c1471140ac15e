"""The leave-group-out nearest-neighbour search and what stands on it, the part that needs no GPU: validation before any
device call (hip_ops.knn_search_groups, nearest_neighbors(groups=...), nearest_neighbor_two_sample_test), the new names in
header / signature table / package, the C entry's error codes and workspace query.  (The compile-time resources of the
by-label kernels: test_knn_search_resources_cpu.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -4
FAKE = ctypes.c_void_p(0x10000)                       # 16-byte aligned, never dereferenced: the calls stop at validation
NAMES = ("am_knn_search_groups_workspace_bytes", "am_knn_search_groups_f32")


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


def test_raw_op_validates_before_any_device_call(monkeypatch):
    from audio_metrics_amd import hip_ops
    for name in ("as_matrix", "_call", "_workspace"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    x, y = torch.zeros((10, 8)), torch.zeros((12, 8))
    gx, gy = torch.zeros(10, dtype=torch.int32), torch.zeros(12, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match=r"knn_search_groups takes float32 rows"):
        hip_ops.knn_search_groups(x.double(), y, 1, gx, gy)
    with pytest.raises(NotImplementedError, match="float32 rows"):
        hip_ops.knn_search_groups(x, y.double(), 1, gx, gy)
    with pytest.raises(ValueError, match="2-D"):
        hip_ops.knn_search_groups(x[0], y, 1, gx, gy)
    with pytest.raises(ValueError, match="feature widths"):
        hip_ops.knn_search_groups(x, torch.zeros((12, 12)), 1, gx, gy)
    with pytest.raises(ValueError, match="rows on both sides"):
        hip_ops.knn_search_groups(x[:0], y, 1, gx[:0], gy)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="k=%d" % bad):
            hip_ops.knn_search_groups(x, y, bad, gx, gy)
    with pytest.raises(ValueError, match="x_group must be an int32 tensor"):
        hip_ops.knn_search_groups(x, y, 1, gx.long(), gy)
    with pytest.raises(ValueError, match="y_group must be an int32 tensor"):
        hip_ops.knn_search_groups(x, y, 1, gx, np.zeros(12, dtype=np.int32))
    with pytest.raises(ValueError, match="x_group must hold one label per row"):
        hip_ops.knn_search_groups(x, y, 1, gx[:9], gy)
    with pytest.raises(ValueError, match="y_group must hold one label per row"):
        hip_ops.knn_search_groups(x, y, 1, gx, gy.reshape(12, 1))
    with pytest.raises(ValueError, match="x_group lives on"):
        hip_ops.knn_search_groups(x, y, 1, gx.to("meta"), gy)


def test_front_ends_validate_before_any_device_call(am, monkeypatch):
    from audio_metrics_amd import hip_ops
    for name in ("as_matrix", "_call", "_workspace", "knn_search", "knn_search_groups", "upload_host_array"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    ok, other = host_set(am, torch.zeros((10, 8))), host_set(am, torch.zeros((12, 8)))
    g10, g12 = np.arange(10) // 2, np.arange(12) // 3
    # nearest_neighbors
    with pytest.raises(ValueError, match="exclude_self=True together with groups"):
        am.nearest_neighbors(ok, ok, exclude_self=True, groups=g10)
    with pytest.raises(ValueError, match="groups without searched_groups"):
        am.nearest_neighbors(ok, other, groups=g10)
    with pytest.raises(ValueError, match="searched_groups without groups"):
        am.nearest_neighbors(ok, other, searched_groups=g12)
    with pytest.raises(ValueError, match="10 stored rows"):
        am.nearest_neighbors(ok, other, groups=g12, searched_groups=g12)
    with pytest.raises(ValueError, match="12 stored rows"):
        am.nearest_neighbors(ok, other, groups=g10, searched_groups=g10)
    with pytest.raises(ValueError, match="integer labels"):
        am.nearest_neighbors(ok, ok, groups=g10.astype(np.float32))
    with pytest.raises(ValueError, match="1-D"):
        am.nearest_neighbors(ok, ok, groups=g10.reshape(5, 2))
    with pytest.raises(ValueError, match="keeps none"):
        am.nearest_neighbors(am.AudioMetricsData(False), ok, groups=g10, searched_groups=g10)
    with pytest.raises(ValueError, match="feature widths"):
        am.nearest_neighbors(ok, host_set(am, torch.zeros((12, 12))), groups=g10, searched_groups=g12)
    with pytest.raises(NotImplementedError, match="float64"):
        am.nearest_neighbors(ok, host_set(am, torch.zeros((12, 8), dtype=torch.float64)), groups=g10, searched_groups=g12)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="k=%d" % bad):
            am.nearest_neighbors(ok, ok, k=bad, groups=g10)
    # nearest_neighbor_two_sample_test
    test = am.nearest_neighbor_two_sample_test
    for bad in (0, 33):
        with pytest.raises(ValueError, match="k=%d" % bad):
            test(ok, other, k=bad)
    with pytest.raises(ValueError, match="n_permutations"):
        test(ok, other, n_permutations=0)
    with pytest.raises(ValueError, match="keeps none"):
        test(am.AudioMetricsData(False), other)
    with pytest.raises(ValueError, match="keeps none"):
        test(ok, host_set(am, torch.zeros((0, 8))), ref_groups=g12)
    with pytest.raises(ValueError, match="12 labels for 10 stored rows"):
        test(ok, other, groups=g12)
    with pytest.raises(ValueError, match="integer labels"):
        test(ok, other, ref_groups=g12.astype(np.float64))
    with pytest.raises(NotImplementedError, match="float64"):
        test(host_set(am, torch.zeros((10, 8), dtype=torch.float64)), other)
    with pytest.raises(ValueError, match="feature widths"):
        test(ok, host_set(am, torch.zeros((12, 12))))
    with pytest.raises(ValueError, match=r"candidate set has 1 unit\(s\)"):
        test(ok, other, groups=np.zeros(10, dtype=np.int64))
    with pytest.raises(ValueError, match=r"reference set has 1 unit\(s\)"):
        test(ok, host_set(am, torch.zeros((1, 8))))


def test_plain_path_of_nearest_neighbors_is_untouched(am, monkeypatch):
    """without labels the call that reaches hip_ops is today's, argument for argument"""
    from audio_metrics_amd import hip_ops
    seen = {}

    def fake(x, y, k, self_offset=None, squared=False):
        seen.update(k=k, self_offset=self_offset, squared=squared, same=x is y)
        return torch.zeros((x.shape[0], k)), torch.zeros((x.shape[0], k), dtype=torch.int64)
    monkeypatch.setattr(hip_ops, "knn_search", fake)
    monkeypatch.setattr(hip_ops, "knn_search_groups", forbidden)
    ok = host_set(am, torch.zeros((10, 8)))
    res = am.nearest_neighbors(ok, ok, k=3, exclude_self=True, squared=True)
    assert seen == dict(k=3, self_offset=0, squared=True, same=True) and sorted(res) == ["nn_distances", "nn_indices"]


def test_labels_are_mapped_jointly_to_dense_int32_ids(am, monkeypatch):
    from audio_metrics_amd import hip_ops
    seen = {}

    def fake(x, y, k, x_group, y_group, squared=False):
        seen.update(gx=x_group, gy=y_group, same=x is y)
        return torch.zeros((x.shape[0], k)), torch.zeros((x.shape[0], k), dtype=torch.int64)
    monkeypatch.setattr(hip_ops, "knn_search_groups", fake)
    monkeypatch.setattr(hip_ops, "knn_search", forbidden)
    a, b = host_set(am, torch.zeros((5, 8))), host_set(am, torch.zeros((4, 8)))
    # any integer values, any order; equal VALUES of the two sets must meet in one id
    res = am.nearest_neighbors(a, b, k=2, groups=np.array([7, -3, 7, 2 ** 40, -3]), searched_groups=torch.tensor([2 ** 40, 5, 7, 5]))
    assert seen["gx"].dtype == torch.int32 and seen["gy"].dtype == torch.int32
    assert seen["gx"].tolist() == [2, 0, 2, 3, 0] and seen["gy"].tolist() == [3, 1, 2, 1]
    assert sorted(res) == ["nn_distances", "nn_indices"] and res["nn_indices"].shape == (5, 2)
    am.nearest_neighbors(a, a, groups=[4, 4, 9, 9, 1])                       # x is y: searched_groups defaults to groups
    assert seen["same"] and seen["gx"].tolist() == seen["gy"].tolist() == [1, 1, 2, 2, 0]


def test_header_exports_signature_table_and_package_agree(am, lib):
    with open(os.path.join(ROOT, "include", "audio_metrics_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in am._lib.SIGNATURES and hasattr(lib, name), name
    assert len(am._lib.SIGNATURES["am_knn_search_groups_f32"][1]) == 16
    from audio_metrics_amd.metrics import neighbors, nn_test
    assert am.nearest_neighbors is neighbors.nearest_neighbors
    assert am.nearest_neighbor_two_sample_test is nn_test.nearest_neighbor_two_sample_test
    assert am.nn_permutation_null is nn_test.nn_permutation_null
    assert callable(am.hip_ops.knn_search_groups)
    import inspect
    params = list(inspect.signature(am.nearest_neighbors).parameters)
    assert params == ["x", "y", "k", "exclude_self", "squared", "groups", "searched_groups"]     # new keywords at the end
    assert list(inspect.signature(am.nearest_neighbor_two_sample_test).parameters) == \
        ["cand", "ref", "groups", "ref_groups", "k", "n_permutations", "seed", "return_rows"]
    assert "nearest_neighbor_two_sample_test" not in am.AudioMetrics.__dict__


def test_entry_point_error_paths(lib):
    n, m, d, k = 1000, 3000, 64, 5
    nb = lib.am_knn_search_groups_workspace_bytes(n, m, d, k)

    def call(x=FAKE, n=n, ldx=d, gx=FAKE, y=FAKE, m=m, ldy=d, gy=FAKE, d=d, k=k, dist=FAKE, idx=FAKE, ws=FAKE, nb=nb):
        return lib.am_knn_search_groups_f32(x, n, ldx, gx, y, m, ldy, gy, d, k, 0, dist, idx, ws, nb, None)
    assert call(x=None) == BAD_ARG and call(y=None) == BAD_ARG
    assert call(gx=None) == BAD_ARG and "x_group is null" in lib.am_last_error().decode()
    assert call(gy=None) == BAD_ARG and "y_group is null" in lib.am_last_error().decode()
    assert call(dist=None) == BAD_ARG and "out_dist is null" in lib.am_last_error().decode()
    assert call(idx=None) == BAD_ARG and "out_idx is null" in lib.am_last_error().decode()
    assert call(n=0) == BAD_SHAPE and call(m=0) == BAD_SHAPE and call(d=0) == BAD_SHAPE
    assert call(k=0) == BAD_SHAPE and call(k=33) == BAD_SHAPE and "33" in lib.am_last_error().decode()
    assert call(ldx=d - 4) == BAD_ARG and call(ldy=d + 1) == BAD_ARG and call(x=ctypes.c_void_p(0x10004)) == BAD_ARG
    assert call(m=1 << 32) == BAD_SHAPE                                 # a column takes 32 bits of a key
    assert call(nb=nb - 1) == WORKSPACE and str(nb) in lib.am_last_error().decode()
    assert "am_knn_search_groups_workspace_bytes" in lib.am_last_error().decode()
    assert call(ws=None) == WORKSPACE and call(nb=0) == WORKSPACE


def test_workspace_query(lib):
    for bad in ((0, 10, 8, 1), (10, 0, 8, 1), (10, 10, 0, 1), (10, 10, 8, 0), (10, 10, 8, 33)):
        assert lib.am_knn_search_groups_workspace_bytes(*bad) == 0, bad
    for k, cap in ((1, 8), (8, 8), (9, 16), (16, 16), (17, 32), (32, 32)):
        n, m = 1000, 5000
        nb = lib.am_knn_search_groups_workspace_bytes(n, m, 64, k)
        lists = lib.am_knn_search_chunks(n, m, 64, k) * n * cap * 8         # uint64 [nchunks][N][KCAP], the plan of the plain search
        assert lists + (n + m) * 4 <= nb <= lists + (n + m) * 4 + 3 * 256, (k, nb)
        assert nb == lib.am_knn_search_workspace_bytes(n, m, 64, k)          # the labels are the caller's: nothing more to hold
    assert lib.am_knn_search_groups_workspace_bytes(3, 2, 8, 5) > 0
