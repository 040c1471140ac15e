"""Nearest-neighbour search, the part that needs no GPU: validation before any device call (nearest_neighbors and
hip_ops.knn_search), the new names in header / signature table / package, the entry point's error paths and workspace
query, and the compile-time resource check of csrc/knn_search.hip (no scratch memory in any instantiation, two workgroups
per CU for the lists of 8 and 16 keys)."""
import ctypes
import os
import re

import pytest
import torch

from kernel_resources import needs_hipcc, resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -4
FAKE = ctypes.c_void_p(0x10000)                       # 16-byte aligned, never dereferenced: the calls stop at validation
NAMES = ("am_knn_search_workspace_bytes", "am_knn_search_chunks", "am_knn_search_f32")


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


def test_validation_happens_before_any_device_call(am, monkeypatch):
    from audio_metrics_amd import hip_ops

    def forbidden(*a, **k):
        raise AssertionError("device call before validation")
    for name in ("as_matrix", "_call", "_workspace"):
        monkeypatch.setattr(hip_ops, name, forbidden)
    ok, other = host_set(am, torch.zeros((10, 8))), host_set(am, torch.zeros((12, 8)))
    # hip_ops.knn_search itself (host tensors: nothing below may touch them)
    with pytest.raises(NotImplementedError, match=r"knn_search takes float32 rows \(the float64 matrix-core form is not implemented\)"):
        hip_ops.knn_search(torch.zeros((10, 8), dtype=torch.float64), torch.zeros((12, 8)), 1)
    with pytest.raises(NotImplementedError, match="float32 rows"):
        hip_ops.knn_search(torch.zeros((10, 8)), torch.zeros((12, 8), dtype=torch.float64), 1)
    with pytest.raises(ValueError, match="feature widths"):
        hip_ops.knn_search(torch.zeros((10, 8)), torch.zeros((12, 12)), 1)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="k=%d" % bad):
            hip_ops.knn_search(torch.zeros((10, 8)), torch.zeros((12, 8)), bad)
    # nearest_neighbors: with the search itself forbidden too
    monkeypatch.setattr(hip_ops, "knn_search", forbidden)
    for empty in (am.AudioMetricsData(False), host_set(am, torch.zeros((0, 8)))):
        with pytest.raises(ValueError, match="keeps none"):             # no stored rows, either side
            am.nearest_neighbors(empty, ok)
        with pytest.raises(ValueError, match="keeps none"):
            am.nearest_neighbors(ok, empty)
    with pytest.raises(ValueError, match="feature widths"):
        am.nearest_neighbors(ok, host_set(am, torch.zeros((10, 12))))
    for bad in (0, 33):
        with pytest.raises(ValueError, match="k=%d" % bad):
            am.nearest_neighbors(ok, other, k=bad)
    with pytest.raises(ValueError, match="exclude_self"):
        am.nearest_neighbors(ok, other, exclude_self=True)
    with pytest.raises(NotImplementedError, match="float64"):
        am.nearest_neighbors(ok, host_set(am, torch.zeros((10, 8), dtype=torch.float64)))
    with pytest.raises(NotImplementedError, match="float64"):
        am.nearest_neighbors(host_set(am, torch.zeros((10, 8), dtype=torch.float64)), ok)


def test_header_exports_signature_table_and_package_agree(am, lib):
    with open(os.path.join(ROOT, "include", "audio_metrics_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in am._lib.SIGNATURES and hasattr(lib, name), name
    assert len(am._lib.SIGNATURES["am_knn_search_f32"][1]) == 15
    from audio_metrics_amd.metrics import neighbors
    assert am.nearest_neighbors is neighbors.nearest_neighbors
    assert callable(am.hip_ops.knn_search) and am.hip_ops.KNN_SEARCH_MAX_K == 32
    assert "scalars" in am.nearest_neighbors.__doc__                    # says that it is not a row of evaluate()


def test_entry_point_error_paths(lib):
    n, m, d, k = 1000, 3000, 64, 5
    nb = lib.am_knn_search_workspace_bytes(n, m, d, k)

    def call(x=FAKE, n=n, ldx=d, y=FAKE, m=m, ldy=d, d=d, k=k, off=-1, dist=FAKE, idx=FAKE, ws=FAKE, nb=nb):
        return lib.am_knn_search_f32(x, n, ldx, y, m, ldy, d, k, off, 0, dist, idx, ws, nb, None)
    assert call(x=None) == BAD_ARG and call(y=None) == BAD_ARG
    assert call(dist=None) == BAD_ARG and "out_dist is null" in lib.am_last_error().decode()
    assert call(idx=None) == BAD_ARG and "out_idx is null" in lib.am_last_error().decode()
    assert call(n=0) == BAD_SHAPE and call(m=0) == BAD_SHAPE and call(d=0) == BAD_SHAPE
    assert call(k=0) == BAD_SHAPE and call(k=33) == BAD_SHAPE and "33" in lib.am_last_error().decode()
    # the alignment / leading-dimension rules of am_knn_radii_f32
    assert call(ldx=d - 4) == BAD_ARG and call(ldy=d + 1) == BAD_ARG and call(x=ctypes.c_void_p(0x10004)) == BAD_ARG
    assert call(m=1 << 32) == BAD_SHAPE                                 # a column takes 32 bits of a key
    assert call(nb=nb - 1) == WORKSPACE and str(nb) in lib.am_last_error().decode()
    assert call(ws=None) == WORKSPACE and call(nb=0) == WORKSPACE


def test_workspace_and_chunk_queries(lib):
    for bad in ((0, 10, 8, 1), (10, 0, 8, 1), (10, 10, 0, 1), (10, 10, 8, 0), (10, 10, 8, 33)):
        assert lib.am_knn_search_workspace_bytes(*bad) == 0 and lib.am_knn_search_chunks(*bad) == 0, bad
    assert lib.am_knn_search_chunks(130, 300, 40, 5) == 3              # one per column tile at most
    assert lib.am_knn_search_chunks(130, 4000, 40, 5) == 32
    assert 8 <= lib.am_knn_search_chunks(100_000, 100_000, 512, 5) <= 64
    prev = 0
    for k, cap in ((1, 8), (8, 8), (9, 16), (16, 16), (17, 32), (32, 32)):
        n, m = 1000, 5000
        nb = lib.am_knn_search_workspace_bytes(n, m, 64, k)
        chunks = lib.am_knn_search_chunks(n, m, 64, k)
        lists = chunks * n * cap * 8                                      # uint64 [nchunks][N][KCAP]
        assert lists + (n + m) * 4 <= nb <= lists + (n + m) * 4 + 3 * 256 and nb >= prev, (k, nb)
        prev = nb
    assert lib.am_knn_search_workspace_bytes(3, 2, 8, 5) > 0             # fewer rows than k is allowed: (+inf, -1) entries


@needs_hipcc
def test_knn_search_kernels_use_no_scratch_memory():
    usage = resource_usage("knn_search.hip")
    search = {n: u for n, u in usage.items() if "knn_search" in n}
    # tile kernel: lists of 8 / 16 / 32 keys x with / without an inner-dimension tail x exclusion by index / by label;
    # merge kernel: one per list length
    tile = {n: u for n, u in search.items() if "knn_search_kernel" in n}
    merge = {n: u for n, u in search.items() if "knn_search_merge_kernel" in n}
    assert len(tile) == 12 and len(merge) == 3 and len(search) == 15, sorted(usage)
    for n, u in search.items():
        assert u["scratch"] == 0, (n, u)
    for cap in (8, 16):
        hits = {n: u for n, u in tile.items() if "ILi%dELb" % cap in n}
        assert len(hits) == 4, (cap, sorted(tile))
        for n, u in hits.items():
            assert u["vgprs"] <= 256 and u["occupancy"] >= 2, (n, u)       # two workgroups of four waves per CU
