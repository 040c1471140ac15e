"""The float64 Kernel Audio Distance path, the part that needs no GPU: which entry points two float64 sets, two float32 sets
and a mixed pair reach (the device layer replaced by recorders), the error paths of the three *_f64 entry points (validated
before the first HIP call), and the compile-time resource check of csrc/kad_f64.hip."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-metrics_amd", "csrc")
BAD_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -4
FAKE = ctypes.c_void_p(0x10008)                       # 8-byte aligned only, never dereferenced: the calls stop at validation
NEW_SYMBOLS = ("am_pairwise_select_f64_workspace_bytes", "am_pairwise_select_f64", "am_mmd_rbf_f64_workspace_bytes",
               "am_mmd_rbf_f64", "am_mmd_rbf_groups_f64_workspace_bytes", "am_mmd_rbf_groups_f64")


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    return audio_metrics_amd


@pytest.fixture(scope="module")
def lib(am):
    return am._lib.load()


# ---------------------------------------------------------------------------------------------------- C1. routing
def test_signature_table_header_and_exports_hold_the_six_symbols(am, lib):
    with open(os.path.join(ROOT, "include", "audio_metrics_hip.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name in am._lib.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        f32 = name.replace("_f64_workspace_bytes", "_workspace_bytes").replace("_f64", "_f32")
        assert am._lib.SIGNATURES[name] == am._lib.SIGNATURES[f32], (name, f32)        # the same argument lists


@pytest.fixture
def recorder(am, monkeypatch):
    """hip_ops with its device layer replaced: _call records the entry point's name, the matrix helpers pass host tensors on"""
    ops = am.hip_ops
    log = {"calls": [], "as_matrix": 0, "as_matrix64": 0, "workspace": 0, "require_cuda": 0}

    def fake_call(lib, name, device, *args):
        log["calls"].append(name)

    def fake_workspace(nbytes, device):
        log["workspace"] += 1
        return torch.zeros(max(int(nbytes), 16), dtype=torch.uint8)

    def fake_matrix(e, name="embeddings"):
        log["as_matrix"] += 1
        assert e.dtype == torch.float32
        return e

    def fake_matrix64(e, name="embeddings"):
        log["as_matrix64"] += 1
        assert e.dtype == torch.float64
        return e

    def fake_require_cuda(t, name):                                       # (the index list of a host-side set is a host tensor)
        log["require_cuda"] += 1
    monkeypatch.setattr(ops, "_require_cuda", fake_require_cuda)
    monkeypatch.setattr(ops, "_call", fake_call)
    monkeypatch.setattr(ops, "_workspace", fake_workspace)
    monkeypatch.setattr(ops, "as_matrix", fake_matrix)
    monkeypatch.setattr(ops, "as_matrix64", fake_matrix64)
    return log


def _ops_calls(ops, x, y):
    ops.pairwise_select_sq(y)
    ops.mmd_rbf_sums(x, y, gamma=0.5)
    ops.mmd_rbf_group_sums(x, None, [0, 4, 10], y, gamma=0.5, rows=True)


def test_ops_layer_routes_by_row_type(am, recorder):
    ops = am.hip_ops
    x64, y64 = torch.zeros((10, 8), dtype=torch.float64), torch.zeros((12, 8), dtype=torch.float64)
    _ops_calls(ops, x64, y64)
    assert recorder["calls"] == ["am_pairwise_select_f64", "am_mmd_rbf_f64", "am_mmd_rbf_groups_f64"]
    assert recorder["as_matrix64"] == 5 and recorder["as_matrix"] == 0
    recorder["calls"].clear()
    _ops_calls(ops, x64.float(), y64.float())
    assert recorder["calls"] == ["am_pairwise_select_f32", "am_mmd_rbf_f32", "am_mmd_rbf_groups_f32"]
    assert recorder["as_matrix64"] == 5 and recorder["as_matrix"] == 5
    # exactly one float64 argument: refused before anything touches the tensors
    before = dict(recorder, calls=list(recorder["calls"]))
    for a, b in ((x64, y64.float()), (x64.float(), y64)):
        with pytest.raises(NotImplementedError, match="takes float32 rows"):
            ops.mmd_rbf_sums(a, b, gamma=0.5)
        with pytest.raises(NotImplementedError, match="takes float32 rows"):
            ops.mmd_rbf_group_sums(a, None, [0, 10], b, gamma=0.5)
    assert recorder == before
    # the select keeps returning a float32 scalar
    out = ops.pairwise_select_sq(y64)
    assert out.dtype == torch.float32 and out.dim() == 0


def _host_set(am, rows):
    s = am.AudioMetricsData(True)
    s._embeddings = rows
    return s


def test_metric_layer_routes_by_row_type(am, recorder):
    """kernel_audio_distance and kernel_audio_distance_per_group on host-side sets: the read-backs see the zeros the fake
    device layer left, so only the calls are looked at."""
    labels = [0] * 4 + [1] * 6
    for dtype, kind in ((torch.float64, "f64"), (torch.float32, "f32")):
        x, y = _host_set(am, torch.zeros((10, 8), dtype=dtype)), _host_set(am, torch.zeros((12, 8), dtype=dtype))
        recorder["calls"].clear()
        am.kernel_audio_distance(x, y, bandwidth=2.0)
        assert recorder["calls"] == ["am_mmd_rbf_" + kind]
        recorder["calls"].clear()
        am.kernel_audio_distance_per_group(x, y, labels, bandwidth=3.0)
        assert recorder["calls"] == ["am_mmd_rbf_" + kind, "am_mmd_rbf_groups_" + kind]
        recorder["calls"].clear()
        try:                                                              # bandwidth=None reaches the select of that kind first
            am.kernel_audio_distance(x, _host_set(am, torch.zeros((12, 8), dtype=dtype)))
        except ValueError as e:                                           # (nothing wrote the "median": it may be refused)
            assert "median pairwise distance" in str(e)
        assert recorder["calls"][0] == "am_pairwise_select_" + kind
    # mixed pairs: NotImplementedError before any of the patched functions is called
    before = dict(recorder, calls=list(recorder["calls"]))
    x32, x64 = _host_set(am, torch.zeros((10, 8))), _host_set(am, torch.zeros((10, 8), dtype=torch.float64))
    with pytest.raises(NotImplementedError, match="candidate set holds float64"):
        am.kernel_audio_distance(x64, x32)
    with pytest.raises(NotImplementedError, match="reference set holds float64"):
        am.kernel_audio_distance(x32, x64)
    with pytest.raises(NotImplementedError, match="candidate set holds float64"):
        am.kernel_audio_distance_per_group(x64, x32, labels)
    with pytest.raises(NotImplementedError, match="reference set holds float64"):
        am.kernel_audio_distance_per_group(x32, x64, labels)
    assert recorder == before


# ---------------------------------------------------------------------------------------------------- C ABI without a device
def test_f64_entry_points_validate_before_any_device_work(lib):
    n, d = 1000, 33
    nb = lib.am_pairwise_select_f64_workspace_bytes(n, d)
    pairs = n * (n - 1) // 2

    def sel(x=FAKE, n=n, ld=d, d=d, rank=-1, out=FAKE, ws=FAKE, nb=nb):
        return lib.am_pairwise_select_f64(x, n, ld, d, rank, out, ws, nb, None)
    assert sel(x=None) == BAD_ARG and sel(out=None) == BAD_ARG
    assert sel(n=1) == BAD_SHAPE and sel(d=0) == BAD_SHAPE and sel(rank=pairs) == BAD_SHAPE and sel(n=1 << 31) == BAD_SHAPE
    assert sel(ld=d - 1) == BAD_ARG
    assert sel(nb=nb - 1) == WORKSPACE and str(nb) in lib.am_last_error().decode() and sel(ws=None) == WORKSPACE
    assert nb >= n * 8 and lib.am_pairwise_select_f64_workspace_bytes(1, d) == 0

    n1, n2 = 1000, 300
    nb = lib.am_mmd_rbf_f64_workspace_bytes(n1, n2, d, 7)

    def mmd(x=FAKE, n1=n1, ldx=d, y=FAKE, n2=n2, ldy=d, d=d, bw2=None, gamma=0.5, blocks=7, out=FAKE, ws=FAKE, nb=nb):
        return lib.am_mmd_rbf_f64(x, n1, ldx, y, n2, ldy, d, bw2, gamma, blocks, out, ws, nb, None)
    assert mmd(x=None) == BAD_ARG and mmd(y=None) == BAD_ARG and mmd(out=None) == BAD_ARG
    assert mmd(blocks=0) == BAD_ARG and mmd(blocks=8) == BAD_ARG and mmd(gamma=-1.0) == BAD_ARG
    assert mmd(n1=0) == BAD_SHAPE and mmd(n2=0) == BAD_SHAPE and mmd(d=0) == BAD_SHAPE
    assert mmd(ldx=d - 1) == BAD_ARG and mmd(ldy=d - 1) == BAD_ARG
    assert mmd(nb=nb - 1) == WORKSPACE and str(nb) in lib.am_last_error().decode()
    assert mmd(blocks=4, nb=lib.am_mmd_rbf_f64_workspace_bytes(n1, n2, d, 4) - 1) == WORKSPACE
    full = lib.am_mmd_rbf_f64_workspace_bytes(5000, 700, 64, 7)
    assert all(0 < lib.am_mmd_rbf_f64_workspace_bytes(5000, 700, 64, b) <= full for b in range(1, 7))
    assert lib.am_mmd_rbf_f64_workspace_bytes(10, 10, 64, 0) == 0

    offs = (ctypes.c_int64 * 4)(0, 1, 300, 1000)
    nb = lib.am_mmd_rbf_groups_f64_workspace_bytes(1000, 3, n2, d)

    def grp(x=FAKE, n1=n1, ldx=d, idx=None, offs=offs, b=3, y=FAKE, n2=n2, ldy=d, d=d, gamma=0.5, out=FAKE, ws=FAKE, nb=nb):
        return lib.am_mmd_rbf_groups_f64(x, n1, ldx, idx, ctypes.cast(offs, ctypes.c_void_p), b, y, n2, ldy, d, None, gamma, out, None,
                                         ws, nb, None)
    assert grp(x=None) == BAD_ARG and grp(y=None) == BAD_ARG and grp(out=None) == BAD_ARG and grp(gamma=-1.0) == BAD_ARG
    assert grp(n2=1) == BAD_SHAPE and grp(d=0) == BAD_SHAPE and grp(ldx=d - 1) == BAD_ARG and grp(ldy=d - 1) == BAD_ARG
    assert grp(offs=(ctypes.c_int64 * 4)(0, 1, 1, 1000)) == BAD_SHAPE and grp(offs=(ctypes.c_int64 * 4)(1, 2, 300, 1000)) == BAD_ARG
    assert grp(n1=999) == BAD_SHAPE                                    # no index list: the groups name more rows than X holds
    assert grp(nb=nb - 1) == WORKSPACE and str(nb) in lib.am_last_error().decode() and grp(ws=None) == WORKSPACE
    assert lib.am_mmd_rbf_groups_f64_workspace_bytes(1 << 30, 3, n2, d) == 0 and nb >= 8 + 4 * 8 + 1000 * 8


# ---------------------------------------------------------------------------------------------------- C2. compile-time resources
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_kad_f64_kernels_use_no_scratch_memory_and_fit_two_workgroups_per_cu():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    import importlib.util
    spec = importlib.util.spec_from_file_location("am_build", os.path.join(ROOT, "audio-metrics_amd", "_build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)                                         # the flags the shipped library is built with
    r = subprocess.run([hipcc, *build.HIPCC_FLAGS, "--cuda-device-only", "-c", "kad_f64.hip", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        for key, short in (("ScratchSize \\[bytes/lane\\]", "scratch"), ("VGPRs", "vgprs"), ("Occupancy \\[waves/SIMD\\]", "occupancy"),
                           ("LDS Size \\[bytes/block\\]", "lds")):
            m = re.search(r"remark:\s+%s: (\d+)" % key, line)
            if m and name:
                usage[name][short] = int(m.group(1))
    stages = 4 * 64 * 17 * 8                                               # two stages x (Q slab, P slab) of 64 rows x 17 doubles
    assert stages == 34816
    # (kernel, instances, LDS beside the stages: the norms / groups of the Q tile, the select's 2048 counters, the wave sums)
    tile_kernels = (("kad64_select_kernel", 3, 64 * 8 + 2048 * 4), ("kad64_mmd_kernel", 1, 64 * 8 + 4 * 8),
                    ("kadg64_rows_kernel", 2, 64 * 8 + 64 * 4))
    # (the scan, reduce, row-sum and finish kernels are those of the f32 forms: tests/test_kad_cpu.py, test_mmd_multi_cpu.py,
    # test_kad_groups_cpu.py)
    small_kernels = (("kad64_norms_kernel", 1), ("kadg64_prep_kernel", 1))
    assert sum(c for _, c, *_ in tile_kernels + small_kernels) == len(usage), sorted(usage)
    for n, u in usage.items():
        assert u["scratch"] == 0, (n, u)
    for kernel, count, side in tile_kernels:
        hits = {n: u for n, u in usage.items() if kernel in n}
        assert len(hits) == count, (kernel, sorted(usage))
        for n, u in hits.items():
            assert u["lds"] == stages + side, (n, u)
            assert 2 * u["lds"] <= 160 * 1024 and u["vgprs"] <= 256 and u["occupancy"] >= 2, (n, u)   # two workgroups of four waves per CU
    for kernel, count in small_kernels:
        assert len([n for n in usage if kernel in n]) == count, (kernel, sorted(usage))
