"""The group-list protocol - group b is rows[idx[offsets[b]:offsets[b + 1]]] - where its three users share it, without a
device: the validation of csrc/groups_common.h behind am_stats_gather_*, am_frechet_groups_* and am_mmd_rbf_groups_f32
(it runs before the first HIP call, so fake pointers do), the workspace queries, and the helpers of hip_ops.py behind
stats_gather, frechet_groups and mmd_rbf_group_sums (offsets, index list, the flag word's check())."""
import ctypes
import re

import pytest
import torch

BAD_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -4
FAKE = ctypes.c_void_p(0x10000)                       # 16-byte aligned, never dereferenced: the calls stop at validation
N, D, N2, SIZES = 1000, 64, 300, [5, 7, 1, 3]


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    return audio_metrics_amd


@pytest.fixture(scope="module")
def lib(am):
    return am._lib.load()


def _offsets_of(sizes):
    offs = [0]
    for s in sizes:
        offs.append(offs[-1] + s)
    return offs


# ---------------------------------------------------------------------------------------------------- C ABI
ENTRIES = ["am_stats_gather_f32", "am_stats_gather_f64", "am_frechet_groups_f32", "am_frechet_groups_f64", "am_mmd_rbf_groups_f32"]


def _caller(lib, entry):
    """call(**overrides) -> status of `entry` on fake pointers, and the workspace size of the default arguments."""
    def workspace(offs):
        n_total, b = offs[-1], len(offs) - 1
        if "stats_gather" in entry:
            return lib.am_stats_gather_workspace_bytes(n_total, b, D)
        if "frechet" in entry:
            return lib.am_frechet_groups_workspace_bytes(n_total, b, D)
        return lib.am_mmd_rbf_groups_workspace_bytes(n_total, b, N2, D)
    nb_default = workspace(_offsets_of(SIZES))

    def call(x=FAKE, n=N, ld=D, idx=FAKE, offs=None, b=None, nb=nb_default):
        offs = _offsets_of(SIZES) if offs is None else offs
        arr = (ctypes.c_int64 * len(offs))(*offs)
        po, b = ctypes.cast(arr, ctypes.c_void_p), len(offs) - 1 if b is None else b
        if "mmd" in entry:
            return lib.am_mmd_rbf_groups_f32(x, n, ld, idx, po, b, FAKE, N2, D, D, None, 0.5, FAKE, None, FAKE, nb, None)
        return getattr(lib, entry)(x, n, ld, D, idx, po, b, FAKE, FAKE, *([FAKE] if "frechet" in entry else []), FAKE, nb, None)
    return call, nb_default


@pytest.mark.parametrize("entry", ENTRIES)
def test_c_abi_error_paths(lib, entry):
    call, nb = _caller(lib, entry)
    err = lambda: lib.am_last_error().decode()
    assert nb > 0
    assert call(offs=[1, 5, 9]) == BAD_ARG and "offsets[0]" in err()
    assert call(offs=[0, 5, 5, 9]) == BAD_SHAPE and "group 1 " in err()
    assert call(offs=[0, 5, 4, 9]) == BAD_SHAPE and "group 1 " in err()
    assert call(b=0) == BAD_SHAPE
    assert call(x=None) == BAD_ARG
    if entry.endswith("f32"):
        assert call(ld=D - 4) == BAD_ARG and call(x=ctypes.c_void_p(0x10004)) == BAD_ARG
        assert call(n=1 << 24) == BAD_SHAPE and "4 GiB" in err()
    else:
        assert call(ld=D - 1) == BAD_ARG
    # one byte short of what THIS entry point carves (never more: a call that passed validation would reach the device).
    # The query of the gathered statistics covers both row types, so the float64 layout may need less than it returns.
    assert call(nb=0) == WORKSPACE
    need = int(re.search(r"need (\d+) bytes", err()).group(1))
    assert need == nb or (entry == "am_stats_gather_f64" and 0 < need < nb)
    assert call(nb=need - 1) == WORKSPACE and str(need) in err()
    if "stats_gather" not in entry:                                          # idx = NULL: the groups are stored rows
        assert call(idx=None, n=sum(SIZES) - 1) == BAD_SHAPE and "stored rows" in err()
    if "frechet" in entry:
        assert call(offs=_offsets_of([5, 7, 1, 129])) == BAD_SHAPE
        assert "group 3 " in err() and "129" in err() and "128" in err()


def test_workspace_queries(lib):
    # the figures of the library before the three files shared one head (its queries, run once): the gathered statistics
    # carved flag word and offsets as two 256-byte pieces and may have shrunk by one of them, the other two stay
    before = 921600
    assert before - 256 <= lib.am_stats_gather_workspace_bytes(1000, 4, 64) <= before
    assert lib.am_frechet_groups_workspace_bytes(16, 4, 64) == 16640
    assert lib.am_mmd_rbf_groups_workspace_bytes(16, 4, 300, 64) == 9216


# ---------------------------------------------------------------------------------------------------- hip_ops glue
class _Recorder:
    def __init__(self, monkeypatch, ops):
        self.calls, self.ws = [], None
        monkeypatch.setattr(ops, "_require_cuda", lambda t, name: None)
        monkeypatch.setattr(ops, "_call", lambda lib, name, dev, *args: self.calls.append((name, args)))
        monkeypatch.setattr(ops, "_workspace", self._workspace)

    def _workspace(self, nbytes, device):
        self.ws = torch.zeros(max(int(nbytes), 16), dtype=torch.uint8)
        return self.ws


# name -> (call(ops, idx, offsets) -> check, position of the offsets among the C arguments, noun, idx=None allowed)
def _stats_gather(ops, idx, offsets):
    return ops.stats_gather(torch.zeros((N, D)), idx, offsets, defer_check=True)[-1]


def _frechet_groups(ops, idx, offsets):
    return ops.frechet_groups(torch.zeros((N, D)), idx, offsets, torch.zeros(D, dtype=torch.float64),
                              torch.zeros((D, D), dtype=torch.float64))[-1]


def _group_sums(ops, idx, offsets):
    return ops.mmd_rbf_group_sums(torch.zeros((N, D)), idx, offsets, torch.zeros((N2, D)), gamma=0.5)[-1]


GLUE = {"stats_gather": (_stats_gather, 5, "subset rows", False), "frechet_groups": (_frechet_groups, 5, "group rows", True),
        "mmd_rbf_group_sums": (_group_sums, 4, "group rows", True)}


@pytest.mark.parametrize("name", list(GLUE))
def test_glue(am, monkeypatch, name):
    ops = am.hip_ops
    run, offs_at, noun, idx_optional = GLUE[name]
    rec = _Recorder(monkeypatch, ops)
    idx = torch.arange(9, dtype=torch.int64) * 7
    for bad in ([], [1, 5], [0, 5, 5], [0, 5, 4]):
        with pytest.raises(ValueError, match="offsets must start at 0 and increase strictly"):
            run(ops, idx, bad)
    with pytest.raises(ValueError, match="idx holds 3 entries, offsets name 9"):
        run(ops, idx[:3], [0, 5, 9])
    assert rec.calls == []
    check = run(ops, idx, [0, 5, 9])
    assert len(rec.calls) == 1
    args = rec.calls[0][1]
    assert args[offs_at + 1] == 2
    assert list((ctypes.c_int64 * 3).from_address(args[offs_at].value)) == [0, 5, 9]
    check()                                                                  # flag word 0: nothing to report
    rec.ws[:8].view(torch.int64)[0] = 6 + 1
    with pytest.raises(ValueError) as e:
        check()
    assert "idx[6] = 42 " in str(e.value) and f"[0, {N})" in str(e.value) and noun in str(e.value)
    if idx_optional:
        check = run(ops, None, [0, 5, 9])
        assert len(rec.calls) == 2 and rec.calls[1][1][offs_at - 1].value is None
        check()
        rec.ws[:8].view(torch.int64)[0] = 6 + 1
        with pytest.raises(ValueError, match=r"idx\[6\] = 6 .*group rows"):
            check()
