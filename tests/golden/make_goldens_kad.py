"""Recorder of the two fixtures that pin the Kernel Audio Distance family (kad.hip, kad_f64.hip, kad_groups.hip, mmd_multi.hip,
mmd_rows.hip) to what an earlier library computed - what a refactor of these files is held to:

    kad_workspace.json   every am_*_workspace_bytes of the family on a grid of shapes (needs no GPU).  A plan or chunk rule that
                         drifts changes a size here - and the summation order, hence the bits, on the device.
    kad_bits.npz         the outputs of the family's calls on an MI355X, bit for bit.  Inputs come from a seed
                         (kd_reference.rbf_rows); only outputs are stored.

Run it against the library to record from, with the unchanged Python:
    AM_HIP_LIBRARY=/abs/path/libaudio_metrics_hip.so python tests/golden/make_goldens_kad.py workspace
    AM_HIP_LIBRARY=/abs/path/libaudio_metrics_hip.so python tests/golden/make_goldens_kad.py bits        (on the GPU)
(a second argument names another output file.)  The tests (tests/test_kad_workspace_cpu.py,
tests/test_gpu_kad_recorded_bits.py) import the case lists below and never run it."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

WORKSPACE_JSON = os.path.join(HERE, "kad_workspace.json")
BITS_NPZ = os.path.join(HERE, "kad_bits.npz")

# ---------------------------------------------------------------------------------------------------- workspace sizes
SIZES = (1, 2, 127, 128, 129, 1_000, 20_000, 300_000)       # every ordered pair (N1, N2): both orders
WIDTHS = (1, 64, 100)
MASKS = tuple(range(1, 8))
NSCALES = (1, 2, 3, 4)
GROUP_COUNTS = (1, 7, 1_000)


def workspace_queries():
    """(query name, argument tuples) in a fixed order: the select, rbf, multi, rows and groups queries of f32, the three of f64"""
    one = [(n, d) for n in SIZES for d in WIDTHS]
    two = [(n1, n2, d, m) for n1 in SIZES for n2 in SIZES for d in WIDTHS for m in MASKS]
    multi = [(n1, n2, d, k, m) for n1 in SIZES for n2 in SIZES for d in WIDTHS for k in NSCALES for m in MASKS]
    groups = [(nt, b, n2, d) for nt in SIZES for b in GROUP_COUNTS for n2 in SIZES for d in WIDTHS]
    return (("am_pairwise_select_workspace_bytes", one), ("am_mmd_rbf_workspace_bytes", two), ("am_mmd_multi_workspace_bytes", multi),
            ("am_mmd_rbf_rows_workspace_bytes", two), ("am_mmd_rbf_groups_workspace_bytes", groups),
            ("am_pairwise_select_f64_workspace_bytes", one), ("am_mmd_rbf_f64_workspace_bytes", two),
            ("am_mmd_rbf_groups_f64_workspace_bytes", groups))


def workspace_sizes(lib):
    return {name: [int(getattr(lib, name)(*a)) for a in args] for name, args in workspace_queries()}


# ---------------------------------------------------------------------------------------------------- recorded bits
# (set, N1, N2, D, float64 rows).  Small: three (f32, 128-row) / five (f64, 64-row) tiles - the diagonal, off-diagonal weight 2
# and padded rows; D = 64 and 72 take the two inner-dimension-tail instantiations.  Chunked: 92 and 93 tile rows, so
# tiles / 2048 >= 2: two Q tiles per workgroup and empty chunks past the diagonal - where the slot layout and the reduce
# kernel's strided order matter; the rows call sweeps two bands there.
SHAPES = (("small64", 300, 257, 64, False), ("small72", 300, 257, 72, False), ("small64_f64", 300, 257, 64, True),
          ("small72_f64", 300, 257, 72, True), ("chunked", 11_700, 640, 32, False), ("chunked_f64", 5_900, 320, 32, True))
GAMMA = 1.0 / 200.0                                          # rbf_rows(sigma = 10): squared distances of the order of 200
GROUP_HEAD = (1, 2, 127, 129)                                # then the rest: a group straddles a tile edge, a P tile holds several


def inputs(case):
    import kd_reference as kr
    name, n1, n2, d, f64 = case
    rng = np.random.default_rng(20_250 + [c[0] for c in SHAPES].index(name))
    x, y = kr.rbf_rows(rng, n1, d, 10.0), kr.rbf_rows(rng, n2, d, 10.0)
    perm = rng.permutation(n1).astype(np.int64)
    if f64:
        x, y = x.astype(np.float64), y.astype(np.float64)
    return x, y, perm


def bits_of(case, ops, torch, device="cuda"):
    """{key: float64 host tensor} of every call recorded for one case"""
    name, n1, n2, d, f64 = case
    small = name.startswith("small")
    xh, yh, perm = inputs(case)
    x, y = torch.as_tensor(xh, device=device), torch.as_tensor(yh, device=device)
    out = {}

    def put(key, t):
        out[name + "__" + key] = t.detach().to("cpu", torch.float64).contiguous()
    bw2 = ops.pairwise_select_sq(y)
    put("select_median_y", bw2)
    put("select_median_x", ops.pairwise_select_sq(x))
    put("select_rank_x", ops.pairwise_select_sq(x, rank=n1 + 12_345))
    for mask in (7, 5, 2) if small else (7,):
        put("rbf_gamma_m%d" % mask, ops.mmd_rbf_sums(x, y, gamma=GAMMA, blocks=mask))
        put("rbf_bw2_m%d" % mask, ops.mmd_rbf_sums(x, y, bw2=bw2, blocks=mask))
    put("rbf_gamma0", ops.mmd_rbf_sums(x, y, gamma=0.0))
    if not f64:
        families = (("gaussian", (0.5, 1.0, 2.0, 4.0)), ("laplacian", (0.5, 2.0)), ("energy", (1.0,)))
        for kernel, scales in families if small else families[:1]:
            put("multi_%s_host" % kernel, ops.mmd_multi_sums(x, y, kernel, scales, bw2=None if kernel == "energy" else 200.0))
            if kernel != "energy":
                put("multi_%s_dev" % kernel, ops.mmd_multi_sums(x, y, kernel, scales, bw2=bw2))
        for mask in (7, 3) if small else (7,):
            ox, oy = ops.mmd_rbf_row_sums(x, y, gamma=GAMMA, blocks=mask)
            put("rows_m%d_x" % mask, ox)
            put("rows_m%d_y" % mask, oy)
    head = sum(GROUP_HEAD)
    offsets = np.concatenate([[0], np.cumsum(GROUP_HEAD + (n1 - head,))]).tolist()
    for tag, idx in (("list", torch.as_tensor(perm, device=device)), ("stored", None)):
        groups, rows, check = ops.mmd_rbf_group_sums(x, idx, offsets, y, bw2=bw2, rows=True)
        check()
        put("groups_%s" % tag, groups)
        put("groups_%s_rows" % tag, rows)
    return out


def main(what, dest=None):
    import audio_metrics_amd as am
    if what == "workspace":
        sizes = workspace_sizes(am._lib.load())
        with open(dest or WORKSPACE_JSON, "w") as f:
            json.dump(sizes, f, separators=(",", ":"))
            f.write("\n")
        print("wrote", dest or WORKSPACE_JSON, sum(len(v) for v in sizes.values()), "sizes from", am._lib.library_path())
    elif what == "bits":
        import torch
        rec = {}
        for case in SHAPES:
            rec.update({k: v.numpy() for k, v in bits_of(case, am.hip_ops, torch).items()})
        np.savez_compressed(dest or BITS_NPZ, **rec)
        print("wrote", dest or BITS_NPZ, len(rec), "arrays from", am._lib.library_path())
    else:
        raise SystemExit("usage: make_goldens_kad.py workspace | bits [output file]")


if __name__ == "__main__":
    main(*sys.argv[1:3])
