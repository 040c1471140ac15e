"""Timing probe of the per-group kernel audio distance on one GPU (HIP events, warm): am_mmd_rbf_groups_f32 on 100 000
candidate rows in 2 000 groups of 50 against a cached 100 000-row reference, beside the whole-set cross pass
am_mmd_rbf_f32(blocks = AM_MMD_XY) on the same two sets - the same Gram work with a scalar epilogue, i.e. the floor - and a
loop of kernel_audio_distance over the first 20 groups, from which the cost of 2 000 such calls is EXTRAPOLATED.

    python tools/kad_groups_probe.py > profiles/kad_groups/probe.txt
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audio_metrics_amd as am                                          # noqa: E402
from audio_metrics_amd import hip_ops as ops                            # noqa: E402

DEV = torch.device("cuda", 0)


def rows(seed, n, d, shift):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    x = torch.randn((n, d), generator=g, device=DEV) + shift
    return x / x.norm(dim=1, keepdim=True)                              # CLAP-like: offset Gaussian, unit norm


def timed(fn, reps):
    fn()                                                                # warm
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, out


def data_of(x):
    s = am.AudioMetricsData(True, device=DEV)
    s.add(x)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--per-group", type=int, default=50)
    ap.add_argument("--loop-groups", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    n, per = args.rows, args.per_group
    b = n // per
    print(f"# {torch.cuda.get_device_name(0)}; events, warm, mean of {args.reps}")
    for d in (512, 128):
        y, x = rows(1, n, d, 0.5), rows(2, n, d, 0.55)
        bw2 = ops.pairwise_select_sq(y)
        offs = list(range(0, n + 1, per))
        perm = torch.randperm(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
        t_xy, _ = timed(lambda: ops.mmd_rbf_sums(x, y, bw2=bw2, blocks=ops.MMD_XY), args.reps)
        print(f"whole-set cross pass am_mmd_rbf_f32(AM_MMD_XY) {n} x {n} x {d}: {t_xy:9.2f} ms  (the floor: the same Gram work, one scalar)")
        for name, idx, want_rows in (("stored order, no index list", None, False), ("random permutation as index list", perm, False),
                                     ("random permutation, out_rows   ", perm, True)):
            t, res = timed(lambda: ops.mmd_rbf_group_sums(x, idx, offs, y, bw2=bw2, rows=want_rows), args.reps)
            res[-1]()
            print(f"am_mmd_rbf_groups_f32 {n} x {d} in {b} groups of {per}, {name}: {t:9.2f} ms  = {t / t_xy:.3f} x the cross pass")
        # where a difference goes: the cross pass alone (one group: the within range is the whole list, so not comparable) is
        # not separable from outside; the small-group within pass is, by giving every row its own group (no within pairs at
        # all, yet the same tiles are visited and masked)
        singles = list(range(n + 1))
        t_1, _ = timed(lambda: ops.mmd_rbf_group_sums(x, None, singles, y, bw2=bw2)[0], args.reps)
        print(f"am_mmd_rbf_groups_f32 {n} x {d} in {n} groups of 1 (diagonal tiles only in the within pass): {t_1:9.2f} ms")
        ref, labels = data_of(y), torch.arange(n, device=DEV) // per
        cand = data_of(x)
        am.kernel_audio_distance_per_group(cand, ref, labels)           # fills the reference-side cache
        t_pg, out = timed(lambda: am.kernel_audio_distance_per_group(cand, ref, labels), args.reps)
        print(f"kernel_audio_distance_per_group, cached reference, {b} groups: {t_pg:9.2f} ms  (sort of the labels, two read-backs, "
              f"combination on the host included); kad of group 0 {out['kad_per_group'][0]:.6f}, median {np.median(out['kad_per_group']):.6f}")
        sets = [data_of(x[g * per:(g + 1) * per]) for g in range(args.loop_groups)]
        t_loop, vals = timed(lambda: [am.kernel_audio_distance(s, ref)["kad"] for s in sets], args.reps)
        print(f"loop of kernel_audio_distance over the first {args.loop_groups} groups: {t_loop:9.2f} ms = {t_loop / args.loop_groups:.3f} ms per group; "
              f"EXTRAPOLATED to {b} groups: {t_loop / args.loop_groups * b:9.1f} ms ({t_loop / args.loop_groups * b / t_pg:.1f} x the one call)")
        print(f"  largest |difference| of the {args.loop_groups} values to the one call: "
              f"{float(np.max(np.abs(np.asarray(vals) - out['kad_per_group'][:args.loop_groups]))):.3e}")
        del ref, cand, sets, x, y


if __name__ == "__main__":
    main()
