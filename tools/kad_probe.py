"""Timing probe of the kernel-audio-distance path on one GPU (HIP events, warm): the pairwise select, the three kernel sums,
kernel_audio_distance against a cached reference, and - at a size torch.pdist can hold - a torch composition of the same
metric for comparison of time and value.

    python tools/kad_probe.py > profiles/kad/probe.txt
    python tools/kad_probe.py --f64 > profiles/kad_f64/probe.txt      (the three float64 entry points at 100 000 x 64 float64
                                                                       rows beside the f32 ones on the same values narrowed)
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
F32_MFMA_PEAK = 157.3e12                                                # flop/s, dense f32 matrix cores of one MI355X
F64_MFMA_PEAK = 78.6e12                                                 # flop/s, f64 matrix cores (v_mfma_f64_16x16x4_f64)


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


def torch_kad(x, y, block=4096):
    """pdist + median + blocked cdist / exp in float32 (sums in float64)."""
    bw2 = torch.median(torch.pdist(y)) ** 2
    how = "pdist"
    full = torch.cdist(y, y)                                            # cross-check: the same median from the cdist upper triangle
    iu = torch.triu_indices(y.shape[0], y.shape[0], 1, device=DEV)
    check = torch.median(full[iu[0], iu[1]]) ** 2
    del full, iu
    if not bool(torch.isfinite(bw2)) or abs(float(bw2) - float(check)) > 1e-3 * float(check):
        how = f"torch.pdist gave a median distance of {float(bw2) ** 0.5:.6f}, which its own cdist contradicts: cdist upper triangle used"
        bw2 = check
    g = 0.5 / bw2

    def ksum(a, b):
        total = torch.zeros((), dtype=torch.float64, device=DEV)
        for i in range(0, a.shape[0], block):
            total += torch.exp(-torch.cdist(a[i:i + block], b) ** 2 * g).sum(dtype=torch.float64)
        return total
    n, m = x.shape[0], y.shape[0]
    mmd2 = (ksum(x, x) - n) / (n * (n - 1.0)) + (ksum(y, y) - m) / (m * (m - 1.0)) - 2.0 * ksum(x, y) / (float(n) * m)
    return mmd2, bw2, how


def probe_f64(n, d, groups, reps):
    """The three float64 entry points beside the f32 ones on the same values narrowed: select, the three sums, and the
    per-group sums of `groups` equal groups.  No time is a pass / fail condition."""
    y64, x64 = rows(1, n, d, 0.5).double(), rows(2, n, d, 0.55).double()
    y64, x64 = y64 / y64.norm(dim=1, keepdim=True), x64 / x64.norm(dim=1, keepdim=True)
    y32, x32 = y64.float(), x64.float()
    half, full = n * (n - 1) / 2 * 2 * d, 2.0 * n * n * d
    offs = [n * b // groups for b in range(groups + 1)]
    for kind, x, y, peak in (("f64", x64, y64, F64_MFMA_PEAK), ("f32", x32, y32, F32_MFMA_PEAK)):
        t, bw2 = timed(lambda: ops.pairwise_select_sq(y), reps)
        print(f"{kind} select        {n} x {d}: {t:9.2f} ms  ({100 * 3 * half / peak / (t * 1e-3):.0f} % of the {kind} matrix peak over 3 passes); "
              f"median d2 {bw2.item():.9f}")
        for name, blocks, flop in (("sums YY", ops.MMD_YY, half), ("sums XY", ops.MMD_XY, full), ("sums all", 7, 2 * half + full)):
            t, out = timed(lambda: ops.mmd_rbf_sums(x, y, bw2=bw2, blocks=blocks), reps)
            print(f"{kind} {name:13s} {n} x {d}: {t:9.2f} ms  ({100 * flop / peak / (t * 1e-3):.0f} % of the {kind} matrix peak)  "
                  f"{[float(v) for v in out.cpu()]}")
        t, res = timed(lambda: ops.mmd_rbf_group_sums(x, None, offs, y, bw2=bw2), reps)
        res[-1]()
        print(f"{kind} group sums    {n} x {d} in {groups} groups: {t:9.2f} ms  ({100 * full / peak / (t * 1e-3):.0f} % of the {kind} matrix peak, "
              f"cross pass alone); sum Sxy {float(res[0][:, 1].sum()):.9e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--f64", action="store_true", help="time the float64 entry points at --rows x 64 beside the f32 ones")
    ap.add_argument("--groups", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--small", type=int, default=1_000)
    ap.add_argument("--torch-rows", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}; events, warm, mean of {args.reps}")
    if args.f64:
        probe_f64(args.rows, 64, args.groups, args.reps)
        return
    for d in (512, 128):
        n = args.rows
        y, x, xs = rows(1, n, d, 0.5), rows(2, n, d, 0.55), rows(3, args.small, d, 0.55)
        pass_flop = n * (n - 1) / 2 * 2 * d
        t_sel, bw2 = timed(lambda: ops.pairwise_select_sq(y), args.reps)
        print(f"select         {n} x {d}: {t_sel:9.2f} ms  = 3 passes; half Gram {pass_flop:.2e} flop per pass -> "
              f"{3 * pass_flop / F32_MFMA_PEAK * 1e3:.1f} ms at the f32 matrix peak ({100 * 3 * pass_flop / F32_MFMA_PEAK / (t_sel * 1e-3):.0f} % of it); "
              f"median d2 {bw2.item():.6f}")
        for name, blocks, flop in (("sums YY", ops.MMD_YY, pass_flop), ("sums XX", ops.MMD_XX, pass_flop), ("sums XY", ops.MMD_XY, 2.0 * n * n * d),
                                   ("sums all", 7, 2 * pass_flop + 2.0 * n * n * d)):
            t, _ = timed(lambda: ops.mmd_rbf_sums(x, y, bw2=bw2, blocks=blocks), args.reps)
            print(f"{name:14s} {n} x {d}: {t:9.2f} ms  ({100 * flop / F32_MFMA_PEAK / (t * 1e-3):.0f} % of the f32 matrix peak)")
        # YY does the select pass's Gram work with the exp epilogue instead of the histogram: (select / 3) - what YY would take
        # without its epilogue is not measurable from outside; the pair (select / 3, sums YY) bounds the two epilogues
        ref = data_of(y)
        for cand, label in ((x, n), (xs, args.small)):
            c = data_of(cand)
            am.kernel_audio_distance(c, ref)                                # fills the reference-side cache
            t, out = timed(lambda: am.kernel_audio_distance(c, ref), args.reps)
            print(f"kad, cached reference {n} x {d} vs {label} candidates: {t:9.2f} ms  kad {out['kad']:.6f} bandwidth {out['kad_bandwidth']:.6f}")
        del ref, x, y, xs
    n, d = args.torch_rows, 512
    y, x = rows(1, n, d, 0.5), rows(2, n, d, 0.55)
    t_t, (mmd_t, bw2_t, how) = timed(lambda: torch_kad(x, y), 1)
    t_o, out = timed(lambda: am.kernel_audio_distance(data_of(x), data_of(y)), 1)     # fresh sets: nothing cached
    print(f"torch pdist + median + blocked cdist / exp, {n} x {d}: {t_t:9.2f} ms  mmd2 {mmd_t.item():.9e} bandwidth {bw2_t.sqrt().item():.7f} ({how})")
    print(f"kernel_audio_distance, nothing cached,      {n} x {d}: {t_o:9.2f} ms  mmd2 {out['kad_mmd2']:.9e} bandwidth {out['kad_bandwidth']:.7f}")


if __name__ == "__main__":
    main()
