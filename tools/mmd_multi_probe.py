"""Timing probe of the multi-scale kernel sums on one GPU (HIP events, warm): one four-scale Gaussian call of
hip_ops.mmd_multi_sums beside four hip_ops.mmd_rbf_sums calls on the same sets - all three blocks, and the XY block alone -,
one four-scale Laplacian call and one energy call, at 100 000 x 512 and 100 000 x 128 float32 rows.

    python tools/mmd_multi_probe.py > profiles/mmd_multi/probe.txt

The bar: the four-scale call takes at most 0.75 x the total of the four single calls of the same run."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audio_metrics_amd import hip_ops as ops                            # noqa: E402

DEV = torch.device("cuda", 0)
F32_MFMA_PEAK = 157.3e12                                                # flop/s, dense f32 matrix cores of one MI355X
SCALES = (0.5, 1.0, 2.0, 4.0)
BAR = 0.75


def rows(seed, n, d, shift):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randn((n, d), generator=g, device=DEV) + shift


def timed(fn, reps):
    """(median ms over `reps` event-bracketed runs after one warm run, the last result)"""
    fn()                                                                # warm
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}; events, warm, median of {args.reps}; randn rows; scales {SCALES} x the median bandwidth")
    n = args.rows
    for d in (512, 128):
        y, x = rows(1, n, d, 0.0), rows(2, n, d, 0.05)
        bw2 = ops.pairwise_select_sq(y)
        bw2_v = float(bw2.item())
        half, full = n * (n - 1) / 2 * 2 * d, 2.0 * n * n * d
        print(f"{n} x {d}, median d2 {bw2_v:.4f}")
        for name, blocks, flop in (("all blocks", 7, 2 * half + full), ("XY alone", ops.MMD_XY, full)):
            t_multi, multi = timed(lambda: ops.mmd_multi_sums(x, y, "gaussian", SCALES, bw2=bw2, blocks=blocks), args.reps)
            singles, equal = [], True
            for j, c in enumerate(SCALES):
                t, one = timed(lambda: ops.mmd_rbf_sums(x, y, gamma=0.5 / (bw2_v * (c * c)), blocks=blocks), args.reps)
                singles.append(t)
                equal = equal and all(torch.equal(multi[b, j], one[b]) for b in range(3) if blocks & (1 << b))
            total = sum(singles)
            print(f"  gaussian, {name:10s}: four scales in one call {t_multi:8.2f} ms ({100 * flop / F32_MFMA_PEAK / (t_multi * 1e-3):.0f} % of the f32 "
                  f"matrix peak); four mmd_rbf_sums calls {total:8.2f} ms ({', '.join(f'{t:.2f}' for t in singles)}); ratio "
                  f"{t_multi / total:.3f} (bar {BAR}: {'met' if t_multi <= BAR * total else 'MISSED'}); same bits: {equal}")
        flop = 2 * half + full
        for kind, grid in (("gaussian", SCALES[:1]), ("gaussian", SCALES[:2]), ("gaussian", SCALES[:3]), ("laplacian", SCALES[:1]),
                           ("laplacian", SCALES), ("energy", (1.0,))):
            t, out = timed(lambda: ops.mmd_multi_sums(x, y, kind, grid, bw2=bw2), args.reps)
            print(f"  {kind + ',':10s} all blocks, {len(grid)} scale{'s' if len(grid) > 1 else ' '}: {t:8.2f} ms "
                  f"({100 * flop / F32_MFMA_PEAK / (t * 1e-3):.0f} % of the f32 matrix peak)  Sxy {[float(v) for v in out[2].cpu()]}")
        del x, y


if __name__ == "__main__":
    main()
