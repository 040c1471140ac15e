"""Timing and accuracy probe of the pair-dependence sweep on one GPU (HIP events, warm, 11 alternating calls, the median):

  dual      am_pair_dependence_f32 (distance kind) at 100 000 paired rows, 512 / 512 and 512 / 128 wide, beside the SUM of two
            am_mmd_multi_f32 energy-kernel calls, XY block, of X against X and of Y against Y as two distinct sets, in the same
            run: the same MFMA work and the same count of f64 square roots.  The bar is dual <= 1.25 x that sum (the margin the
            soft-min was given over its kernel-sum pass: a simpler schedule than the early-commit pipeline)
  kinds     the Gaussian and Laplacian kinds at the same shapes (two exp per pair more)
  accuracy  the largest error of the five row sums and their totals against the float64 oracle (tests/dependence_reference.py)
            as a share of MARGIN x the emulated error, at the real-valued sets of tests/test_gpu_dependence.py

    python tools/dependence_probe.py            # writes profiles/dependence/probe.txt and profiles/dependence/accuracy.txt
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import audio_metrics_amd as am                                          # noqa: E402,F401
from audio_metrics_amd import hip_ops as ops                            # noqa: E402

DEV = torch.device("cuda", 0)
BAR = 1.25
CALLS = 11
SHAPES = ((100_000, 512, 512), (100_000, 512, 128))


def randn_rows(seed, n, d):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randn((n, d), generator=g, device=DEV)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(fa, fb, calls=CALLS):
    """Median (and range) per call of two functions timed call by call, alternating."""
    fa()
    fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(calls):
        ta.append(event_ms(fa))
        tb.append(event_ms(fb))
    med = lambda t: sorted(t)[len(t) // 2]                              # noqa: E731
    return med(ta), (min(ta), max(ta)), med(tb), (min(tb), max(tb))


def timing(lines, shapes):
    for n, dx, dy in shapes:
        x, y = randn_rows(1, n, dx), randn_rows(2, n, dy)
        x2, y2 = x.clone(), y.clone()                                   # two distinct sets: the XY block sweeps the full square
        dual = lambda: ops.pair_dependence(x, y, "energy")              # noqa: E731

        def two_sums():
            ops.mmd_multi_sums(x, x2, "energy", (1.0,), blocks=ops.MMD_XY)
            ops.mmd_multi_sums(y, y2, "energy", (1.0,), blocks=ops.MMD_XY)
        td, rd, ts, rs = alternate(dual, two_sums)
        ratio = td / ts
        flop = 2.0 * n * n * (dx + dy)
        lines.append(f"{n} x {dx} / {dy}: dual pass {td:.2f} ms ({rd[0]:.2f} .. {rd[1]:.2f}; {flop / td / 1e9:.1f} Tflop/s), two energy XY "
                     f"passes {ts:.2f} ms ({rs[0]:.2f} .. {rs[1]:.2f}): ratio {ratio:.3f}, bar {BAR} {'met' if ratio <= BAR else 'MISSED'}")
        print(lines[-1], flush=True)
        bwx, bwy = 2.0 * dx, 2.0 * dy
        for kind in ("gaussian", "laplacian"):
            fk = lambda: ops.pair_dependence(x, y, kind, bw2x=bwx, bw2y=bwy)     # noqa: E731
            fk()
            torch.cuda.synchronize()
            t = sorted(event_ms(fk) for _ in range(5))[2]
            lines.append(f"{n} x {dx} / {dy}: {kind} {t:.2f} ms ({t / td:.3f} x the distance kind)")
            print(lines[-1], flush=True)
        nb = am._lib.load().am_pair_dependence_workspace_bytes(n, dx, dy)
        lines.append(f"{n} x {dx} / {dy}: workspace {nb / 1e6:.1f} MB")
        del x, y, x2, y2
        torch.cuda.empty_cache()


def accuracy(lines):
    import dependence_reference as dr
    import inputs as gi
    import kd_reference as kr
    for rows, seed, d in (("randn", 864, 64), ("unit", 1312, 512)):
        y, x = gi.pair(rows, seed, 1000, 1000, d)
        xt, yt = torch.as_tensor(x).to(DEV), torch.as_tensor(y).to(DEV)
        bwx, bwy = float(np.median(dr.ka.pair_values(x))), float(np.median(dr.ka.pair_values(y)))
        for kind in dr.KINDS:
            got_rows, got_sums = (t.cpu().numpy() for t in ops.pair_dependence(xt, yt, kind, bw2x=bwx, bw2y=bwy))
            want = dr.row_sums(dr.pair_matrix(x, kind, bwx), dr.pair_matrix(y, kind, bwy))
            emu = dr.row_sums(dr.pair_matrix(x, kind, bwx, kr.emulated_dots("f32")), dr.pair_matrix(y, kind, bwy, kr.emulated_dots("f32")))
            scale = np.abs(want).mean(0)
            limit = kr.MARGIN * float((np.abs(emu - want).max(0) / scale).max())
            share = float((np.abs(got_rows - want).max(0) / scale).max()) / limit
            tot = float((np.abs(got_sums[:5] - want.sum(0)) / np.abs(want.sum(0))).max())
            lines.append(f"{rows} D={d} {kind}: row sums {share * kr.MARGIN:.2f} of the {kr.MARGIN:.0f} allowed (limit {limit:.3e} of "
                         f"mean |value|), totals relative error {tot:.3e}")
            print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dependence"))
    ap.add_argument("--rows", type=int, default=0, help="time at this many rows instead of 100 000 (a quick look)")
    ap.add_argument("--only", choices=("timing", "accuracy"), help="write one of the two files only")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    shapes = tuple((args.rows or n, dx, dy) for n, dx, dy in SHAPES)
    head = [f"device: {torch.cuda.get_device_name(0)}; HIP events, warm, median of {CALLS} alternating calls"]
    if args.only != "accuracy":
        lines = list(head)
        timing(lines, shapes)
        with open(os.path.join(args.out, "probe.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    if args.only != "timing":
        lines = [f"device: {torch.cuda.get_device_name(0)}"]
        accuracy(lines)
        with open(os.path.join(args.out, "accuracy.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
