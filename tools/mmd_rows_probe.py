"""Timing probe of the two-sided row sums on one GPU (HIP events, warm): am_mmd_rbf_rows_f32 with all three blocks on
100 000 x 100 000 randn rows at 512 and at 128 columns, beside - in the same run, on the same library -
  * the two am_mmd_rbf_groups_f32 calls with one group each (x against Y, then y against X) that yield the same four vectors
    by one-sided row sums: the XY block twice, XX and YY as full squares;
  * am_mmd_rbf_f32 with all three blocks: the same Gram work with a scalar epilogue, i.e. the floor;
and the XX | XY blocks alone for a 1 000-row candidate set against the 100 000-row reference (the reference's row sums
cached).  The bar: the new call takes at most 0.75 x the two group calls at both widths.

Each width is one step: a child process of its own under its own time limit; the first step that fails ends the run.

    python tools/mmd_rows_probe.py > profiles/mmd_rows/probe.txt
"""
import argparse
import os
import subprocess
import sys

BAR = 0.75


def step(args, d):
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from audio_metrics_amd import hip_ops as ops

    dev = torch.device("cuda", 0)

    def rows(seed, n):
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        return torch.randn((n, d), generator=g, device=dev)

    def timed(fn):
        fn()                                                            # warm
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.reps, out

    n = args.rows
    gamma = 0.5 / (2.0 * d)                                             # fixed: E d2 = 2 d for standard normal rows
    x, y, small = rows(2, n), rows(1, n), rows(3, args.small)
    print(f"# {torch.cuda.get_device_name(0)}; {n} x {n} x {d} randn, gamma = 0.5 / (2 d); events, warm, mean of {args.reps}")
    t_rows, (out_x, out_y) = timed(lambda: ops.mmd_rbf_row_sums(x, y, gamma=gamma))
    print(f"am_mmd_rbf_rows_f32, XX | YY | XY: {t_rows:9.2f} ms")

    def two_group_calls():
        a = ops.mmd_rbf_group_sums(x, None, [0, n], y, gamma=gamma, rows=True)
        b = ops.mmd_rbf_group_sums(y, None, [0, n], x, gamma=gamma, rows=True)
        return a, b
    t_groups, (ga, gb) = timed(two_group_calls)
    ga[-1]()
    gb[-1]()
    ratio = t_rows / t_groups
    print(f"two am_mmd_rbf_groups_f32 calls of one group each (the same four vectors): {t_groups:9.2f} ms; "
          f"ratio {ratio:.3f} (bar {BAR}: {'met' if ratio <= BAR else 'MISSED'})")
    worst = max(float(((out_x - ga[1]).abs().max(0).values / torch.tensor([n - 1.0, n], device=dev, dtype=torch.float64)).max()),
                float(((out_y - gb[1]).abs().max(0).values / torch.tensor([n - 1.0, n], device=dev, dtype=torch.float64)).max()))
    print(f"  largest |difference| of a normalised row sum between the two: {worst:.3e}")
    t_sums, sums = timed(lambda: ops.mmd_rbf_sums(x, y, gamma=gamma))
    print(f"am_mmd_rbf_f32, XX | YY | XY (the same Gram work, three scalars): {t_sums:9.2f} ms; the row sums take {t_rows / t_sums:.3f} x that")
    totals = torch.stack([out_x[:, 0].sum(), out_y[:, 0].sum(), out_x[:, 1].sum()])
    print(f"  largest relative difference of the three totals: {float(((totals - sums).abs() / sums.abs()).max()):.3e}")
    t_small, _ = timed(lambda: ops.mmd_rbf_row_sums(small, y, gamma=gamma, blocks=ops.MMD_XX | ops.MMD_XY))
    t_small_sums, _ = timed(lambda: ops.mmd_rbf_sums(small, y, gamma=gamma, blocks=ops.MMD_XX | ops.MMD_XY))
    print(f"am_mmd_rbf_rows_f32, XX | XY, {args.small} candidate rows against the {n}: {t_small:9.2f} ms "
          f"(am_mmd_rbf_f32 with the same blocks: {t_small_sums:.2f} ms)")
    return 0 if ratio <= BAR else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--small", type=int, default=1_000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds a step may take")
    ap.add_argument("--one", type=int, default=0, help="(internal) run the step of this width in this process")
    args = ap.parse_args()
    if args.one:
        return step(args, args.one)
    missed = False
    for d in (512, 128):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", str(d), "--rows", str(args.rows), "--small", str(args.small),
               "--reps", str(args.reps)]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"# the step at {d} columns ran into its limit of {args.limit} s; nothing further is started", flush=True)
            return 124
        if rc == 3:
            missed = True
        elif rc != 0:
            print(f"# the step at {d} columns ended with status {rc}; nothing further is started", flush=True)
            return rc
    return 3 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
