"""Timing probe of the unit-pair kernel sums on one GPU (HIP events, warm): am_mmd_rbf_cells_f32 with all three blocks on
100 000 x 100 000 randn rows at 512 and at 128 columns, beside - in the same run, on the same library -
  * am_mmd_rbf_rows_f32 with all three blocks: the nearest existing kernel (the same Gram and exp work, a butterfly per tile
    where the cell sums take one short tree);
  * am_mmd_rbf_f32 with all three blocks: the same Gram work with a scalar epilogue, i.e. the floor, and what ONE relabelling
    costs when it is recomputed - the figure for 1 000 relabellings is that time x 1 000, an EXTRAPOLATION, never run;
then the XX | XY blocks alone for a 1 000-row candidate set against the 100 000-row reference (the reference's matrix cached),
and the whole front end, kernel_audio_distance_permutation_test with 999 permutations, on host clocks around a synchronise.
The bar: the cells call takes at most 1.05 x the row-sum call of the same run at both widths (5 % for run-to-run noise).

Each width is one step: a child process of its own under its own time limit; the first step that fails ends the run.

    python tools/mmd_cells_probe.py > profiles/mmd_cells/probe.txt
"""
import argparse
import os
import subprocess
import sys
import time

BAR = 1.05


def step(args, d):
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import audio_metrics_amd as am
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
    t_cells, cells = timed(lambda: ops.mmd_rbf_cell_sums(x, y, gamma=gamma))
    print(f"am_mmd_rbf_cells_f32, XX | YY | XY ({cells[0].shape[0]} x {cells[1].shape[0]} cells): {t_cells:9.2f} ms")
    t_rows, (out_x, out_y) = timed(lambda: ops.mmd_rbf_row_sums(x, y, gamma=gamma))
    ratio = t_cells / t_rows
    print(f"am_mmd_rbf_rows_f32, XX | YY | XY (the nearest existing kernel): {t_rows:9.2f} ms; "
          f"ratio {ratio:.3f} (bar {BAR}: {'met' if ratio <= BAR else 'MISSED'})")
    t_sums, sums = timed(lambda: ops.mmd_rbf_sums(x, y, gamma=gamma))
    print(f"am_mmd_rbf_f32, XX | YY | XY (the same Gram work, three scalars): {t_sums:9.2f} ms; the cell sums take {t_cells / t_sums:.3f} x that")
    totals = torch.stack([c.sum() for c in cells])
    print(f"  largest relative difference of the three totals: {float(((totals - sums).abs() / sums.abs()).max()):.3e}")
    print(f"  1 000 relabellings recomputed through am_mmd_rbf_f32 (EXTRAPOLATED, 1 000 x the line above, not run): {t_sums:.0f} s")
    t_small, _ = timed(lambda: ops.mmd_rbf_cell_sums(small, y, gamma=gamma, blocks=ops.MMD_XX | ops.MMD_XY))
    print(f"am_mmd_rbf_cells_f32, XX | XY, {args.small} candidate rows against the {n}: {t_small:9.2f} ms")
    del cells, out_x, out_y

    def data(e):
        s = am.AudioMetricsData(True, device=dev)
        s.embeddings = e
        return s
    cand, ref = data(x), data(y)
    bw = (2.0 * d) ** 0.5
    for what in ("first call (YY computed)", "second call (YY cached)"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = am.kernel_audio_distance_permutation_test(cand, ref, n_permutations=999, seed=0, bandwidth=bw)
        torch.cuda.synchronize()
        print(f"kernel_audio_distance_permutation_test, 999 permutations, {res['kad_units']} units, {what}: "
              f"{(time.perf_counter() - t0) * 1e3:9.2f} ms host clock (p = {res['kad_p_value']:.3f})")
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
