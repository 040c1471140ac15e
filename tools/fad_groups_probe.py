"""Timing probe of the per-group Frechet distance on one GPU (HIP events, warm): the dual-form call on 100 000 float32 rows
in 2 000 groups of 50, the front end on the same rows with labels, and - beside it - the composition of the entry points
that existed before it (stats_gather + frechet_batch: a D x D covariance and a Newton-Schulz solve per group) on as many
of the same groups as one solver workspace of hip_ops.FRECHET_BATCH_WS_CAP bytes holds.  Per-group times for both.

    python tools/fad_groups_probe.py > profiles/fad_groups/probe.txt
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audio_metrics_amd as am                                          # noqa: E402
from audio_metrics_amd import hip_ops as ops                            # noqa: E402
from audio_metrics_amd.metrics import fad                               # noqa: E402

DEV = torch.device("cuda", 0)
F64_MFMA_PEAK = 78.6e12                                                 # flop/s, dense f64 matrix cores of one MI355X


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=2_000)
    ap.add_argument("--per-group", type=int, default=50)
    ap.add_argument("--ref-rows", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--widths", type=int, nargs="+", default=[512, 128])
    args = ap.parse_args()
    b, per = args.groups, args.per_group
    n = b * per
    lib = am._lib.load()
    print(f"# {torch.cuda.get_device_name(0)}; events, warm, mean of {args.reps} (the composition of the older entry points: 1 run)")
    for d in args.widths:
        x = rows(2, n, d, 0.55)
        ref = am.AudioMetricsData(False, device=DEV)
        ref.add(rows(1, args.ref_rows, d, 0.5))
        mu_y, cov_y = ref.mean.reshape(-1), ref.cov
        offs = (np.arange(b + 1) * per).tolist()
        ws = lib.am_frechet_groups_workspace_bytes(n, b, d)

        def dual():
            out, check = ops.frechet_groups(x, None, offs, mu_y, cov_y)
            rec = out.cpu()
            check()
            return rec
        t, rec = timed(dual, args.reps)
        gemm_flop = 2.0 * n * d * d
        print(f"frechet_groups        {n} x {d} in {b} groups of {per}: {t:9.2f} ms = {1e3 * t / b:8.2f} us per group; workspace "
              f"{ws / 2 ** 20:.0f} MiB; Z = Xc cov_y alone is {gemm_flop:.2e} flop = {gemm_flop / F64_MFMA_PEAK * 1e3:.2f} ms at the f64 matrix "
              f"peak; sweeps {int(rec[:, 2].min())} .. {int(rec[:, 2].max())}, stop codes {sorted(set(rec[:, 4].int().tolist()))}, "
              f"mean fd {rec[:, 0].mean().item():.6f}")
        cand = am.AudioMetricsData(True, device=DEV)
        cand.embeddings = x
        labels = torch.arange(n, device=DEV) // per
        t, res = timed(lambda: am.frechet_distance_per_group(cand, ref, labels), args.reps)
        print(f"frechet_distance_per_group, same rows with labels:       {t:9.2f} ms = {1e3 * t / b:8.2f} us per group; "
              f"mean fd {res['fad_per_group'].mean():.6f}")
        # the older entry points: as many of the same groups as ONE batched solve may hold
        per_set = int(lib.am_frechet_batch_workspace_bytes(1, d))
        nb = max(1, min(b, ops.FRECHET_BATCH_WS_CAP // per_set))
        idx = torch.arange(nb * per, device=DEV)

        def composed():
            means, covs, check = ops.stats_gather(x, idx, offs[:nb + 1], defer_check=True)
            res = ops.frechet_batch(means, covs, mu_y, cov_y, fad.NS_MAX_ITER, fad.NS_TOL)
            check()
            return res
        t_c, res_c = timed(composed, 1)
        fds = np.array([r["fd"] for r in res_c])
        print(f"stats_gather + frechet_batch, the first {nb} groups (covariances {nb * d * d * 8 / 2 ** 20:.0f} MiB, solver workspace "
              f"{nb * per_set / 2 ** 20:.0f} MiB): {t_c:9.2f} ms = {1e3 * t_c / nb:8.2f} us per group; iterations "
              f"{min(r['iters'] for r in res_c)} .. {max(r['iters'] for r in res_c)}; max |fd - dual fd| "
              f"{np.abs(fds - rec[:nb, 0].numpy()).max():.3e} (mean fd {fds.mean():.6f})")
        del x, cand, ref


if __name__ == "__main__":
    main()
