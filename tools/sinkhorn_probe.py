"""Timing probe of the soft-min and the Sinkhorn divergence on one GPU (HIP events, warm, alternating calls, the median):

  softmin   one am_softmin_f32 call beside am_kmeans_assign_f32 (the hard-min form of the same sweep) and
            am_mmd_rbf_f32(AM_MMD_XY) (the same epilogue without the running maximum) on the same two matrices; the bar is
            softmin <= 1.25 x the MMD pass in the same run ("Sinkhorn divergence")
  solve     a whole sinkhorn_divergence at 10 000 x 10 000 x 512, with the step counts

    python tools/sinkhorn_probe.py          (writes profiles/sinkhorn/probe.txt)
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_metrics_amd as am                                          # noqa: E402
from audio_metrics_amd import hip_ops as ops                            # noqa: E402

DEV = torch.device("cuda", 0)


def rows(seed, n, d, shift=0.0):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randn((n, d), generator=g, device=DEV) + shift


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(fns, calls):
    """Median (and range) per call of the functions, timed call by call, alternating."""
    for _ in range(2):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(calls):
        for t, fn in zip(times, fns):
            t.append(event_ms(fn))
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=11, help="timed calls per function; the median is printed")
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--solve-rows", type=int, default=10_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sinkhorn", "probe.txt"))
    args = ap.parse_args()
    lib = am._lib.load()
    lines = [f"# {torch.cuda.get_device_name(0)}; HIP events, warm, median of {args.calls} alternating calls; randn rows"]
    n = m = args.rows
    for d in (512, 128):
        x, y = rows(1, n, d), rows(2, m, d, 0.1)
        eps = float(d)                                                  # of the order of the costs
        g = torch.randn(m, dtype=torch.float64, device=DEV)
        out = torch.empty(n, dtype=torch.float64, device=DEV)
        stats = torch.empty(2, dtype=torch.float64, device=DEV)
        nb_s = lib.am_softmin_workspace_bytes(n, m, d)
        ws_s = ops._workspace(nb_s, DEV)
        labels = torch.empty(n, dtype=torch.int64, device=DEV)
        d2 = torch.empty(n, dtype=torch.float32, device=DEV)
        inertia = torch.empty((), dtype=torch.float64, device=DEV)
        nb_a = lib.am_kmeans_assign_workspace_bytes(n, m, d)
        ws_a = ops._workspace(nb_a, DEV)

        def run_softmin():
            ops._call(lib, "am_softmin_f32", DEV, ops._ptr(x), n, ops._ld(x), ops._ptr(y), m, ops._ld(y), d, ops._ptr(g), eps, None,
                      0.0, ops._ptr(out), ops._ptr(stats), ops._ptr(ws_s), nb_s)

        def run_assign():
            ops._call(lib, "am_kmeans_assign_f32", DEV, ops._ptr(x), n, ops._ld(x), ops._ptr(y), m, ops._ld(y), d, ops._ptr(labels),
                      ops._ptr(d2), ops._ptr(inertia), ops._ptr(ws_a), nb_a)

        def run_mmd():
            ops.mmd_rbf_sums(x, y, gamma=0.5 / eps, blocks=ops.MMD_XY)
        (t_s, lo_s, hi_s), (t_a, lo_a, hi_a), (t_m, lo_m, hi_m) = alternate((run_softmin, run_assign, run_mmd), args.calls)
        lines.append(f"{n} x {m} x {d}: am_softmin_f32 {t_s:9.3f} ms ({lo_s:.3f} .. {hi_s:.3f})  am_kmeans_assign_f32 {t_a:9.3f} ms "
                     f"({lo_a:.3f} .. {hi_a:.3f})  am_mmd_rbf_f32(AM_MMD_XY) {t_m:9.3f} ms ({lo_m:.3f} .. {hi_m:.3f})  softmin / mmd "
                     f"{t_s / t_m:5.3f} (bar <= 1.25)  softmin / assign {t_s / t_a:5.3f}  workspace {nb_s / 2 ** 20:.1f} MiB")
        print(lines[-1], flush=True)
        del x, y, ws_s, ws_a
    n = m = args.solve_rows
    d = 512
    sx, sy = am.AudioMetricsData(True), am.AudioMetricsData(True)
    sx.add(rows(3, n, d))
    sy.add(rows(4, m, d, 0.1))
    am.sinkhorn_divergence(sx, sy)                                      # warm: the median, the first launches
    times = []
    for _ in range(3):
        ref = am.AudioMetricsData(True)                                 # a fresh reference: nothing cached
        ref.add(sy.embeddings)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = am.sinkhorn_divergence(sx, ref, blur=got_blur(sx, sy))
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    cached = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        am.sinkhorn_divergence(sx, ref, blur=got["sinkhorn_blur"])
        torch.cuda.synchronize()
        cached.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"sinkhorn_divergence {n} x {m} x {d}, default blur {got['sinkhorn_blur']:.4f}: {sorted(times)[1]:9.2f} ms wall (median of 3, "
                 f"reference not cached), {sorted(cached)[1]:9.2f} ms with the reference's solve cached; steps (XY, XX, YY) "
                 f"{got['sinkhorn_iterations']}, converged {got['sinkhorn_converged']}, S {got['sinkhorn_divergence']:.6f}, "
                 f"marginal error {got['sinkhorn_marginal_error']:.3e}")
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def got_blur(sx, sy):
    """The default blur of the warm call, as a number: the timed calls then skip nothing but the median's read-back."""
    import math
    return 0.25 * math.sqrt(float(ops.pairwise_select_sq(sy.embeddings)))


if __name__ == "__main__":
    main()
