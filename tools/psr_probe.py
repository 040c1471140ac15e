"""Timing and accuracy probe of the probabilistic scoring rule on one GPU (HIP events, warm, alternating calls, the median):

  sparse    am_psr_f32 beside am_sample_scores_f32 (radii of k = 5) on the same two matrices of latent rows (q = 8), radius
            a = 1.2, k = 4: in-range pairs are rare and the epilogue is a compare; the bar is psr <= 1.05 x sample_scores
  dense     am_psr_f32 beside am_mmd_rbf_f32(AM_MMD_XY) on the same two matrices of randn rows with a radius that puts every
            pair in range: the ungated path, one correctly rounded square root per pair; the bar is psr <= 1.25 x the MMD pass
  whole     one probabilistic_precision_recall at 100 000 x 100 000 x 512 with the k-NN radii cached
  accuracy  the largest error / bound of the per-row PSR against the float64 oracle (tests/psr_reference.py) at the shapes of
            tests/test_gpu_psr.py

    python tools/psr_probe.py            # writes profiles/psr/probe.txt and profiles/psr/accuracy.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import audio_metrics_amd as am                                          # noqa: E402
from audio_metrics_amd import hip_ops as ops                            # noqa: E402
import psr_reference as pr                                              # noqa: E402

DEV = torch.device("cuda", 0)
F32_MFMA_PEAK = 157.3e12                                                # flop/s, dense f32 matrix cores of one MI355X
K, A, Q = 4, 1.2, 8
SHAPES = ((100_000, 100_000, 512), (100_000, 100_000, 128), (1_000, 100_000, 512))
ACCURACY_SHAPES = ((130, 300, 40), (257, 130, 64), (130, 4000, 40), (1000, 130, 64), (300, 257, 40))


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


def alternate(fa, fb, calls):
    """Median (and range) per call of two functions timed call by call, alternating."""
    for _ in range(2):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(calls):
        ta.append(event_ms(fa))
        tb.append(event_ms(fb))
    med = lambda t: sorted(t)[len(t) // 2]                              # noqa: E731
    return med(ta), (min(ta), max(ta)), med(tb), (min(tb), max(tb))


def psr_call(lib, x, y, radius):
    n, d = x.shape
    m = y.shape[0]
    psr = torch.empty(n, dtype=torch.float64, device=DEV)
    count = torch.empty(n, dtype=torch.int32, device=DEV)
    sums = torch.empty(2, dtype=torch.float64, device=DEV)
    nb = lib.am_psr_workspace_bytes(n, m, d)
    ws = ops._workspace(nb, DEV)

    def run():
        ops._call(lib, "am_psr_f32", DEV, ops._ptr(x), n, ops._ld(x), ops._ptr(y), m, ops._ld(y), d, float(radius), ops._ptr(psr),
                  ops._ptr(count), ops._ptr(sums), ops._ptr(ws), nb)
    return run, psr, count, sums, nb, ws


def scores_call(lib, x, y, r):
    n, d = x.shape
    m = y.shape[0]
    out = [torch.empty(n, dtype=t, device=DEV) for t in (torch.float32, torch.int64, torch.int32, torch.float32, torch.int64)]
    nb = lib.am_sample_scores_workspace_bytes(n, m, d)
    ws = ops._workspace(nb, DEV)

    def run():
        ops._call(lib, "am_sample_scores_f32", DEV, ops._ptr(x), n, ops._ld(x), ops._ptr(y), m, ops._ld(y), d, ops._ptr(r),
                  *(ops._ptr(t) for t in out), ops._ptr(ws), nb)
    return run, out, ws


def mmd_call(lib, x, y, gamma):
    n, d = x.shape
    m = y.shape[0]
    sums = torch.empty(3, dtype=torch.float64, device=DEV)
    nb = lib.am_mmd_rbf_workspace_bytes(n, m, d, 4)
    ws = ops._workspace(nb, DEV)

    def run():
        ops._call(lib, "am_mmd_rbf_f32", DEV, ops._ptr(x), n, ops._ld(x), ops._ptr(y), m, ops._ld(y), d, None, float(gamma), 4,
                  ops._ptr(sums), ops._ptr(ws), nb)
    return run, sums, ws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=11, help="timed calls per function; the median is printed")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "psr"))
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    lib = am._lib.load()
    lines = [f"# {torch.cuda.get_device_name(0)}; HIP events, warm, median of {args.calls} alternating calls, one process"]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say(f"# sparse: latent rows (q = {Q}), radius = {A} * mean knn_radii(y, {K}); beside am_sample_scores_f32 with knn_radii(y, 5); bar <= 1.05")
    for n, m, d in SHAPES:
        x, y = torch.as_tensor(pr.latent_rows(n, d, Q, 1, 0.5)).to(DEV), torch.as_tensor(pr.latent_rows(m, d, Q, 2, 0.0)).to(DEV)
        radius = A * float(ops.knn_radii(y, K).to(torch.float64).mean())
        r5 = ops.knn_radii(y, 5)
        run_p, psr, count, sums, nb, ws_p = psr_call(lib, x, y, radius)
        run_s, out, ws_s = scores_call(lib, x, y, r5)
        t_s, r_s, t_p, r_p = alternate(run_s, run_p, args.calls)
        flop = 2.0 * n * m * d
        say(f"sparse {n} x {m} x {d}: sample_scores {t_s:9.3f} ms ({r_s[0]:.3f} .. {r_s[1]:.3f})  psr {t_p:9.3f} ms "
            f"({r_p[0]:.3f} .. {r_p[1]:.3f})  ratio {t_p / t_s:5.3f} (bar <= 1.05)  psr at "
            f"{100 * flop / F32_MFMA_PEAK / (t_p * 1e-3):.0f} % of the f32 matrix peak, {lib.am_psr_chunks(n, m, d)} column chunks, "
            f"workspace {nb / 2 ** 20:.1f} MiB; radius {radius:.4f}, mean count {float(sums[1]) / n:.2f} "
            f"({100 * float(sums[1]) / n / m:.4f} % of the pairs), mean psr {float(sums[0]) / n:.4f}")
        del x, y, ws_p, ws_s
    say("# dense: randn rows, radius = 2 * the largest distance scale (every pair in range); beside am_mmd_rbf_f32(AM_MMD_XY); bar <= 1.25")
    for n, m, d in SHAPES:
        x, y = randn_rows(1, n, d), randn_rows(2, m, d)
        radius = 2.0 * float(np.sqrt(2.0 * d)) + 8.0                    # |x - y| ~ sqrt(2 D) +- a few: all of them below
        run_p, psr, count, sums, nb, ws_p = psr_call(lib, x, y, radius)
        run_m, msums, ws_m = mmd_call(lib, x, y, 0.5 / (2.0 * d))
        t_m, r_m, t_p, r_p = alternate(run_m, run_p, args.calls)
        flop = 2.0 * n * m * d
        say(f"dense  {n} x {m} x {d}: am_mmd_rbf_f32(AM_MMD_XY) {t_m:9.3f} ms ({r_m[0]:.3f} .. {r_m[1]:.3f})  psr {t_p:9.3f} ms "
            f"({r_p[0]:.3f} .. {r_p[1]:.3f})  ratio {t_p / t_m:5.3f} (bar <= 1.25)  psr at "
            f"{100 * flop / F32_MFMA_PEAK / (t_p * 1e-3):.0f} % of the f32 matrix peak; "
            f"{100 * float(sums[1]) / n / m:.2f} % of the pairs in range")
        del x, y, ws_p, ws_m
    n, m, d = SHAPES[0]
    cand, ref = am.AudioMetricsData(True), am.AudioMetricsData(True)
    cand.add(torch.as_tensor(pr.latent_rows(n, d, Q, 1, 0.5)).to(DEV))
    ref.add(torch.as_tensor(pr.latent_rows(m, d, Q, 2, 0.0)).to(DEV))
    cand.get_radii(K), ref.get_radii(K)
    torch.cuda.synchronize()
    first = time.perf_counter()
    res = am.probabilistic_precision_recall(cand, ref)
    first = time.perf_counter() - first
    walls = []
    for _ in range(5):
        t0 = time.perf_counter()
        res = am.probabilistic_precision_recall(cand, ref)
        walls.append(time.perf_counter() - t0)
    say(f"whole  probabilistic_precision_recall {n} x {m} x {d}, latent rows, k-NN radii cached: first call {1e3 * first:.1f} ms "
        f"(reduces the radii), then median {1e3 * sorted(walls)[2]:.1f} ms wall per call ({1e3 * min(walls):.1f} .. {1e3 * max(walls):.1f}); "
        f"p_precision {res['p_precision']:.4f} p_recall {res['p_recall']:.4f}")
    with open(os.path.join(args.out_dir, "probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")

    acc = [f"# {torch.cuda.get_device_name(0)}; per-row PSR of am_psr_f32 against the float64 oracle (tests/psr_reference.py): latent rows "
           f"(q = 3), radius = {A} * mean knn_radii(y, {K}); `dense` is randn 400 x 500 x 64"]
    for n, m, d in (*ACCURACY_SHAPES, (400, 500, 64)):
        dense = (n, m, d) == (400, 500, 64)
        if dense:
            x = np.random.default_rng(21).standard_normal((n, d)).astype(np.float32)
            y = np.random.default_rng(22).standard_normal((m, d)).astype(np.float32)
        else:
            x, y = pr.latent_pair(n, m, d)
        xt, yt = torch.as_tensor(x).to(DEV), torch.as_tensor(y).to(DEV)
        radius = A * float(ops.knn_radii(yt, K).to(torch.float64).mean())
        psr, count, _ = ops.psr_scores(xt, yt, radius)
        psr, count = psr.cpu().numpy(), count.cpu().numpy()
        want, _, dist = pr.psr_f64(x, y, radius)
        bound = pr.error_bound(x, y, dist, radius)
        err = np.abs(psr - want)
        acc.append(f"{'dense ' if dense else ''}{n} x {m} x {d}: radius {radius:.4f} mean psr {psr.mean():.4f} mean count {count.mean():.1f}  "
                   f"largest error {err.max():.3e}  bound median {np.median(bound):.3e} max {bound.max():.3e}  "
                   f"largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.4f}  "
                   f"|mean error| {abs(psr.mean() - want.mean()):.3e} (mean bound {bound.mean():.3e})")
        print(acc[-1], flush=True)
    with open(os.path.join(args.out_dir, "accuracy.txt"), "w") as f:
        f.write("\n".join(acc) + "\n")


if __name__ == "__main__":
    main()
