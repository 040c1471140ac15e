"""Timing probe of the sliced Wasserstein distance on one GPU (HIP events, warm, alternating calls, the median; one process):

  sort      am_sort_rows_f32 on a [128, rows] matrix beside torch.sort(z, dim=1).values on the same matrix; the bar is
            sort <= 1.0 x torch.sort in the same run (README, "Sliced Wasserstein distance")
  project   am_sliced_project_f32 beside x @ theta.T (torch, f32) at the same shape, for scale
  merge     am_sliced_w_f32 on two sorted [128, rows] matrices, with its achieved GB/s over their bytes
  call      a whole sliced_wasserstein_distance (L = 512) without and with the cached reference, and with 1 000 candidate
            rows against the cached reference: wall time around a device synchronise

    python tools/swd_probe.py          (writes profiles/swd/probe.txt)
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


def wall_ms(fn, calls=3):
    times = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return sorted(times)[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=11, help="timed calls per function; the median is printed")
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--chunk", type=int, default=128)
    ap.add_argument("--projections", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swd", "probe.txt"))
    args = ap.parse_args()
    lib = am._lib.load()
    lines = [f"# {torch.cuda.get_device_name(0)}; HIP events, warm, median of {args.calls} alternating calls; randn rows"]
    n, nl = args.rows, args.chunk

    def say(line):
        lines.append(line)
        print(line, flush=True)

    for d in (512, 128):
        x, y = rows(1, n, d), rows(2, n, d, 0.1)
        theta = torch.as_tensor(am.sliced_directions(d, nl, 0)).to(DEV)
        z = ops.sliced_project(x, theta)
        # ---- sort: the library call with its buffers made once, beside torch.sort on the same matrix
        out = torch.empty_like(z)
        nb = lib.am_sort_rows_workspace_bytes(nl, n)
        ws = ops._workspace(nb, DEV)

        def run_sort():
            ops._call(lib, "am_sort_rows_f32", DEV, ops._ptr(z), nl, n, n, ops._ptr(out), n, ops._ptr(ws), nb)

        def run_torch_sort():
            torch.sort(z, dim=1).values
        (t_s, lo_s, hi_s), (t_t, lo_t, hi_t) = alternate((run_sort, run_torch_sort), args.calls)
        same = bool(torch.equal(out, torch.sort(z, dim=1).values))
        verdict = "met" if t_s <= t_t else f"MISSED by {100.0 * (t_s / t_t - 1.0):.0f} %"
        say(f"sort [{nl}, {n}] (projections of {d} columns): am_sort_rows_f32 {t_s:8.3f} ms ({lo_s:.3f} .. {hi_s:.3f})  torch.sort(dim=1).values "
            f"{t_t:8.3f} ms ({lo_t:.3f} .. {hi_t:.3f})  ratio {t_s / t_t:5.3f} (bar <= 1.0: {verdict})  equal to torch's order: {same}  "
            f"workspace {nb / 2 ** 20:.1f} MiB")
        # ---- projection, for scale
        zz = torch.empty_like(z)

        def run_project():
            ops._call(lib, "am_sliced_project_f32", DEV, ops._ptr(x), n, ops._ld(x), ops._ptr(theta), nl, ops._ld(theta), d, ops._ptr(zz), n)

        def run_matmul():
            torch.matmul(x, theta.T)
        (t_p, lo_p, hi_p), (t_m, lo_m, hi_m) = alternate((run_project, run_matmul), args.calls)
        say(f"project {n} x {nl} x {d}: am_sliced_project_f32 {t_p:8.3f} ms ({lo_p:.3f} .. {hi_p:.3f})  x @ theta.T (torch, f32) {t_m:8.3f} ms "
            f"({lo_m:.3f} .. {hi_m:.3f})  {2.0 * n * nl * d / t_p / 1e9:.1f} TFLOP/s, {(4.0 * n * d + 4.0 * nl * n) / t_p / 1e6:.0f} GB/s over X and Z")
        # ---- merge
        zy = ops.sort_rows(ops.sliced_project(y, theta))
        w = torch.empty(nl, dtype=torch.float64, device=DEV)
        bad = torch.empty(nl, dtype=torch.int32, device=DEV)
        nbw = lib.am_sliced_w_workspace_bytes(nl, n, n)
        wsw = ops._workspace(nbw, DEV)

        def run_w():
            ops._call(lib, "am_sliced_w_f32", DEV, ops._ptr(out), n, n, ops._ptr(zy), n, n, nl, 2, ops._ptr(w), ops._ptr(bad), ops._ptr(wsw), nbw)
        ((t_w, lo_w, hi_w),) = alternate((run_w,), args.calls)
        say(f"merge [{nl}, {n}] x 2, p = 2: am_sliced_w_f32 {t_w:8.3f} ms ({lo_w:.3f} .. {hi_w:.3f})  {8.0 * nl * n / t_w / 1e6:.0f} GB/s over the two "
            f"sorted matrices")
        del z, out, zz, zy, ws
        # ---- the whole call
        sx, sy, small = am.AudioMetricsData(True), am.AudioMetricsData(True), am.AudioMetricsData(True)
        sx.add(x)
        sy.add(y)
        small.add(x[:1000])
        kw = dict(n_projections=args.projections, p=2, seed=0, chunk_projections=args.chunk)
        got = am.sliced_wasserstein_distance(sx, sy, cache_reference=False, **kw)                 # warm
        t_un = wall_ms(lambda: am.sliced_wasserstein_distance(sx, sy, cache_reference=False, **kw))
        am.sliced_wasserstein_distance(sx, sy, **kw)                                                # fills the cache
        t_ca = wall_ms(lambda: am.sliced_wasserstein_distance(sx, sy, **kw))
        am.sliced_wasserstein_distance(small, sy, **kw)
        t_sm = wall_ms(lambda: am.sliced_wasserstein_distance(small, sy, **kw))
        say(f"sliced_wasserstein_distance {n} x {n} x {d}, L = {args.projections}, chunks of {args.chunk}: {t_un:9.2f} ms wall (median of 3, "
            f"reference not cached), {t_ca:9.2f} ms with the reference's sorted projections cached, {t_sm:9.2f} ms for 1000 candidate rows "
            f"against the cached reference; swd {got['swd']:.6f} +- {got['swd_std_error']:.6f}, D swd^2 {d * got['swd'] ** 2:.4f}")
        del sx, sy, small, x, y
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
