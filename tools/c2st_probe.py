"""Timing probe of the classifier two-sample test on one GPU (HIP events, warm, alternating calls, the median):

  pass      one am_logit_pass_f32 call (K = 5 models, every row trains four of them) beside the cheapest honest torch
            composition on the same inputs in the same run, in float32:
                z = x @ a.T + b;  t = s z;  r = -s sigmoid(-t) masked;  g = r.T @ x;  r.sum(0);  softplus(-t) masked .sum(0)
            - which reads x twice and writes and reads three N x K intermediates; the bar is library call <= composition
  copy      a device copy of x, and the bytes of x per second the pass achieves against it (the pass reads x twice, the
            second time from L2 where the block still is)
  whole     the wall time of one classifier_two_sample_test at 100 000 + 100 000 rows, with its pass count

    python tools/c2st_probe.py            # writes profiles/c2st/probe.txt
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
SHAPES = ((100_000, 512), (100_000, 128))
K = 5


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(functions, calls):
    """Median (and range) per call of several functions timed call by call, taking turns."""
    for _ in range(2):
        for fn in functions:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in functions]
    for _ in range(calls):
        for t, fn in zip(times, functions):
            t.append(event_ms(fn))
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in times]


def rows_of(seed, n, d, shift):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    mix = torch.eye(d, device=DEV) + 0.3 / d ** 0.5 * torch.randn((d, d), generator=g, device=DEV)
    return torch.randn((n, d), generator=g, device=DEV) @ mix + shift * torch.randn(d, generator=g, device=DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=11, help="timed calls per function; the median is printed")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "c2st"))
    ap.add_argument("--no-whole", action="store_true", help="the pass only: skip the whole test at 100 000 + 100 000 rows")
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    lib = am._lib.load()
    lines = [f"# {torch.cuda.get_device_name(0)}; HIP events, warm, median of {args.calls} alternating calls, one process"]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    for n, d in SHAPES:
        x = ops.as_rows(rows_of(1, n, d, 0.3))
        g = torch.Generator(device=DEV)
        g.manual_seed(3)
        fold = torch.randint(0, K, (n,), generator=g, device=DEV, dtype=torch.int32)
        coef = torch.randn((K, d + 1), generator=g, device=DEV, dtype=torch.float64) / d ** 0.5
        sums = torch.empty((K, d + 2), dtype=torch.float64, device=DEV)
        counts = torch.empty(2, dtype=torch.float64, device=DEV)
        nb = lib.am_logit_pass_workspace_bytes(n, d, K)
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
        a32, b32 = coef[:, :d].float().contiguous(), coef[:, d].float().contiguous()
        trains = fold[:, None] != torch.arange(K, device=DEV, dtype=torch.int32)[None, :]
        spare = torch.empty_like(x)

        def library():
            ops._call(lib, "am_logit_pass_f32", DEV, ops._ptr(x), n, ops._ld(x), d, ops._ptr(fold), 1, ops._ptr(coef), K, ops._ptr(sums),
                      None, ops._ptr(counts), ops._ptr(ws), nb)

        def composition():
            t = torch.addmm(b32, x, a32.T)                              # s = +1
            r = torch.where(trains, -torch.sigmoid(-t), 0.0)
            return r.T @ x, r.sum(0), torch.where(trains, torch.nn.functional.softplus(-t), 0.0).sum(0)

        def copy():
            spare.copy_(x)

        (t_k, lo_k, hi_k), (t_c, lo_c, hi_c), (t_m, lo_m, hi_m) = alternate((library, composition, copy), args.calls)
        g_lib, g_torch = sums[:, :d].float(), composition()[0]
        agree = float((g_lib - g_torch).abs().max() / g_torch.abs().max())
        ratio = t_k / t_c
        nbytes = x.numel() * 4
        say(f"pass   {n} x {d}, K = {K}: am_logit_pass_f32 {t_k:8.3f} ms ({lo_k:.3f} .. {hi_k:.3f})  torch composition (float32) "
            f"{t_c:8.3f} ms ({lo_c:.3f} .. {hi_c:.3f})  ratio {ratio:.3f}  bar 1.00: {'MET' if ratio <= 1.0 else 'MISSED'}  "
            f"(gradients agree to {agree:.1e} of their largest)")
        say(f"copy   {n} x {d}: device copy of x {t_m:8.3f} ms ({lo_m:.3f} .. {hi_m:.3f}) = {2 * nbytes / t_m / 1e9:.2f} TB/s read + "
            f"written; the pass moves the bytes of x at {nbytes / t_k / 1e9:.2f} TB/s, {t_k / t_m:.2f} x the copy's time")
        if args.no_whole:
            continue
        cand, ref = am.AudioMetricsData(True), am.AudioMetricsData(True)
        cand.add(x)
        ref.add(rows_of(2, n, d, 0.0))
        for attempt in range(2):                                        # the second call is the warm one
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = am.classifier_two_sample_test(cand, ref)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
        say(f"whole  classifier_two_sample_test {n} + {n} x {d}, 5 folds: {wall:9.1f} ms wall, {out['c2st_passes']} passes "
            f"(+ 1 for the logits), converged {int(out['c2st_converged'].sum())} of 5, accuracy {out['c2st_accuracy']:.4f}, "
            f"holdout {out['c2st_accuracy_holdout']:.4f}, z {out['c2st_z']:.2f}, p {out['c2st_p_value']:.3g}")
    with open(os.path.join(args.out_dir, "probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
