"""Timing probe of the k-means kernels on one GPU (HIP events, warm, alternating windows):

  assign   am_kmeans_assign_f32 beside am_knn_search_f32(k = 1) on the same operands - the same Gram sweep with lists of 8 keys
  update   am_kmeans_update_f32 (with its device sort) beside index_add_ + divide in torch
  kmeans   a full run beside a blocked cdist / argmin / index_add_ loop in torch, same start, same iteration count

    python tools/kmeans_probe.py > profiles/kmeans/probe.txt
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audio_metrics_amd as am                                          # noqa: E402
from audio_metrics_amd import hip_ops as ops                            # noqa: E402

DEV = torch.device("cuda", 0)
F32_MFMA_PEAK = 157.3e12                                                # flop/s, dense f32 matrix cores of one MI355X
HBM_RATE = 6.3e12                                                       # bytes/s a streaming kernel reaches


def rows(seed, n, d, shift):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    x = torch.randn((n, d), generator=g, device=DEV) + shift
    return x / x.norm(dim=1, keepdim=True)                              # CLAP-like: offset Gaussian, unit norm


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternate(fa, fb, rounds, min_ms):
    """Median (and range) per call of two functions timed in alternating windows of at least min_ms of the first."""
    fa()
    fb()
    torch.cuda.synchronize()
    reps = max(2, int(min_ms / max(event_ms(fa, 2), 1e-3)) + 1)
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(event_ms(fa, reps))
        tb.append(event_ms(fb, reps))
    med = lambda t: sorted(t)[len(t) // 2]                              # noqa: E731
    return med(ta), (min(ta), max(ta)), med(tb), (min(tb), max(tb)), reps


def torch_assign(x, c, block=8192):
    out = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    for s in range(0, x.shape[0], block):
        out[s:s + block] = torch.cdist(x[s:s + block], c).argmin(dim=1)
    return out


def torch_update(x, labels, c_old):
    k = c_old.shape[0]
    sums = torch.zeros((k, x.shape[1]), dtype=torch.float32, device=x.device).index_add_(0, labels, x)
    counts = torch.bincount(labels, minlength=k)
    return torch.where(counts[:, None] > 0, sums / counts.clamp_min(1)[:, None], c_old), counts


def torch_kmeans(x, c, iters):
    for _ in range(iters):
        labels = torch_assign(x, c)
        c, _ = torch_update(x, labels, c)
    return c, torch_assign(x, c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--rounds", type=int, default=3, help="alternating windows; the median is printed")
    ap.add_argument("--min-ms", type=float, default=200.0, help="least work per timed window")
    ap.add_argument("--iters", type=int, default=10, help="Lloyd iterations of the full run")
    args = ap.parse_args()
    lib = am._lib.load()
    print(f"# {torch.cuda.get_device_name(0)}; HIP events, warm, median of {args.rounds} alternating windows of >= {args.min_ms:.0f} ms")
    for d, k in ((512, 10_000), (128, 1_000)):
        n = args.rows
        x = rows(1, n, d, 0.5)
        gen = torch.Generator(device="cpu")
        gen.manual_seed(0)
        c = x[torch.randperm(n, generator=gen)[:k].to(DEV)].contiguous()
        print(f"## {n} x {d} rows, K = {k}")
        # ---- assign beside the k = 1 search
        dist = torch.empty((n, 1), dtype=torch.float32, device=DEV)
        idx = torch.empty((n, 1), dtype=torch.int64, device=DEV)
        nb_s = lib.am_knn_search_workspace_bytes(n, k, d, 1)
        ws_s = ops._workspace(nb_s, DEV)
        labels = torch.empty(n, dtype=torch.int64, device=DEV)
        d2 = torch.empty(n, dtype=torch.float32, device=DEV)
        inertia = torch.empty((), dtype=torch.float64, device=DEV)
        nb_a = lib.am_kmeans_assign_workspace_bytes(n, k, d)
        ws_a = ops._workspace(nb_a, DEV)

        def run_search():
            ops._call(lib, "am_knn_search_f32", DEV, ops._ptr(x), n, ops._ld(x), ops._ptr(c), k, ops._ld(c), d, 1, -1, 1,
                      ops._ptr(dist), ops._ptr(idx), ops._ptr(ws_s), nb_s)

        def run_assign():
            ops._call(lib, "am_kmeans_assign_f32", DEV, ops._ptr(x), n, ops._ld(x), ops._ptr(c), k, ops._ld(c), d, ops._ptr(labels),
                      ops._ptr(d2), ops._ptr(inertia), ops._ptr(ws_a), nb_a)
        t_s, r_s, t_a, r_a, reps = alternate(run_search, run_assign, args.rounds, args.min_ms)
        same = bool(torch.equal(labels, idx[:, 0]) and torch.equal(d2.view(torch.int32), dist[:, 0].view(torch.int32)))
        flop = 2.0 * n * k * d
        print(f"assign: search(k = 1) {t_s:8.3f} ms ({r_s[0]:.3f} .. {r_s[1]:.3f})  assign {t_a:8.3f} ms ({r_a[0]:.3f} .. {r_a[1]:.3f})  "
              f"ratio {t_a / t_s:5.2f}  assign at {100 * flop / F32_MFMA_PEAK / (t_a * 1e-3):.0f} % of the f32 matrix peak, "
              f"{lib.am_knn_search_chunks(n, k, d, 1)} column chunks, {reps} calls per window, same bits: {same}, "
              f"workspace {nb_a / 2 ** 20:.1f} MiB against {nb_s / 2 ** 20:.1f} MiB")
        # ---- update beside index_add_ + divide
        keep = {}

        def run_update():
            keep["ours"] = ops.kmeans_update(x, labels, c)

        def run_torch_update():
            keep["torch"] = torch_update(x, labels, c)
        t_u, r_u, t_t, r_t, reps = alternate(run_update, run_torch_update, args.rounds, args.min_ms)
        err = float((keep["ours"][0] - keep["torch"][0]).abs().max())
        byts = 4.0 * n * d
        print(f"update: kmeans_update (sort + kernels) {t_u:8.3f} ms ({r_u[0]:.3f} .. {r_u[1]:.3f})  index_add_ + divide {t_t:8.3f} ms "
              f"({r_t[0]:.3f} .. {r_t[1]:.3f})  ratio {t_u / t_t:5.2f}  one read of the rows at {HBM_RATE / 1e12:.1f} TB/s: "
              f"{1e3 * byts / HBM_RATE:.3f} ms, {reps} calls per window, largest difference {err:.2e}, counts equal: "
              f"{bool(torch.equal(keep['ours'][1], keep['torch'][1]))}")
        # ---- a full run beside the torch loop: same start, same number of iterations
        am.kmeans(x, k, max_iter=2, init=c)
        torch_kmeans(x, c, 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run = am.kmeans(x, k, max_iter=args.iters, init=c)
        torch.cuda.synchronize()
        t_ours = time.perf_counter() - t0
        assigns = len(run["inertia_history"])
        t0 = time.perf_counter()
        tc, tl = torch_kmeans(x, c, assigns - 1)
        torch.cuda.synchronize()
        t_torch = time.perf_counter() - t0
        agree = float((tl == run["labels"]).double().mean())
        print(f"kmeans: {assigns} assigns, {assigns - 1} updates: ours {1e3 * t_ours:9.1f} ms  "
              f"torch loop {1e3 * t_torch:9.1f} ms  ratio {t_ours / t_torch:5.2f}  inertia {run['inertia']:.6f}  "
              f"checksum of our centroids {float(run['centroids'].double().sum()):.6f}, of the loop's {float(tc.double().sum()):.6f}, "
              f"labels agree on {100 * agree:.3f} % of the rows (the loop rounds differently)")
        del x, c


if __name__ == "__main__":
    main()
