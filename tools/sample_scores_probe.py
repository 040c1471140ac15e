"""Timing probe of the per-sample scores on one GPU (HIP events, warm, alternating calls, the median):

  scores   am_sample_scores_f32 beside am_kmeans_assign_f32 on the same two matrices - the same Gram sweep with a one-key
           epilogue; the bar is the ratio of the two in the same run ("Per-sample realism and rarity")
  torch    a blocked torch.cdist composition of the same three reductions at 20 000 x 20 000 (the N x M matrix does not
           fit above that), for scale only: its distances have other bits

    python tools/sample_scores_probe.py > profiles/sample_scores/probe.txt
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audio_metrics_amd as am                                          # noqa: E402
from audio_metrics_amd import hip_ops as ops                            # noqa: E402

DEV = torch.device("cuda", 0)
F32_MFMA_PEAK = 157.3e12                                                # flop/s, dense f32 matrix cores of one MI355X


def rows(seed, n, d):
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


def torch_scores(x, y, r, block=4096):
    n = x.shape[0]
    realism = torch.empty(n, device=DEV)
    count = torch.empty(n, dtype=torch.int64, device=DEV)
    rarity = torch.empty(n, device=DEV)
    for s in range(0, n, block):
        dist = torch.cdist(x[s:s + block], y)
        inside = dist < r[None, :]
        realism[s:s + block] = (r[None, :] / dist).max(dim=1).values
        count[s:s + block] = inside.sum(dim=1)
        rarity[s:s + block] = torch.where(inside, r[None, :], torch.inf).min(dim=1).values
    return realism, count, torch.where(count > 0, rarity, 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=11, help="timed calls per function; the median is printed")
    ap.add_argument("--nearest-k", type=int, default=5)
    args = ap.parse_args()
    lib = am._lib.load()
    print(f"# {torch.cuda.get_device_name(0)}; HIP events, warm, median of {args.calls} alternating calls; randn rows, "
          f"radii = knn_radii({args.nearest_k})")
    for n, m, d in ((100_000, 100_000, 512), (100_000, 100_000, 128), (1_000, 100_000, 512), (1_000, 100_000, 128)):
        x, y = rows(1, n, d), rows(2, m, d)
        r = ops.knn_radii(y, args.nearest_k)
        out = [torch.empty(n, dtype=t, device=DEV) for t in (torch.float32, torch.int64, torch.int32, torch.float32, torch.int64)]
        nb_s = lib.am_sample_scores_workspace_bytes(n, m, d)
        ws_s = ops._workspace(nb_s, DEV)
        labels = torch.empty(n, dtype=torch.int64, device=DEV)
        d2 = torch.empty(n, dtype=torch.float32, device=DEV)
        inertia = torch.empty((), dtype=torch.float64, device=DEV)
        nb_a = lib.am_kmeans_assign_workspace_bytes(n, m, d)
        ws_a = ops._workspace(nb_a, DEV)

        def run_scores():
            ops._call(lib, "am_sample_scores_f32", DEV, ops._ptr(x), n, ops._ld(x), ops._ptr(y), m, ops._ld(y), d, ops._ptr(r),
                      *(ops._ptr(t) for t in out), ops._ptr(ws_s), nb_s)

        def run_assign():
            ops._call(lib, "am_kmeans_assign_f32", DEV, ops._ptr(x), n, ops._ld(x), ops._ptr(y), m, ops._ld(y), d, ops._ptr(labels),
                      ops._ptr(d2), ops._ptr(inertia), ops._ptr(ws_a), nb_a)
        t_a, r_a, t_s, r_s = alternate(run_assign, run_scores, args.calls)
        flop = 2.0 * n * m * d
        inside = float((out[2] > 0).double().mean())
        print(f"{n} x {m} x {d}: assign {t_a:9.3f} ms ({r_a[0]:.3f} .. {r_a[1]:.3f})  sample_scores {t_s:9.3f} ms "
              f"({r_s[0]:.3f} .. {r_s[1]:.3f})  ratio {t_s / t_a:5.2f} (target <= 1.5)  scores at "
              f"{100 * flop / F32_MFMA_PEAK / (t_s * 1e-3):.0f} % of the f32 matrix peak, {lib.am_sample_scores_chunks(n, m, d)} column "
              f"chunks, workspace {nb_s / 2 ** 20:.1f} MiB; {100 * inside:.2f} % of the samples in the manifold, median realism "
              f"{float(out[0].median()):.4f}")
        del x, y, ws_s, ws_a
    for d in (512, 128):
        n = m = 20_000
        x, y = rows(3, n, d), rows(4, m, d)
        r = ops.knn_radii(y, args.nearest_k)
        keep = {}

        def run_ours():
            keep["ours"] = ops.sample_scores(x, y, r)

        def run_torch():
            keep["torch"] = torch_scores(x, y, r)
        t_o, r_o, t_t, r_t = alternate(run_ours, run_torch, args.calls)
        same_count = float((keep["ours"][2].to(torch.int64) == keep["torch"][1]).double().mean())
        err = float(((keep["ours"][0] - keep["torch"][0]).abs() / keep["torch"][0]).max())
        print(f"{n} x {m} x {d}: sample_scores {t_o:9.3f} ms ({r_o[0]:.3f} .. {r_o[1]:.3f})  blocked cdist composition {t_t:9.3f} ms "
              f"({r_t[0]:.3f} .. {r_t[1]:.3f})  ratio {t_o / t_t:5.2f}  (scale only: cdist's d2 has other bits - counts agree on "
              f"{100 * same_count:.3f} % of the rows, largest relative difference of the realism {err:.2e})")


if __name__ == "__main__":
    main()
