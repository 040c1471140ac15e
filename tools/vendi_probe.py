"""Timing probe of the Vendi score on one GPU (HIP events, warm, median of 11 unless a step is slow enough to say otherwise):

  * the per-group kernel on 100 000 x 512 float32 rows in 2 000 groups of 50, cosine and Gaussian - and beside it, in the same
    run, the torch composition: gather, bmm in f64, batched torch.linalg.eigvalsh, entropy;
  * the moment route at 100 000 x 512 and 100 000 x 128, beside xh.T @ xh in f64 on normalised rows, each with am_eigh_sym_f64;
  * the Gram route at 2048 rows, which is what its cap costs.

    python tools/vendi_probe.py > profiles/vendi/probe.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audio_metrics_amd as am                                          # noqa: E402
from audio_metrics_amd import hip_ops as ops                            # noqa: E402

DEV = torch.device("cuda", 0)


def rows(seed, n, d, shift):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    x = torch.randn((n, d), generator=g, device=DEV) + shift
    return x / x.norm(dim=1, keepdim=True)                              # CLAP-like: offset Gaussian, unit norm


def timed(fn, reps, slow_s=1.5):
    """(median ms over reps, reps used, last result); a step whose warm run takes longer than slow_s gets 3 repetitions"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()                                                          # warm
    torch.cuda.synchronize()
    if time.perf_counter() - t0 > slow_s:
        reps = min(reps, 3)
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), reps, out


def torch_groups(x, idx, b, per, kernel, gamma):
    xg = x[idx].view(b, per, -1).to(torch.float64)                      # gather + convert
    g = torch.bmm(xg, xg.transpose(1, 2))
    diag = torch.diagonal(g, dim1=1, dim2=2)
    if kernel == "cosine":
        s = diag.sqrt()
        k = g / (s[:, :, None] * s[:, None, :])
    else:
        k = torch.exp(-gamma * ((diag[:, :, None] + diag[:, None, :]) - 2.0 * g).clamp_min(0.0))
    lam = torch.linalg.eigvalsh(k / per)
    lam = torch.where(lam > 4.0 * per * 2.0 ** -52 * lam[:, -1:], lam, torch.ones_like(lam))      # ln 1 = 0: dropped
    return torch.exp(-(lam * lam.log()).sum(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=2_000)
    ap.add_argument("--per-group", type=int, default=50)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--bandwidth", type=float, default=0.7)
    args = ap.parse_args()
    b, per, reps = args.groups, args.per_group, args.reps
    n = b * per
    gamma = 1.0 / (2.0 * args.bandwidth ** 2)
    print(f"# {torch.cuda.get_device_name(0)}; HIP events, warm, median of {reps} (a step slower than 1.5 s: of 3)")
    # ---- per group
    d = 512
    x = rows(2, n, d, 0.55)
    offs = (np.arange(b + 1) * per).tolist()
    idx = torch.arange(n, device=DEV)
    worst = 0.0
    for kernel in ("cosine", "gaussian"):
        kw = {"gamma": gamma} if kernel == "gaussian" else {}
        t, r, (rec, _, _) = timed(lambda: ops.vendi_groups(x, None, offs, kernel, **kw), reps)
        t_i, _, _ = timed(lambda: ops.vendi_groups(x, idx, offs, kernel, **kw), reps)
        t_t, r_t, ref = timed(lambda: torch_groups(x, idx, b, per, kernel, gamma), reps)
        rel = float((rec[:, 0] / ref - 1.0).abs().max())
        worst = max(worst, t / t_t)
        print(f"vendi_groups {kernel:8s} {n} x {d} float32 in {b} groups of {per}: {t:9.3f} ms = {1e3 * t / b:7.2f} us per group "
              f"(behind an index list {t_i:9.3f} ms; median of {r}); sweeps {int(rec[:, 4].min())} .. {int(rec[:, 4].max())}, stop codes "
              f"{sorted(set(rec[:, 6].int().tolist()))}, mean score {rec[:, 0].mean().item():.6f}")
        print(f"  torch: gather, bmm f64, batched eigvalsh, entropy:            {t_t:9.3f} ms = {1e3 * t_t / b:7.2f} us per group "
              f"(median of {r_t}); ratio ours / torch {t / t_t:.3f}; max relative difference of the scores {rel:.2e}")
    print(f"bar: at most 1.0 x the torch composition for the {b}-group case: worst ratio {worst:.3f} -> {'met' if worst <= 1.0 else 'MISSED'}")
    # ---- moment route
    for d in (512, 128):
        x = rows(3, n, d, 0.55)
        t_m, r, (s, _) = timed(lambda: ops.vendi_moment(x), reps)
        t_e, r_e, (lam, _) = timed(lambda: ops.eigh_descending(s), reps)

        def composed():
            xh = x.to(torch.float64)
            xh = xh / xh.norm(dim=1, keepdim=True)
            return xh.T @ xh / n
        t_c, r_c, s_ref = timed(composed, reps)
        t_v, r_v, res = timed(lambda: am.vendi_score(x, route="moment"), reps)
        print(f"vendi_moment {n} x {d} float32 ({ops.vendi_moment_chunks(n, d)} chunks): {t_m:9.3f} ms (median of {r}); xh.T @ xh in f64 on "
              f"normalised rows: {t_c:9.3f} ms (median of {r_c}); max |S - torch| {float((s - s_ref).abs().max()):.2e}; am_eigh_sym_f64 of "
              f"{d} x {d}: {t_e:9.3f} ms (median of {r_e}); vendi_score end to end {t_v:9.3f} ms (median of {r_v}), score {res['vendi']:.4f}, "
              f"rank {res['vendi_rank']}")
        del x
    # ---- Gram route at its cap
    m, d = ops.vendi_gram_max_rows(), 512
    x = rows(4, m, d, 0.55)
    for kernel in ("cosine", "gaussian"):
        kw = {"gamma": gamma} if kernel == "gaussian" else {}
        t_g, r, (mat, _) = timed(lambda: ops.vendi_gram(x, None, kernel, **kw), reps)
        t_e, r_e, _ = timed(lambda: ops.eigh_descending(mat), reps)
        t_v, r_v, res = timed(lambda: am.vendi_score(x, kernel=kernel, bandwidth=args.bandwidth if kernel == "gaussian" else None,
                                                     route="gram"), reps)
        print(f"vendi_gram {kernel:8s} {m} x {d} float32: {t_g:9.3f} ms (median of {r}); am_eigh_sym_f64 of {m} x {m}: {t_e:9.3f} ms "
              f"(median of {r_e}); vendi_score end to end {t_v:9.3f} ms (median of {r_v}), score {res['vendi']:.4f}, rank {res['vendi_rank']}")


if __name__ == "__main__":
    main()
