"""Timing probe of the classifier-output scores on one GPU (HIP events, warm, alternating calls, the median; one process), at
100 000 x 527 and 100 000 x 1000 float32 logits:

  groups   am_class_groups_f32 with 10 splits (buffers made once) beside the torch float64 composition of the same ten values
           (lp = x.double().log_softmax(1); p = lp.exp(); per-split marginals and means) and beside a plain device copy of the
           same bytes, the bandwidth floor.  Bar: the call <= 1.0 x the composition in the same run.  The fraction of the
           copy's bandwidth is printed without a bar.
  pairs    am_row_pairs_f32 in the kl_softmax mode beside F.kl_div on float64 log-softmaxes, and in the cosine mode beside
           F.cosine_similarity(...).double(); the same bar.

    python tools/class_scores_probe.py          (writes profiles/class_scores/probe.txt)
"""
import argparse
import ctypes
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_metrics_amd as am                                          # noqa: E402
from audio_metrics_amd import hip_ops as ops                            # noqa: E402
from audio_metrics_amd.metrics.classifier import split_offsets          # noqa: E402

DEV = torch.device("cuda", 0)


def rows(seed, n, c):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randn((n, c), generator=g, device=DEV) * 2.0


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


def verdict(ours, theirs):
    return "met" if ours <= theirs else f"MISSED by {100.0 * (ours / theirs - 1.0):.0f} %"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=11, help="timed calls per function; the median is printed")
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--splits", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_scores", "probe.txt"))
    args = ap.parse_args()
    lib = am._lib.load()
    lines = [f"# {torch.cuda.get_device_name(0)}; HIP events, warm, median of {args.calls} alternating calls; float32 randn x 2 logits"]
    n, nb_splits = args.rows, args.splits
    null = ctypes.c_void_p(None)

    def say(line):
        lines.append(line)
        print(line, flush=True)

    for c in (527, 1000):
        x, y = ops.as_matrix(rows(1, n, c)), ops.as_matrix(rows(2, n, c))
        offs = split_offsets(n, nb_splits)
        host_offs = (ctypes.c_int64 * len(offs))(*offs)
        rec = torch.empty((nb_splits, 4), dtype=torch.float64, device=DEV)
        nb = lib.am_class_groups_workspace_bytes(n, nb_splits, c)
        ws = ops._workspace(nb, DEV)
        copy_dst = torch.empty_like(x)

        def run_groups():
            ops._call(lib, "am_class_groups_f32", DEV, ops._ptr(x), n, ops._ld(x), c, null, ctypes.cast(host_offs, ctypes.c_void_p), nb_splits,
                      ops._ptr(rec), null, ops._ptr(ws), nb)

        def torch_groups():
            lp = x.double().log_softmax(1)
            p = lp.exp()
            h = (p * lp).sum(1)
            out = []
            for a, b in zip(offs, offs[1:]):
                pbar = p[a:b].mean(0)
                out.append(h[a:b].mean() - (pbar * pbar.clamp_min(1e-300).log()).sum())
            return torch.stack(out)

        def run_copy():
            copy_dst.copy_(x)
        (t_g, lo_g, hi_g), (t_t, lo_t, hi_t), (t_c, lo_c, hi_c) = alternate((run_groups, torch_groups, run_copy), args.calls)
        run_groups()
        diff = float((rec[:, 2] - torch_groups()).abs().max())
        say(f"groups {n} x {c}, {nb_splits} splits: am_class_groups_f32 {t_g:8.3f} ms ({lo_g:.3f} .. {hi_g:.3f})  torch f64 composition "
            f"{t_t:8.3f} ms ({lo_t:.3f} .. {hi_t:.3f})  ratio {t_g / t_t:5.3f} (bar <= 1.0: {verdict(t_g, t_t)})  device copy of the same bytes "
            f"{t_c:8.3f} ms ({lo_c:.3f} .. {hi_c:.3f}): {4.0 * n * c / t_g / 1e6:.0f} GB/s read, {100.0 * t_c / t_g / 2.0:.0f} % of the copy's bandwidth (its read + write)  "
            f"largest |log IS - torch| {diff:.2e}  workspace {nb / 2 ** 20:.1f} MiB")
        sums = torch.empty(4, dtype=torch.float64, device=DEV)
        nbp = lib.am_row_pairs_workspace_bytes(n)
        wsp = ops._workspace(nbp, DEV)

        def run_pairs(mode):
            ops._call(lib, "am_row_pairs_f32", DEV, ops._ptr(y), ops._ld(y), ops._ptr(x), ops._ld(x), n, c, ops.PAIR_MODES[mode], 0.0, null,
                      ops._ptr(sums), ops._ptr(wsp), nbp)

        def torch_kl():
            return F.kl_div(y.double().log_softmax(1), x.double().log_softmax(1), reduction="none", log_target=True).sum(1).mean()

        def torch_cos():
            return F.cosine_similarity(y, x, dim=1).double().mean()
        for mode, theirs, name in (("kl_softmax", torch_kl, "F.kl_div on f64 log-softmaxes"), ("cosine", torch_cos, "F.cosine_similarity(...).double()")):
            (t_p, lo_p, hi_p), (t_o, lo_o, hi_o) = alternate((lambda: run_pairs(mode), theirs), args.calls)
            run_pairs(mode)
            diff = abs(float(sums[0] / sums[2]) - float(theirs()))
            say(f"pairs {n} x {c}, {mode}: am_row_pairs_f32 {t_p:8.3f} ms ({lo_p:.3f} .. {hi_p:.3f})  {name} {t_o:8.3f} ms ({lo_o:.3f} .. {hi_o:.3f})  "
                f"ratio {t_p / t_o:5.3f} (bar <= 1.0: {verdict(t_p, t_o)})  {8.0 * n * c / t_p / 1e6:.0f} GB/s over the two matrices  "
                f"|mean - torch| {diff:.2e}")
        del x, y, ws, copy_dst
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
