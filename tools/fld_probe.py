"""Timing probe of the feature likelihood sweeps on one GPU (HIP events, warm, alternating calls, the median):

  sweeps   one am_fld_loglik_f32 call (rows: training set, columns: centres) and one am_fld_grad_f32 call (the swapped sweep)
           beside am_softmin_f32 on the same two matrices in the same orientation; the bars are loglik <= 1.10 x and
           gradient <= 1.25 x the soft-min of the same run.  Inputs are randn rows after the default normalisation, theta
           comes from a short fit
  fit      the wall time of a whole feature_likelihood_fit (100 steps) at the same shapes

    python tools/fld_probe.py          (writes profiles/fld/probe.txt)
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
from audio_metrics_amd.metrics import fld                               # noqa: E402

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


def verdict(ratio, bar):
    return f"{ratio:5.3f} (bar <= {bar:.2f}: {'MET' if ratio <= bar else 'MISSED'})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=11, help="timed calls per function; the median is printed")
    ap.add_argument("--shapes", default="100000x100000x512,100000x100000x128,1000x100000x512",
                    help="comma-separated (generated rows) x (training rows) x D")
    ap.add_argument("--steps", type=int, default=100, help="steps of the timed fit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fld", "probe.txt"))
    args = ap.parse_args()
    lib = am._lib.load()
    lines = [f"# {torch.cuda.get_device_name(0)}; HIP events, warm, median of {args.calls} alternating calls; randn rows after the "
             "default normalisation, theta from a 5-step fit; shapes are (generated rows = centres) x (training rows) x D"]
    for shape in args.shapes.split(","):
        m, n, d = (int(v) for v in shape.split("x"))
        gen, train = am.AudioMetricsData(True), am.AudioMetricsData(True)
        gen.add(rows(1, m, d, 0.1))
        train.add(rows(2, n, d))
        g, x = fld._prepare(((gen, "generated"), (train, "training")), train, "train", "fld_probe")
        theta, ll, history = fld._fit(g, x, 5, 0.5, -10.0)
        n_finite = history[5, 1:2].clone()
        mom, var = (torch.zeros(m, dtype=torch.float64, device=DEV) for _ in range(2))
        theta_out, out_a, out_b = (torch.empty(m, dtype=torch.float64, device=DEV) for _ in range(3))
        stats = torch.empty(3, dtype=torch.float64, device=DEV)
        ll_out = torch.empty(n, dtype=torch.float64, device=DEV)
        nb_l, nb_g = lib.am_fld_loglik_workspace_bytes(n, m, d), lib.am_fld_grad_workspace_bytes(m, n, d)
        ws_l, ws_g = ops._workspace(nb_l, DEV), ops._workspace(nb_g, DEV)
        eps = 1.0                                                       # of the order of the squared distances after the normalisation
        pot_g, pot_x = torch.zeros(m, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.float64, device=DEV)
        out_x, out_g = torch.empty(n, dtype=torch.float64, device=DEV), torch.empty(m, dtype=torch.float64, device=DEV)
        sstats = torch.empty(2, dtype=torch.float64, device=DEV)
        nb_sx, nb_sg = lib.am_softmin_workspace_bytes(n, m, d), lib.am_softmin_workspace_bytes(m, n, d)
        ws_sx, ws_sg = ops._workspace(nb_sx, DEV), ops._workspace(nb_sg, DEV)

        def run_loglik():
            ops._call(lib, "am_fld_loglik_f32", DEV, ops._ptr(x), n, ops._ld(x), ops._ptr(g), m, ops._ld(g), d, ops._ptr(theta),
                      ops._ptr(ll_out), ops._ptr(stats), ops._ptr(ws_l), nb_l)

        def run_grad():
            ops._call(lib, "am_fld_grad_f32", DEV, ops._ptr(g), m, ops._ld(g), ops._ptr(x), n, ops._ld(x), d, ops._ptr(theta), ops._ptr(ll),
                      ops._ptr(n_finite), ops._ptr(mom), ops._ptr(var), 6, 0.5, -10.0, ops._ptr(theta_out), ops._ptr(out_a),
                      ops._ptr(out_b), ops._ptr(ws_g), nb_g)

        def run_softmin_rows():                                         # the orientation of the loglik sweep
            ops._call(lib, "am_softmin_f32", DEV, ops._ptr(x), n, ops._ld(x), ops._ptr(g), m, ops._ld(g), d, ops._ptr(pot_g), eps, None,
                      0.0, ops._ptr(out_x), ops._ptr(sstats), ops._ptr(ws_sx), nb_sx)

        def run_softmin_centres():                                      # the orientation of the gradient sweep
            ops._call(lib, "am_softmin_f32", DEV, ops._ptr(g), m, ops._ld(g), ops._ptr(x), n, ops._ld(x), d, ops._ptr(pot_x), eps, None,
                      0.0, ops._ptr(out_g), ops._ptr(sstats), ops._ptr(ws_sg), nb_sg)
        (t_l, lo_l, hi_l), (t_g, lo_g, hi_g), (t_sx, lo_sx, hi_sx), (t_sg, lo_sg, hi_sg) = alternate(
            (run_loglik, run_grad, run_softmin_rows, run_softmin_centres), args.calls)
        lines.append(f"{m} x {n} x {d}: am_fld_loglik_f32 {t_l:9.3f} ms ({lo_l:.3f} .. {hi_l:.3f})  am_softmin_f32 same orientation "
                     f"{t_sx:9.3f} ms ({lo_sx:.3f} .. {hi_sx:.3f})  loglik / softmin {verdict(t_l / t_sx, 1.10)}")
        print(lines[-1], flush=True)
        lines.append(f"{m} x {n} x {d}: am_fld_grad_f32   {t_g:9.3f} ms ({lo_g:.3f} .. {hi_g:.3f})  am_softmin_f32 same orientation "
                     f"{t_sg:9.3f} ms ({lo_sg:.3f} .. {hi_sg:.3f})  gradient / softmin {verdict(t_g / t_sg, 1.25)}  "
                     f"workspace {nb_l / 2 ** 20:.1f} + {nb_g / 2 ** 20:.1f} MiB")
        print(lines[-1], flush=True)
        del ws_l, ws_g, ws_sx, ws_sg, g, x
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = am.feature_likelihood_fit(gen, train, steps=args.steps)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        lines.append(f"{m} x {n} x {d}: feature_likelihood_fit, {args.steps} steps: {wall:10.1f} ms wall (one run, normalisation and "
                     f"read-back included); nll_train {fit['fld_nll_train_history'][0]:.4f} -> {fit['fld_nll_train']:.4f}")
        print(lines[-1], flush=True)
        del gen, train, fit
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
