"""Timing and accuracy probe of the random-feature Gaussian Vendi score on one GPU (HIP events, warm, alternating calls, the
median of 11; one process):

  moment    am_rff_moment_f32 at rows x D, R = 1024, beside the torch composition on the same inputs in the same run:
                z = x @ w.T * inv_bw;  phi = cat(cos z, sin z).double() / sqrt(R);  phi.T @ phi / n
            the bar is moment <= 1.0 x torch (README, "Gaussian Vendi at scale"); the largest difference of the two is printed
  features  am_rff_features_f32 over all rows alone
  calls     a whole vendi_score_rff, cold (a fresh set: the median bandwidth is selected) and with the bandwidth cached; the
            share of am_eigh_sym_f64 in it; a whole kernel_novelty_score with the reference's matrix cached; rke_score
  bytes     the workspace of the moment

    python tools/rff_probe.py          (writes profiles/rff/probe.txt and profiles/rff/accuracy.txt)

accuracy.txt: the float64 oracle of tests/rff_reference.py against the exact Gaussian spectrum (1200 x 32 cluster set, seeds
0 .. 7, R = 1024 and 256), the exact RKE identity, and the device against both on the same set."""
import argparse
import math
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
import rff_reference as ref                                             # noqa: E402

DEV = torch.device("cuda", 0)


def rows(seed, n, d, shift=0.0):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return (torch.randn((n, d), generator=g, device=DEV) + shift) / math.sqrt(d)       # norms near 1, as CLAP rows have


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


def data_set(x):
    s = am.AudioMetricsData(True)
    s.add(x)
    return s


def timing(args, say):
    lib = am._lib.load()
    n, r = args.rows, args.features
    for d in (512, 128):
        x = rows(1, n, d)
        w = torch.as_tensor(am.rff_frequencies(d, r, 0)).to(DEV)
        inv_bw = 1.0 / math.sqrt(2.0)                              # the median distance of such rows is near sqrt(2)
        s = torch.empty((2 * r, 2 * r), dtype=torch.float64, device=DEV)
        nb = lib.am_rff_moment_workspace_bytes(n, d, r)
        ws = ops._workspace(nb, DEV)

        def run_moment():
            ops._call(lib, "am_rff_moment_f32", DEV, ops._ptr(x), n, ops._ld(x), d, ops._ptr(w), r, ops._ld(w), inv_bw, None, ops._ptr(s),
                      ops._ptr(ws), nb)

        def run_torch():
            z = x @ w.T * inv_bw
            phi = torch.cat([torch.cos(z), torch.sin(z)], dim=1).double() / math.sqrt(r)
            return phi.T @ phi / n
        (t_m, lo_m, hi_m), (t_t, lo_t, hi_t) = alternate((run_moment, run_torch), args.calls)
        diff = float((s - run_torch()).abs().max())
        verdict = "MET" if t_m <= t_t else f"MISSED by {100.0 * (t_m / t_t - 1.0):.0f} %"
        say(f"moment {n} x {d}, R = {r}: am_rff_moment_f32 {t_m:8.3f} ms ({lo_m:.3f} .. {hi_m:.3f})  torch composition {t_t:8.3f} ms "
            f"({lo_t:.3f} .. {hi_t:.3f})  ratio {t_m / t_t:5.3f} (bar <= 1.0: {verdict})  {lib.am_rff_moment_chunks(n, r)} chunks, workspace "
            f"{nb} bytes = {nb / 2 ** 20:.1f} MiB; largest |S - torch's| {diff:.2e} (torch takes cos and sin in float32)")
        # ---- the features alone, over all rows
        f = torch.empty((2 * r, n), dtype=torch.float64, device=DEV)
        nbf = lib.am_rff_features_workspace_bytes(n)
        wsf = ops._workspace(nbf, DEV)

        def run_features():
            ops._call(lib, "am_rff_features_f32", DEV, ops._ptr(x), n, ops._ld(x), d, ops._ptr(w), r, ops._ld(w), 0, n, inv_bw, None, ops._ptr(f),
                      n, ops._ptr(wsf), nbf)
        ((t_f, lo_f, hi_f),) = alternate((run_features,), args.calls)
        say(f"features {n} x {d}, R = {r}: am_rff_features_f32 {t_f:8.3f} ms ({lo_f:.3f} .. {hi_f:.3f})  {16.0 * r * n / t_f / 1e6:.0f} GB/s of "
            f"feature stores")
        del f, wsf
        # ---- the solver's share and the whole calls
        run_moment()
        ((t_e, lo_e, hi_e),) = alternate((lambda: ops.eigh_descending(s),), 3)
        t_cold = wall_ms(lambda: am.vendi_score_rff(data_set(x), n_features=r))
        cached = data_set(x)
        am.vendi_score_rff(cached, n_features=r)
        t_warm = wall_ms(lambda: am.vendi_score_rff(cached, n_features=r))
        got = am.vendi_score_rff(cached, n_features=r)
        say(f"vendi_score_rff {n} x {d}, R = {r}: {t_cold:9.2f} ms wall cold (median of 3; the median bandwidth is selected), {t_warm:9.2f} ms "
            f"with the bandwidth cached, of which am_eigh_sym_f64 {t_e:8.2f} ms ({lo_e:.2f} .. {hi_e:.2f}) = {100.0 * t_e / t_warm:.0f} %; "
            f"scores {np.round(got['vendi_rff_per_order'], 3).tolist()} at bandwidth {got['vendi_rff_bandwidth']:.4f}, rank {got['vendi_rff_rank']}")
        cand = data_set(rows(2, n, d, 0.02))
        am.kernel_novelty_score(cand, cached, n_features=r)
        t_nov = wall_ms(lambda: am.kernel_novelty_score(cand, cached, n_features=r))
        t_rke = wall_ms(lambda: am.rke_score(cached))
        say(f"kernel_novelty_score {n} x {n} x {d}, R = {r}, the reference's matrix cached: {t_nov:9.2f} ms wall;  rke_score {n} x {d}: "
            f"{t_rke:9.2f} ms wall, rke {am.rke_score(cached)['rke']:.3f}")
        del x, w, s, ws, cached, cand
        torch.cuda.empty_cache()


def accuracy(say):
    x = ref.cluster_set()
    bw = ref.median_bandwidth(x)
    exact = ref.exact_eigenvalues(x, bw)
    orders = (1.0, 2.0, math.inf)
    want = np.log(ref.scores(exact, orders))
    rke, _ = ref.rke_exact(x, bw)
    say(f"cluster set 1200 x 32 (ten N(0, I) centres + 0.3 N(0, I)), median bandwidth {bw:.6f}; exact scores at orders 1, 2, inf: "
        f"{np.round(np.exp(want), 4).tolist()}")
    say(f"oracle: exact rke {rke!r} against 1 / sum lam^2 of the exact K / n {1.0 / float(np.sum(exact ** 2))!r}: relative "
        f"{abs(rke * float(np.sum(exact ** 2)) - 1.0):.2e}")
    xd = torch.as_tensor(x).to(DEV)
    for r in (1024, 256):
        gaps, dev_gaps = [], []
        for seed in range(8):
            lam = ref.eigenvalues(x, ref.frequencies(32, r, seed), 1.0 / bw)
            gaps.append(np.abs(np.log(ref.scores(lam, orders)) - want))
            got = am.vendi_score_rff(xd, orders=orders, bandwidth=bw, n_features=r, seed=seed)
            dev_gaps.append(np.abs(np.log(got["vendi_rff_per_order"]) - np.log(ref.scores(lam, orders))))
        say(f"oracle, R = {r}, seeds 0 .. 7: max |ln(rff / exact)| at orders 1, 2, inf: {np.max(gaps, axis=0).round(5).tolist()}")
        say(f"device, R = {r}, seeds 0 .. 7: max |ln(device / oracle with the same W)| at orders 1, 2, inf: "
            f"{[float('%.2e' % v) for v in np.max(dev_gaps, axis=0)]}")
    dev_rke = am.rke_score(xd, bandwidth=bw)["rke"]
    gram = am.vendi_score(xd, "gaussian", orders=(1.0,), bandwidth=bw, route="gram")["vendi"]
    got = am.vendi_score_rff(xd, orders=(1.0, 2.0), bandwidth=bw, n_features=1024, seed=0)["vendi_rff_per_order"]
    say(f"device, R = 1024, seed 0: ln(order 1 / vendi_score on the Gram route) {math.log(got[0] / gram):+.5f}, ln(order 2 / rke_score) "
        f"{math.log(got[1] / dev_rke):+.5f}; rke_score / oracle - 1 = {dev_rke / rke - 1.0:+.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=11, help="timed calls per function; the median is printed")
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rff"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    for name, part, head in (("accuracy.txt", lambda say: accuracy(say), "float64 numpy oracle (tests/rff_reference.py) and the device"),
                             ("probe.txt", lambda say: timing(args, say), f"HIP events, warm, median of {args.calls} alternating calls; randn rows / sqrt(D)")):
        lines = [f"# {torch.cuda.get_device_name(0)}; {head}"]

        def say(line):
            lines.append(line)
            print(line, flush=True)
        part(say)
        with open(os.path.join(args.out, name), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
