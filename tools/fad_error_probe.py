"""Timing and accuracy probe of the Frechet-distance error bars on one GPU (HIP events, warm, alternating calls, the median):

  rows      am_frechet_influence_f32 beside the torch composition that produces the same vector in the same run,
            c = x.double() - mu; ((c @ B) * c).sum(1) - which writes and reads two N x D float64 intermediates the kernel
            never forms; the bar is kernel <= composition
  maps      am_frechet_maps_f64 beside am_frechet_f64 on the same statistics; the bar is the plain solve plus two
            D x D x D products (an iteration of the solve is three)
  whole     the wall time of one frechet_distance_with_error at 100 000 x 100 000 x 512
  accuracy  the ACCURACY lines that tests/test_gpu_fad_stats.py prints before it asserts: the figures its measured
            tolerances are taken from (the test run is a child process, started before this one touches the GPU)

    python tools/fad_error_probe.py            # writes profiles/fad_error/probe.txt and profiles/fad_error/accuracy.txt
"""
import argparse
import ctypes
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_metrics_amd as am                                          # noqa: E402
from audio_metrics_amd import hip_ops as ops                            # noqa: E402

DEV = torch.device("cuda", 0)
F64_MFMA_PEAK = 78.6e12                                                 # flop/s, dense f64 matrix cores of one MI355X
SHAPES = ((100_000, 512), (100_000, 128))


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


def rows_of(seed, n, d, shift):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    mix = torch.eye(d, device=DEV) + 0.3 / d ** 0.5 * torch.randn((d, d), generator=g, device=DEV)
    return torch.randn((n, d), generator=g, device=DEV) @ mix + shift * torch.randn(d, generator=g, device=DEV)


def accuracy_lines(timeout):
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_fad_stats.py"), "-m", "gpu", "-s", "-q",
                        "-p", "no:cacheprovider"], cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    lines = [line[line.index("ACCURACY ") + 9:].rstrip() for line in r.stdout.splitlines() if "ACCURACY " in line]
    tail = [line for line in r.stdout.splitlines() if " passed" in line or " failed" in line]
    return lines, (tail[-1].strip("= ") if tail else f"pytest exit status {r.returncode}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=11, help="timed calls per function; the median is printed")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "fad_error"))
    ap.add_argument("--no-accuracy", action="store_true", help="timing only: leave accuracy.txt as it is")
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    if not args.no_accuracy:
        acc, verdict = accuracy_lines(900)
        print("\n".join(acc), flush=True)
    lib = am._lib.load()
    name = torch.cuda.get_device_name(0)
    if not args.no_accuracy:
        with open(os.path.join(args.out_dir, "accuracy.txt"), "w") as f:
            f.write(f"# {name}; the figures tests/test_gpu_fad_stats.py prints before it asserts (float64 numpy oracle: "
                    f"tests/fad_stats_reference.py); that run: {verdict}\n" + "\n".join(acc) + "\n")
    lines = [f"# {name}; HIP events, warm, median of {args.calls} alternating calls, one process"]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    sets = {}
    for n, d in SHAPES:
        x, y = rows_of(1, n, d, 0.3), rows_of(2, n, d, 0.0)
        cand, ref = am.AudioMetricsData(True), am.AudioMetricsData(True)
        cand.add(x)
        ref.add(y)
        sets[d] = (cand, ref)
        mu_x, cov_x, mu_y, cov_y = cand.mean.reshape(-1), cand.cov, ref.mean.reshape(-1), ref.cov

        # ---- the solve with and without the maps
        nb = lib.am_frechet_workspace_bytes(d)
        ws = ops._workspace(nb, DEV)
        out4, out5 = (ctypes.c_double * 4)(), (ctypes.c_double * 5)()
        map_xy, map_yx = (torch.empty((d, d), dtype=torch.float64, device=DEV) for _ in range(2))
        head = (ops._ptr(mu_x), ops._ptr(cov_x), ops._ptr(mu_y), ops._ptr(cov_y), d, 64, 1e-13)

        def plain():
            ops._call(lib, "am_frechet_f64", DEV, *head, ctypes.cast(out4, ctypes.c_void_p), ops._ptr(ws), nb)

        def with_maps():
            ops._call(lib, "am_frechet_maps_f64", DEV, *head, ctypes.cast(out5, ctypes.c_void_p), ops._ptr(map_xy), ops._ptr(map_yx),
                      ops._ptr(ws), nb)
        t_p, r_p, t_m, r_m = alternate(plain, with_maps, args.calls)
        iters = int(out5[2])
        per_product = t_p / (3.0 * iters + 1.0)                         # the chain: one product, then three per iteration
        say(f"maps   D = {d}: am_frechet_f64 {t_p:8.3f} ms ({r_p[0]:.3f} .. {r_p[1]:.3f})  am_frechet_maps_f64 {t_m:8.3f} ms "
            f"({r_m[0]:.3f} .. {r_m[1]:.3f})  difference {t_m - t_p:7.3f} ms; {iters} iterations, stop code {int(out5[4])}: a D x D x D "
            f"product of the chain is about {per_product:.3f} ms, the bar (two of them) {2 * per_product:.3f} ms - "
            f"{'met' if t_m - t_p <= 2 * per_product else 'MISSED'}")

        # ---- the row pass beside the torch composition
        b = torch.eye(d, dtype=torch.float64, device=DEV) - map_xy
        lin = 2.0 * (mu_x - mu_y)
        c0 = -float((b * cov_x).sum())
        rows = ops.as_rows(cand.embeddings)
        psi, sums = torch.empty(n, dtype=torch.float64, device=DEV), torch.empty(4, dtype=torch.float64, device=DEV)
        nbi = lib.am_frechet_influence_workspace_bytes(n)
        wsi = ops._workspace(nbi, DEV)
        keep = {}

        def kernel():
            ops._call(lib, "am_frechet_influence_f32", DEV, ops._ptr(rows), n, ops._ld(rows), d, ops._ptr(mu_x), ops._ptr(b), ops._ptr(lin),
                      c0, ops._ptr(psi), ops._ptr(sums), ops._ptr(wsi), nbi)

        def composition():
            c = rows.double() - mu_x
            keep["quad"] = ((c @ b) * c).sum(1)
        t_c, r_c, t_k, r_k = alternate(composition, kernel, args.calls)
        quad = psi - (rows.double() - mu_x) @ lin - c0
        agree = float((quad - keep["quad"]).abs().max() / keep["quad"].abs().max())
        flop = 2.0 * n * d * d
        say(f"rows   {n} x {d}: torch composition {t_c:8.3f} ms ({r_c[0]:.3f} .. {r_c[1]:.3f})  am_frechet_influence_f32 {t_k:8.3f} ms "
            f"({r_k[0]:.3f} .. {r_k[1]:.3f})  ratio {t_k / t_c:5.3f} (bar <= 1: {'met' if t_k <= t_c else 'MISSED'})  kernel at "
            f"{100 * flop / F64_MFMA_PEAK / (t_k * 1e-3):.0f} % of the f64 matrix peak; the two vectors agree to {agree:.1e} of the largest")
        del keep, quad

    cand, ref = sets[512]
    torch.cuda.synchronize()
    walls = []
    for _ in range(6):
        t0 = time.perf_counter()
        res = am.frechet_distance_with_error(cand, ref)
        walls.append(time.perf_counter() - t0)
    say(f"whole  frechet_distance_with_error 100000 x 100000 x 512: first call {1e3 * walls[0]:.1f} ms, then median "
        f"{1e3 * sorted(walls[1:])[2]:.1f} ms wall per call ({1e3 * min(walls[1:]):.1f} .. {1e3 * max(walls[1:]):.1f}); fad {res['fad']:.6f} "
        f"+- {res['fad_std_error']:.6f}, map residual {res['fad_map_residual']:.2e}")
    t0 = time.perf_counter()
    am.frechet_distance(cand, ref)
    say(f"whole  frechet_distance on the same sets: {1e3 * (time.perf_counter() - t0):.1f} ms wall")
    with open(os.path.join(args.out_dir, "probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
