"""Timing probe of the leave-group-out per-sample scores on one GPU (HIP events, warm, alternating calls, the median):

  kernel    am_sample_scores_groups_f32 beside am_sample_scores_f32 in the same run, on the same matrices and radii: windowed
            rows (runs of 36 windows per song, window spread 0.3 of the song spread), the samples being OTHER windows of the
            manifold's songs, leave-group-out radii of k = 5; 100 000 x 100 000 rows at 512 and at 128 columns and
            1 000 x 100 000 at 512
              disjoint   the samples' label values shifted away from the manifold's: the labels are pure overhead, the five
                         outputs are those of the plain kernel (checked).  Bar: grouped <= 1.05 x plain - the margin the
                         leave-group-out search met for the same step (tools/knn_groups_probe.py).  MET or MISSED with the ratio.
              shared     the same rows with the songs' own labels on both sides: the outputs differ, and the excluded members
                         visit the rare path.  Reported only, no bar.
              scattered  shared labels under a seeded permutation of the stored order of both sets.  Reported only, no bar.
  whole     the wall time of one prdc_leave_group_out at 100 000 x 100 000 x 512 (five Gram sweeps on the exact engine)

    python tools/sample_scores_groups_probe.py            # writes profiles/sample_scores_groups/probe.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_metrics_amd as am                                          # noqa: E402
from audio_metrics_amd import hip_ops as ops                            # noqa: E402

DEV = torch.device("cuda", 0)
M, RUN, SPREAD, K = 100_000, 36, 0.3, 5
SHAPES = ((100_000, 512), (100_000, 128), (1_000, 512))                 # (samples, columns) against M manifold rows
BAR = 1.05
FAR = 1 << 20                                                           # shifts the samples' labels past the manifold's


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


def windowed_rows(seed_songs, seed_windows, n, d, shift=0.0):
    """(rows float32 [n, d], labels int32 [n]) on the device: runs of RUN windows around song centres N(shift, I); the centres
    depend on seed_songs alone, so two calls with one seed_songs give other windows of the same songs"""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed_songs)
    songs = -(-n // RUN)
    song = torch.arange(songs, device=DEV).repeat_interleave(RUN)[:n]
    centres = torch.randn((songs, d), generator=g, device=DEV) + shift
    g.manual_seed(seed_windows)
    rows = centres[song] + SPREAD * torch.randn((n, d), generator=g, device=DEV)
    return ops.as_matrix(rows), song.to(torch.int32)


def same_bits(a, b):
    return all(torch.equal(s.view(torch.int32) if s.dtype == torch.float32 else s, t.view(torch.int32) if t.dtype == torch.float32 else t)
               for s, t in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=11, help="timed calls per function; the median is printed")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "sample_scores_groups"))
    ap.add_argument("--no-whole", action="store_true", help="the kernel only: skip the whole prdc_leave_group_out")
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    lib = am._lib.load()
    lines = [f"# {torch.cuda.get_device_name(0)}; HIP events, warm, median of {args.calls} alternating calls, one process",
             f"# samples x {M} windowed manifold rows, runs of {RUN} per song, window spread {SPREAD}, the samples other windows of the "
             f"same songs; leave-group-out radii of k = {K}; plain = am_sample_scores_f32, grouped = am_sample_scores_groups_f32 on the "
             "same matrices and radii"]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    missed = 0
    for n, d in SHAPES:
        y, gy = windowed_rows(1, 2, M, d)
        x, gx = windowed_rows(1, 3, M, d)
        x, gx = ops.as_matrix(x[:n]), gx[:n].contiguous()
        radii = ops.knn_search_groups(y, y, K, gy, gy)[0][:, K - 1].contiguous()
        px = torch.as_tensor(np.random.default_rng(4).permutation(n)).to(DEV)
        py = torch.as_tensor(np.random.default_rng(5).permutation(M)).to(DEV)
        cases = (("disjoint", x, y, radii, (gx + FAR).contiguous(), gy),
                 ("shared", x, y, radii, gx, gy),
                 ("scattered", ops.as_matrix(x[px]), ops.as_matrix(y[py]), radii[py].contiguous(), gx[px].contiguous(), gy[py].contiguous()))
        for order, xs, ys, rs, lx, ly in cases:
            out = [torch.empty(n, dtype=t, device=DEV) for t in (torch.float32, torch.int64, torch.int32, torch.float32, torch.int64)]
            out_g = [torch.empty_like(t) for t in out]
            nb = lib.am_sample_scores_groups_workspace_bytes(n, M, d)
            assert nb == lib.am_sample_scores_workspace_bytes(n, M, d)
            ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)

            def plain():
                ops._call(lib, "am_sample_scores_f32", DEV, ops._ptr(xs), n, ops._ld(xs), ops._ptr(ys), M, ops._ld(ys), d, ops._ptr(rs),
                          *(ops._ptr(t) for t in out), ops._ptr(ws), nb)

            def grouped():
                ops._call(lib, "am_sample_scores_groups_f32", DEV, ops._ptr(xs), n, ops._ld(xs), ops._ptr(lx), ops._ptr(ys), M, ops._ld(ys),
                          ops._ptr(ly), d, ops._ptr(rs), *(ops._ptr(t) for t in out_g), ops._ptr(ws), nb)

            (t_p, lo_p, hi_p), (t_g, lo_g, hi_g) = alternate((plain, grouped), args.calls)
            plain()
            grouped()
            torch.cuda.synchronize()
            members, members_g = int(out[2].to(torch.int64).sum()), int(out_g[2].to(torch.int64).sum())
            inside, inside_g = float((out[2] > 0).float().mean()), float((out_g[2] > 0).float().mean())
            ratio = t_g / t_p
            verdict = "report only"
            if order == "disjoint":
                assert same_bits(out, out_g), "disjoint labels must give the plain outputs"
                verdict = f"bar {BAR:.2f}: {'MET' if ratio <= BAR else 'MISSED'}"
                missed += ratio > BAR
            say(f"kernel {order:9s} {n} x {M} x {d}: plain {t_p:8.3f} ms ({lo_p:.3f} .. {hi_p:.3f})  grouped {t_g:8.3f} ms "
                f"({lo_g:.3f} .. {hi_g:.3f})  ratio {ratio:.3f}  {verdict}  ({lib.am_sample_scores_chunks(n, M, d)} column chunks; "
                f"member pairs {members} -> {members_g}, rows inside some ball {inside:.3f} -> {inside_g:.3f})")
    say(f"# disjoint labels: {'every case MET' if not missed else '%d case(s) MISSED' % missed} the bar grouped <= {BAR:.2f} x plain")
    if not args.no_whole:
        d = SHAPES[0][1]
        cand, ref = am.AudioMetricsData(True), am.AudioMetricsData(True)
        y, gy = windowed_rows(1, 2, M, d)
        x, gx = windowed_rows(1, 3, M, d)
        cand.add(x)
        ref.add(y)
        for attempt in range(2):                                        # the second call is the warm one
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = am.prdc_leave_group_out(ref, cand, K, gy, gx)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
        say(f"whole  prdc_leave_group_out {M} x {M} x {d}, k = {K}, {res['shared_labels']} shared songs: {wall:9.1f} ms wall  "
            f"precision {res['precision']:.4f} recall {res['recall']:.4f} density {res['density']:.4f} coverage {res['coverage']:.4f}")
    with open(os.path.join(args.out_dir, "probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
