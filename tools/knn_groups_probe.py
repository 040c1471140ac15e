"""Timing probe of the leave-group-out nearest-neighbour search on one GPU (HIP events, warm, alternating calls, the median):

  search    am_knn_search_groups_f32 beside am_knn_search_f32 with self_offset = 0 in the same run: one 100 000-row set of
            windowed rows (runs of 36 windows per song, window spread 0.3 of the song spread) against itself, at 512 and
            128 columns, k = 1 and k = 5
              runs       labels in runs of 36, the stored order of the embedding pipeline.  Bar: grouped <= 1.05 x plain
                         (the Gram and gate work are the same; 5 % is the spread the README records between repeated runs
                         of one build).  MET or MISSED with the ratio.
              scattered  the same rows and labels under a seeded permutation of the stored order: every 32 x 32 sub-tile
                         that holds a same-label pair passes the first gate.  Reported only, no bar.
  whole     the wall time of one nearest_neighbor_two_sample_test at 100 000 + 100 000 rows with labels

    python tools/knn_groups_probe.py            # writes profiles/knn_groups/probe.txt
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
N, RUN, SPREAD = 100_000, 36, 0.3
WIDTHS, KS = (512, 128), (1, 5)
BAR = 1.05


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


def windowed_rows(seed, n, d, shift=0.0):
    """(rows float32 [n, d], labels int32 [n]) on the device: runs of RUN windows around song centres N(shift, I)"""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    songs = -(-n // RUN)
    song = torch.arange(songs, device=DEV).repeat_interleave(RUN)[:n]
    centres = torch.randn((songs, d), generator=g, device=DEV) + shift
    rows = centres[song] + SPREAD * torch.randn((n, d), generator=g, device=DEV)
    return ops.as_matrix(rows), song.to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=11, help="timed calls per function; the median is printed")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "knn_groups"))
    ap.add_argument("--no-whole", action="store_true", help="the search only: skip the whole test at 100 000 + 100 000 rows")
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    lib = am._lib.load()
    lines = [f"# {torch.cuda.get_device_name(0)}; HIP events, warm, median of {args.calls} alternating calls, one process",
             f"# {N} windowed rows against themselves, runs of {RUN} per song, window spread {SPREAD}; plain = am_knn_search_f32 with "
             "self_offset = 0, grouped = am_knn_search_groups_f32 on the same rows"]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    missed = 0
    for d in WIDTHS:
        rows, song = windowed_rows(1, N, d)
        perm = torch.as_tensor(np.random.default_rng(2).permutation(N)).to(DEV)
        for order, x, grp in (("runs", rows, song), ("scattered", ops.as_matrix(rows[perm]), song[perm].contiguous())):
            for k in KS:
                dist = torch.empty((N, k), dtype=torch.float32, device=DEV)
                idx = torch.empty((N, k), dtype=torch.int64, device=DEV)
                nb = lib.am_knn_search_groups_workspace_bytes(N, N, d, k)
                assert nb == lib.am_knn_search_workspace_bytes(N, N, d, k)
                ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)

                def plain():
                    ops._call(lib, "am_knn_search_f32", DEV, ops._ptr(x), N, ops._ld(x), ops._ptr(x), N, ops._ld(x), d, k, 0, 1,
                              ops._ptr(dist), ops._ptr(idx), ops._ptr(ws), nb)

                def grouped():
                    ops._call(lib, "am_knn_search_groups_f32", DEV, ops._ptr(x), N, ops._ld(x), ops._ptr(grp), ops._ptr(x), N, ops._ld(x),
                              ops._ptr(grp), d, k, 1, ops._ptr(dist), ops._ptr(idx), ops._ptr(ws), nb)

                (t_p, lo_p, hi_p), (t_g, lo_g, hi_g) = alternate((plain, grouped), args.calls)
                plain()
                sibling = float((grp[idx[:, 0].clamp(min=0)] == grp).float().mean())
                grouped()
                own = int(((idx >= 0) & (grp[idx.clamp(min=0)] == grp[:, None])).sum())
                ratio = t_g / t_p
                verdict = "report only"
                if order == "runs":
                    verdict = f"bar {BAR:.2f}: {'MET' if ratio <= BAR else 'MISSED'}"
                    missed += ratio > BAR
                say(f"search {order:9s} {N} x {N} x {d}, k = {k}: plain {t_p:8.3f} ms ({lo_p:.3f} .. {hi_p:.3f})  grouped {t_g:8.3f} ms "
                    f"({lo_g:.3f} .. {hi_g:.3f})  ratio {ratio:.3f}  {verdict}  ({lib.am_knn_search_chunks(N, N, d, k)} column chunks; "
                    f"nearest row is a sibling for {sibling:.3f} of the rows without labels, own-group neighbours with labels: {own})")
    say(f"# labels in runs: {'every case MET' if not missed else '%d case(s) MISSED' % missed} the bar grouped <= {BAR:.2f} x plain")
    if not args.no_whole:
        d = WIDTHS[0]
        cand, ref = am.AudioMetricsData(True), am.AudioMetricsData(True)
        x, gx = windowed_rows(3, N, d, shift=0.02)
        y, gy = windowed_rows(4, N, d)
        cand.add(x)
        ref.add(y)
        for attempt in range(2):                                        # the second call is the warm one
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = am.nearest_neighbor_two_sample_test(cand, ref, groups=gx, ref_groups=gy)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
        say(f"whole  nearest_neighbor_two_sample_test {N} + {N} x {d}, k = 1, 999 relabellings of {sum(out['nn_units'])} songs: "
            f"{wall:9.1f} ms wall, accuracy {out['nn_accuracy']:.4f}, null mean {out['nn_null_mean']:.4f}, p {out['nn_p_value']:.3g}")
    with open(os.path.join(args.out_dir, "probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
