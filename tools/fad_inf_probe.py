#!/usr/bin/env python3
"""FAD-infinity against the composition of the entry points that existed before it (GPU-box aid).

For each shape (candidate rows x columns, dtype; reference of 100 000 rows or as many as the candidate), steps = 15 and
min_n = 5000 (a quarter of the set where it holds fewer than 20 000 rows):
  (a) frechet_distance_inf: one gathered-statistics call, one batched solve, host fit;
  (b) per subset X.index_select(0, idx_b) -> hip_ops.stats -> hip_ops.frechet on the SAME indices, then the same fit.
Median of 20 calls after 3 warm-ups, torch.cuda.synchronize around each; the split of (a) into draw / statistics /
solve / fit; max |difference| between the per-subset values of (a) and (b)."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_metrics_amd as am  # noqa: E402
from audio_metrics_amd import _build, _lib, hip_ops as ops  # noqa: E402
from audio_metrics_amd.metrics import fad  # noqa: E402

SHAPES = ((100_000, 512, torch.float32), (100_000, 128, torch.float32), (20_000, 64, torch.float64))
STEPS, WARMUP, REPEAT = 15, 3, 20
dev = torch.device("cuda:0")


def timed(fn):
    for _ in range(WARMUP):
        fn()
    times = []
    for _ in range(REPEAT):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), out


with open(_build._stamp_path(_lib.library_path())) as fh:
    print("library", json.load(fh).get("sources_sha256"), torch.cuda.get_device_name(0))
for n, d, dtype in SHAPES:
    gen = torch.Generator(device=dev).manual_seed(n + d)
    spectrum = 1.0 / torch.sqrt(1.0 + torch.arange(d, device=dev, dtype=torch.float64))
    cand_rows = ((torch.randn((n, d), generator=gen, device=dev, dtype=torch.float64) * spectrum) * 1.05 + 0.05).to(dtype)
    ref_rows = (torch.randn((max(n, 100_000) if d > 64 else n, d), generator=gen, device=dev, dtype=torch.float64) * spectrum).to(dtype)
    x, y = am.AudioMetricsData(True), am.AudioMetricsData(False)
    x.add(cand_rows)
    y.add(ref_rows)
    min_n = 5000 if n >= 20_000 * 4 else n // 4
    sizes = np.linspace(min_n, n, STEPS).round().astype(int)
    rows = x.embeddings
    mu_y, cov_y = y.mean, y.cov

    def new_way():
        return am.frechet_distance_inf(x, y, steps=STEPS, min_n=min_n, seed=0), list(fad.last_info["fads"])

    def old_way():
        idx, offsets = fad.fad_inf_subset_indices(n, sizes, 0, dev)
        fads = []
        for b in range(STEPS):
            mean, cov = ops.stats(rows.index_select(0, idx[offsets[b]:offsets[b + 1]]))
            fads.append(ops.frechet(mean, cov, mu_y, cov_y, fad.NS_MAX_ITER, fad.NS_TOL)["fd"])
        return fad.fit_inverse_n(sizes, fads), fads

    ms_a, (res_a, fads_a) = timed(new_way)
    ms_b, (res_b, fads_b) = timed(old_way)
    draw, (idx, offsets) = timed(lambda: fad.fad_inf_subset_indices(n, sizes, 0, dev))
    stat, (means, covs) = timed(lambda: ops.stats_gather(rows, idx, offsets))
    solve, recs = timed(lambda: ops.frechet_batch(means, covs, mu_y, cov_y, fad.NS_MAX_ITER, fad.NS_TOL))
    fit, _ = timed(lambda: fad.fit_inverse_n(sizes, [r["fd"] for r in recs]))
    diff = max(abs(a - b) for a, b in zip(fads_a, fads_b))
    print(f"{n} x {d} {str(dtype).split('.')[-1]} steps {STEPS} min_n {min_n}: (a) frechet_distance_inf {ms_a:.3f} ms | "
          f"(b) index_select + stats + frechet per subset {ms_b:.3f} ms | (a) split: draw {draw:.3f} statistics {stat:.3f} "
          f"solve {solve:.3f} fit {fit:.3f} ms | max |a - b| per subset {diff:.3e} | fad_inf {res_a['fad_inf']:.6e} "
          f"(b: {res_b[0]:.6e}) iterations {[r['iters'] for r in recs]}")
