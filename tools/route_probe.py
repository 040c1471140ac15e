#!/usr/bin/env python3
"""Which data-dependent route of the filter path a (family, shape) takes - read from am_filter_stats - and whether its
outputs equal the exact kernels' bit for bit, all in ONE process with the SHIPPED library: the exact k-NN values come from
the general entry point (columns = a copy of the set: am_knn_path == 0), the exact membership counts from reference-row
chunks small enough for am_prdc_path == 0.  Feeds tests/test_gpu_routes.py and, with WIDE_CASES (512 < D <= 4096),
tests/test_gpu_wide_filter.py and profiles/wide_filter/routes.txt.  Usage: tools/route_probe.py [case ...]"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ab_data import make  # noqa: E402
from audio_metrics_amd import hip_ops as ops  # noqa: E402


def shared_clusters(n, d, seed, offset):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    centers = torch.randn(50, d, generator=gen, device="cuda")
    gen2 = torch.Generator(device="cuda").manual_seed(seed + offset)
    lab = torch.randint(0, 50, (n,), generator=gen2, device="cuda")
    return centers[lab] + 1e-3 * torch.randn(n, d, generator=gen2, device="cuda")


def manifold_sets(n, n2, d, seed):
    """The `manifold` family of tests/test_gpu_routes.py (sets_of), draw for draw: a 24-dimensional set embedded in d dimensions
    plus noise - randn at d = 4096 has no nearest neighbours to speak of and goes to check A."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    basis = torch.randn(24, d, generator=g, device="cuda") / 24 ** 0.5
    return [torch.randn(rows, 24, generator=g, device="cuda") @ basis + 0.02 * torch.randn(rows, d, generator=g, device="cuda")
            for rows in (n, n2)]


def overflow_sets(n, d, seed):
    """The membership filter's `overflow` route by construction (tests/test_gpu_routes.py, test_membership_overflow_queue_route):
    40 identical candidate rows h in ONE column chunk; giving the first 256 reference rows radii equal to their distance to h
    (overflow_radii) puts 256 x 40 pairs ON their thresholds, all queued by one workgroup."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, d, generator=g, device="cuda")
    y = torch.randn(n, d, generator=g, device="cuda")
    y[1000:1040] = 0.3 * torch.randn(d, generator=g, device="cuda")
    return x, y


def overflow_radii(x, y, r):
    r = r.clone()
    r[:256] = (x[:256] - y[1000]).square().sum(1).sqrt()
    return r


def exact_radii(x, k):
    assert ops.knn_path(x.shape[0], x.shape[0], x.shape[1], k, self_distance=False) == 0
    return ops.knn_radii(x, k, columns=x.clone())


def exact_counts(ref, cand, r_ref, r_cand, want_min=False):
    nr, nc, d = ref.shape[0], cand.shape[0], ref.shape[1]
    step = nr
    while ops.prdc_path(step, nc, d) != 0:
        step = (step + 1) // 2
    cols, anys, covs, mins = 0, [], [], []
    for lo in range(0, nr, step):
        out = ops.prdc_counts(ref[lo:lo + step], cand, r_ref[lo:lo + step], r_cand, want_min=want_min)
        cols = cols + out[0]
        anys.append(out[1])
        covs.append(out[2])
        if want_min:
            mins.append(out[3])
    return (cols, torch.cat(anys), torch.cat(covs)) + ((torch.cat(mins),) if want_min else ())


CASES = {
    # name: (family, rows, rows2, dim, k, seed)
    "randn_20k_128": ("randn", 20000, 20000, 128, 5, 1),
    "unit_33k_192": ("unit", 33000, 9000, 192, 10, 2),
    "clustered_20k_512": ("clustered", 20000, 20000, 512, 5, 3),
    "shared_20k_512": ("shared", 20000, 20000, 512, 5, 4),
    "silence_40k_256": ("silence", 40000, 3001, 256, 5, 5),
    "hub_30k_128": ("hub", 30000, 30000, 128, 3, 6),
    "dups_12k_67": ("dups", 12000, 12000, 67, 8, 7),
    "scales_34567_130": ("scales", 34567, 4938, 130, 1, 8),
    "lowrank_20k_257": ("lowrank", 20000, 20000, 257, 5, 9),
    "randn_8200_512": ("randn", 8200, 8200, 512, 10, 10),
    "sparse_16400_64": ("sparse", 16400, 16400, 64, 5, 11),
    "tiny_20k_96": ("tiny", 20000, 20000, 96, 5, 12),
}

# The streamed 256 x 256 engine (512 < D <= 4096): the seeded cases of tests/test_gpu_wide_filter.py, which checks that the two
# tables agree.  Radii cases carry a token second set (64 rows); `manifold` is manifold_sets, `overflow` overflow_sets.
WIDE_CASES = {
    # radii over the slab counts nk = ceil(D / 64) = 9 ... 64, k <= 5 (KCAP = 6) and k = 10 (KCAP = 11)
    "wide_randn_6411_513_k5": ("randn", 6411, 64, 513, 5, 7),
    "wide_randn_6411_576_k5": ("randn", 6411, 64, 576, 5, 7),
    "wide_randn_6411_576_k10": ("randn", 6411, 64, 576, 10, 7),
    "wide_randn_6411_640_k5": ("randn", 6411, 64, 640, 5, 7),
    "wide_randn_6411_704_k5": ("randn", 6411, 64, 704, 5, 7),
    "wide_randn_6411_768_k5": ("randn", 6411, 64, 768, 5, 7),
    "wide_randn_6411_768_k10": ("randn", 6411, 64, 768, 10, 7),
    "wide_randn_6411_1000_k5": ("randn", 6411, 64, 1000, 5, 7),
    "wide_randn_6411_1024_k5": ("randn", 6411, 64, 1024, 5, 7),
    "wide_randn_6411_2048_k5": ("randn", 6411, 64, 2048, 5, 7),
    "wide_randn_6411_2048_k10": ("randn", 6411, 64, 2048, 10, 7),
    "wide_manifold_6411_4096_k5": ("manifold", 6411, 64, 4096, 5, 28),
    "wide_unit_6411_768_k5": ("unit", 6411, 64, 768, 5, 7),
    "wide_randn_6400_768_k5": ("randn", 6400, 64, 768, 5, 7),
    "wide_randn_6145_768_k5": ("randn", 6145, 64, 768, 5, 7),
    # membership counts, 4111 x 4203 (>= 2^24 pairs), and two unequal pairs
    "wide_counts_randn_513": ("randn", 4111, 4203, 513, 5, 31),
    "wide_counts_randn_576": ("randn", 4111, 4203, 576, 5, 31),
    "wide_counts_randn_768": ("randn", 4111, 4203, 768, 5, 31),
    "wide_counts_randn_1024": ("randn", 4111, 4203, 1024, 5, 31),
    "wide_counts_randn_2048": ("randn", 4111, 4203, 2048, 5, 31),
    "wide_counts_manifold_3328": ("manifold", 4111, 4203, 3328, 5, 31),
    "wide_counts_randn_1100x16000_768": ("randn", 1100, 16000, 768, 5, 33),
    "wide_counts_randn_16000x1100_768": ("randn", 16000, 1100, 768, 5, 35),
    # the data-dependent routes at D = 768
    "wide_silence_6411_768": ("silence", 6411, 6411, 768, 5, 26),
    "wide_clustered_6411_768": ("clustered", 6411, 6411, 768, 5, 3),
    "wide_tiny_6411_768": ("tiny", 6411, 6411, 768, 5, 12),
    "wide_shared_6411_768": ("shared", 6411, 6411, 768, 5, 4),
    "wide_overflow_6411_768": ("overflow", 6411, 6411, 768, 5, 830),
}
CASES.update(WIDE_CASES)

if __name__ == "__main__":
    names = sys.argv[1:] or list(CASES)
    ops.filter_stats_enable("cuda:0", True)
    for name in names:
        fam, n, n2, d, k, seed = CASES[name]
        if fam == "shared":
            x, y = shared_clusters(n, d, seed, 1), shared_clusters(n2, d, seed, 2)
        elif fam == "manifold":
            x, y = manifold_sets(n, n2, d, seed)
        elif fam == "overflow":
            x, y = overflow_sets(n, d, seed)
        else:
            x, y = make(fam, n, d, seed), make(fam, n2, d, seed + 100)
        ops.filter_stats_read("cuda:0")
        t0 = time.perf_counter()
        r = ops.knn_radii(x, k)
        torch.cuda.synchronize()
        t_knn = time.perf_counter() - t0
        s_knn = ops.filter_stats_read("cuda:0")
        ok_r = torch.equal(r.view(torch.int32), exact_radii(x, k).view(torch.int32))
        r2 = ops.knn_radii(y, k)
        if fam == "overflow":
            r = overflow_radii(x, y, r)
        ops.filter_stats_read("cuda:0")
        want_min = seed % 2 == 1
        t0 = time.perf_counter()
        got = ops.prdc_counts(x, y, r, r2, want_min=want_min)
        torch.cuda.synchronize()
        t_cross = time.perf_counter() - t0
        s_cross = ops.filter_stats_read("cuda:0")
        want = exact_counts(x, y, r, r2, want_min)
        ok_c = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
                   for a, b in zip(got, want))
        print(f"{name}: paths {ops.knn_path(n, n, d, k)}/{ops.prdc_path(n, n2, d)} radii {'ok' if ok_r else 'MISMATCH'} counts {'ok' if ok_c else 'MISMATCH'} | "
              f"knn {t_knn * 1e3:.1f} ms queued {s_knn['knn_queued']} spilled {s_knn['knn_spilled']} verified {s_knn['knn_verified_pairs']} "
              f"fallback_rows {s_knn['knn_fallback_rows']} bound {s_knn['bound_ratio_max']:.3f} on {s_knn['bound_pairs']} | "
              f"cross {t_cross * 1e3:.1f} ms queued {s_cross['prdc_queued']} overflow {s_cross['prdc_overflow_queue']} "
              f"fallback {s_cross['prdc_fallback_calls']}", flush=True)
