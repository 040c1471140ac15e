"""The streamed 256 x 256 f16 filter engine (csrc/wide_engine.h; knn_wide_kernel<6|11> and cross_wide_kernel<false|true> of
csrc/pairwise_wide.hip, bodies in csrc/wide_kernels.h instantiated with WideEng) at the widths only it serves: 512 < D <= 4096.

What is its own and what the stationary engines' tests (test_gpu_routes.py, test_gpu_pstat_shape.py, test_gpu_fuzz_slice.py,
all at D <= 512) therefore cannot see:
  * the lane geometry NT = 2, MT = 4, GROUPS = 2, GSTRIDE = 8 with four partial lists per row - another register -> (row, column)
    map in both epilogues;
  * every !ACC_INIT branch of the shared epilogues (athr[], aux rows in distance units, the fma that adds the column norm);
  * wide_pipeline's run-time slab count nk = ceil(D / 64) = 9 ... 64: stages alternate LDS buffers by g = t nk + kt, the side
    data by t & 1 - with an odd nk the first stage of successive tiles changes buffers while the aux buffer does not.

Shapes are the smallest that reach the kernels: 6411 rows for the radii (above the 6144-row threshold of D >= 256: 25 full
256-row blocks and a last one of 11 rows; pre_stride = 16, so the sample pass sees tiles 0 and 16), 4111 x 4203 for the
membership counts (>= 2^24 pairs; last blocks of 15 and 107 rows).  Exact values as in test_gpu_routes.py: the general entry
points of the SHIPPED library (tools/route_probe.py, exact_radii / exact_counts), and those are anchored to plain float64
arithmetic on the CPU at these widths at the end of this file.  Every case asserts the ROUTE it took through am_filter_stats;
the seeded cases are also in route_probe.CASES (the two tables are compared), their measured routes and bound ratios in
profiles/wide_filter/routes.txt."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

N = 6411
NR, NC = 4111, 4203

# name: (family, rows, rows of the second set, dim, k, seed) - the tuple of route_probe.CASES[name]
RADII = {
    "wide_randn_6411_513_k5": ("randn", N, 64, 513, 5, 7),           # nk = 9: padded to 576, the last slab holds one element
    "wide_randn_6411_576_k5": ("randn", N, 64, 576, 5, 7),           # nk = 9, odd
    "wide_randn_6411_576_k10": ("randn", N, 64, 576, 10, 7),
    "wide_randn_6411_640_k5": ("randn", N, 64, 640, 5, 7),           # nk = 10, even
    "wide_randn_6411_704_k5": ("randn", N, 64, 704, 5, 7),           # nk = 11, odd
    "wide_randn_6411_768_k5": ("randn", N, 64, 768, 5, 7),           # nk = 12
    "wide_randn_6411_768_k10": ("randn", N, 64, 768, 10, 7),
    "wide_randn_6411_1000_k5": ("randn", N, 64, 1000, 5, 7),         # nk = 16, padded to 1024
    "wide_randn_6411_1024_k5": ("randn", N, 64, 1024, 5, 7),
    "wide_randn_6411_2048_k5": ("randn", N, 64, 2048, 5, 7),         # nk = 32
    "wide_randn_6411_2048_k10": ("randn", N, 64, 2048, 10, 7),
    "wide_manifold_6411_4096_k5": ("manifold", N, 64, 4096, 5, 28),  # nk = 64 (randn is a check-A case there: test_gpu_routes.py)
    "wide_unit_6411_768_k5": ("unit", N, 64, 768, 5, 7),
    "wide_randn_6400_768_k5": ("randn", 6400, 64, 768, 5, 7),        # no ragged block
    "wide_randn_6145_768_k5": ("randn", 6145, 64, 768, 5, 7),        # a last block of ONE row
}
COUNTS = {
    "wide_counts_randn_513": ("randn", NR, NC, 513, 5, 31),
    "wide_counts_randn_576": ("randn", NR, NC, 576, 5, 31),
    "wide_counts_randn_768": ("randn", NR, NC, 768, 5, 31),
    "wide_counts_randn_1024": ("randn", NR, NC, 1024, 5, 31),
    "wide_counts_randn_2048": ("randn", NR, NC, 2048, 5, 31),
    "wide_counts_manifold_3328": ("manifold", NR, NC, 3328, 5, 31),  # the widest membership filter (verify_lds limit)
    # the grouped block order of plan_cross_fast (grp_rows = 8): few row blocks, then few column tiles
    "wide_counts_randn_1100x16000_768": ("randn", 1100, 16000, 768, 5, 33),
    "wide_counts_randn_16000x1100_768": ("randn", 16000, 1100, 768, 5, 35),
}
# name: tuple as above + (expected k-NN route, expected membership route); None = not asserted
ROUTES = {
    "wide_silence_6411_768": ("silence", N, N, 768, 5, 26, "marking", None),
    "wide_clustered_6411_768": ("clustered", N, N, 768, 5, 3, "check A", None),
    "wide_tiny_6411_768": ("tiny", N, N, 768, 5, 12, "scale", "scale"),
    "wide_shared_6411_768": ("shared", N, N, 768, 5, 4, None, "budget"),
    "wide_overflow_6411_768": ("overflow", N, N, 768, 5, 830, None, "overflow"),
}


@pytest.fixture(scope="module")
def probe():
    import audio_metrics_amd
    audio_metrics_amd._lib.load()
    import route_probe
    route_probe.ops.filter_stats_enable("cuda:0", True)
    yield route_probe
    route_probe.ops.filter_stats_enable("cuda:0", False)


@pytest.fixture(scope="module")
def sets(probe):
    """(family, rows, rows2, dim, seed) -> (set, second set), built once and never written to."""
    from test_gpu_routes import sets_of
    cache = {}

    def get(fam, n, n2, d, seed):
        key = (fam, n, n2, d, seed)
        if key not in cache:
            cache[key] = probe.overflow_sets(n, d, seed) if fam == "overflow" else tuple(sets_of(probe, fam, n, n2, d, seed))
        return cache[key]
    return get


@pytest.fixture(scope="module")
def exact(probe, sets):
    """(family, rows, rows2, dim, seed), k -> the exact general kernel's radii of the first set, computed once."""
    cache = {}

    def get(key, k):
        if (key, k) not in cache:
            cache[(key, k)] = probe.exact_radii(sets(*key)[0], k)
        return cache[(key, k)]
    return get


def same_bits(a, b):
    return torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


# ----------------------------------------------------------------- 0. selection boundaries (no kernel runs)
def test_selection_boundaries(probe):
    ops = probe.ops
    assert ops.filter_engine(512) == 1 and ops.filter_engine(513) == 0 and ops.filter_engine(4096) == 0
    assert ops.knn_path(N, N, 4096, 5) == 3 and ops.knn_path(N, N, 4097, 5) != 3
    # the membership filter's verification tile: 16 ceil(D / 8) 8 + 8192 <= 61440 bytes of LDS
    assert ops.prdc_path(NR, NC, 3328) == 3 and ops.prdc_path(NR, NC, 3329) == 0
    assert ops.knn_path(N, N, 768, 11) == 2                      # k > 10 leaves the 256-row engine


def test_case_tables_agree_with_the_probe(probe):
    for table in (RADII, COUNTS, ROUTES):
        for name, case in table.items():
            assert probe.CASES[name] == case[:6], name


# ----------------------------------------------------------------- 1. radii over the slab counts
@pytest.mark.parametrize("name", list(RADII))
def test_radii(probe, sets, exact, name):
    fam, n, n2, d, k, seed = RADII[name]
    ops = probe.ops
    x = sets(fam, n, n2, d, seed)[0]
    assert ops.knn_path(n, n, d, k) == 3 and ops.filter_engine(d) == 0
    ops.filter_stats_read("cuda:0")
    r = ops.knn_radii(x, k)
    s = ops.filter_stats_read("cuda:0")
    print(f"{name}: queued {s['knn_queued']}, verified {s['knn_verified_pairs']}, fallback rows {s['knn_fallback_rows']}, "
          f"|a - t| / bound <= {s['bound_ratio_max']:.3f} over {s['bound_pairs']} pairs")
    assert same_bits(r, exact((fam, n, n2, d, seed), k)), "radii differ from the exact kernel's"
    # the sweep decided the call: a whole-call fallback (check A, check B, scale) reports n fallback rows
    assert s["knn_queued"] > 0 and s["knn_verified_pairs"] > 0 and s["knn_fallback_rows"] < n // 8, s
    assert s["bound_pairs"] > 0 and 0.0 <= s["bound_ratio_max"] <= 1.0, s


# ----------------------------------------------------------------- 2. membership counts
@pytest.fixture(scope="module")
def count_sets(probe, sets):
    """name -> (reference set, candidate set, their k = 5 radii), once per module."""
    cache = {}

    def get(name):
        if name not in cache:
            fam, n, n2, d, k, seed = COUNTS[name]
            x, y = sets(fam, n, n2, d, seed)
            cache[name] = (x, y, probe.ops.knn_radii(x, k), probe.ops.knn_radii(y, k))
        return cache[name]
    return get


@pytest.mark.parametrize("want_min", [False, True])
@pytest.mark.parametrize("name", list(COUNTS))
def test_membership_counts(probe, count_sets, name, want_min):
    fam, n, n2, d, k, seed = COUNTS[name]
    ops = probe.ops
    x, y, r, r2 = count_sets(name)
    assert ops.prdc_path(n, n2, d) == 3 and ops.filter_engine(d) == 0
    ops.filter_stats_read("cuda:0")
    got = ops.prdc_counts(x, y, r, r2, want_min=want_min)
    s = ops.filter_stats_read("cuda:0")
    print(f"{name} want_min={want_min}: queued {s['prdc_queued']}, through the overflow queue {s['prdc_overflow_queue']}")
    assert s["prdc_calls"] == 1 and s["prdc_fallback_calls"] == 0 and s["prdc_queued"] > 0, s
    want = probe.exact_counts(x, y, r, r2, want_min)
    assert len(got) == len(want) == (4 if want_min else 3)
    for a, b in zip(got, want):
        assert same_bits(a, b)


# ----------------------------------------------------------------- 3. the data-dependent routes on this engine
@pytest.mark.parametrize("name", list(ROUTES))
def test_route_and_bits(probe, sets, name):
    fam, n, n2, d, k, seed, knn_route, cross_route = ROUTES[name]
    ops = probe.ops
    x, y = sets(fam, n, n2, d, seed)
    assert ops.knn_path(n, n, d, k) == 3 and ops.prdc_path(n, n2, d) == 3 and ops.filter_engine(d) == 0
    ops.filter_stats_read("cuda:0")
    r = ops.knn_radii(x, k)
    s = ops.filter_stats_read("cuda:0")
    print(f"{name}: k-NN queued {s['knn_queued']}, verified {s['knn_verified_pairs']}, fallback rows {s['knn_fallback_rows']}, "
          f"|a - t| / bound <= {s['bound_ratio_max']:.3f} over {s['bound_pairs']} pairs")
    assert same_bits(r, probe.exact_radii(x, k)), "radii differ from the exact kernel's"
    if s["bound_pairs"] > 0:
        assert 0.0 <= s["bound_ratio_max"] <= 1.0, s
    if knn_route == "plain":
        assert s["knn_fallback_rows"] == 0 and s["knn_verified_pairs"] > 0 and s["bound_pairs"] == s["knn_verified_pairs"], s
    elif knn_route in ("check A", "scale"):
        assert s["knn_fallback_rows"] == n, s                               # the exact general kernel took every row
        if knn_route == "check A":
            assert s["knn_queued"] == 0, s                                  # ... before the sweep queued anything
    elif knn_route == "marking":
        assert 32 <= s["knn_fallback_rows"] < n // 8 and s["knn_verified_pairs"] > 0, s    # the identical block: batched fix-up
    r2 = ops.knn_radii(y, k)
    if fam == "overflow":
        r = probe.overflow_radii(x, y, r)
    ops.filter_stats_read("cuda:0")
    want_min = seed % 2 == 1
    got = ops.prdc_counts(x, y, r, r2, want_min=want_min)
    s = ops.filter_stats_read("cuda:0")
    print(f"{name}: membership queued {s['prdc_queued']}, through the overflow queue {s['prdc_overflow_queue']}, "
          f"fallback calls {s['prdc_fallback_calls']}")
    want = probe.exact_counts(x, y, r, r2, want_min)
    for a, b in zip(got, want):
        assert same_bits(a, b)
    assert s["prdc_calls"] == 1, s
    if cross_route == "overflow":
        assert s["prdc_fallback_calls"] == 0 and s["prdc_overflow_queue"] > 0, s
    elif cross_route in ("budget", "scale"):
        assert s["prdc_fallback_calls"] == 1, s
        if cross_route == "budget":
            assert s["prdc_overflow_queue"] > 0, s


# ----------------------------------------------------------------- 4. the partitioned sweep (no check A / B: the sweep always runs)
@pytest.mark.parametrize("fam,rows,dim,k,world,seed", [
    ("randn", N, 576, 5, 3, 7), ("unit", N, 1024, 10, 2, 7),
    ("randn", N, 4096, 5, 2, 7)])          # 64 slabs on data the one-GPU form hands to check A
def test_partitioned_sweep(probe, sets, exact, fam, rows, dim, k, world, seed):
    ops = probe.ops
    x = sets(fam, rows, 64, dim, seed)[0]
    assert ops.knn_sym_eligible(rows, dim, k) and ops.knn_path(rows, rows, dim, k) == 3 and ops.filter_engine(dim) == 0
    want = ops.knn_radii(x, k)
    shards = [(rows * p // world, rows * (p + 1) // world) for p in range(world)]
    bounds = torch.cat([ops.knn_bounds(x, k, lo, hi - lo) for lo, hi in shards])
    ops.filter_stats_read("cuda:0")
    lists = torch.stack([ops.knn_sym_part(x, k, p, world, bounds) for p in range(world)])
    s = ops.filter_stats_read("cuda:0")
    print(f"{fam} {rows} x {dim} k={k} in {world} parts: queued {s['knn_queued']}, verified {s['knn_verified_pairs']}")
    assert s["knn_calls"] == world and s["knn_queued"] > 0 and s["knn_verified_pairs"] > 0, s    # every rank's share of the sweep ran
    got = ops.knn_lists_finish(lists, x, k)
    assert same_bits(got, want)
    assert same_bits(got, exact((fam, rows, 64, dim, seed), k))


# ----------------------------------------------------------------- 5. prepared sets and the fused call at D = 768
def test_prepared_sets_change_no_bit(probe, sets):
    ops = probe.ops
    k, n2 = 5, 6300
    x, y = sets("randn", N, n2, 768, 7)
    px, py = ops.prepare(x), ops.prepare(y)
    ops.filter_stats_read("cuda:0")
    rx, ry = ops.knn_radii(x, k), ops.knn_radii(y, k)
    s = ops.filter_stats_read("cuda:0")
    assert s["knn_calls"] == 2 and s["knn_queued"] > 0 and s["knn_fallback_rows"] < n2 // 8, s       # both on the filter
    assert same_bits(rx, ops.knn_radii(x, k, prepared=px)) and same_bits(ry, ops.knn_radii(y, k, prepared=py))
    s = ops.filter_stats_read("cuda:0")
    assert s["knn_calls"] == 2 and s["knn_queued"] > 0 and s["knn_fallback_rows"] < n2 // 8, s
    plain = ops.prdc_counts(x, y, rx, ry)
    shared = ops.prdc_counts(x, y, rx, ry, prepared_ref=px, prepared_cand=py)
    assert all(same_bits(a, b) for a, b in zip(plain, shared))
    lo, hi = 1000, 3700                                            # a row shard that stays on the filter: 2700 x 6300 >= 2^24
    assert (hi - lo) * n2 >= 2 ** 24 and ops.prdc_path(hi - lo, n2, 768) == 3
    part = ops.prdc_counts(x[lo:hi], y, rx[lo:hi], ry, prepared_ref=px.rows(lo, hi), prepared_cand=py)
    want = ops.prdc_counts(x[lo:hi], y, rx[lo:hi], ry)
    assert all(same_bits(a, b) for a, b in zip(part, want))
    s = ops.filter_stats_read("cuda:0")
    assert s["prdc_calls"] == 4 and s["prdc_fallback_calls"] == 0, s
    assert all(same_bits(a, b) for a, b in zip(plain, probe.exact_counts(x, y, rx, ry)))


def test_fused_evaluate_equals_separate_entry_points(probe, sets):
    from audio_metrics_amd.distributed import evaluate_sharded
    ref, cand = sets("randn", N, 6300, 768, 7)
    fused = evaluate_sharded(ref, cand, metrics=("prdc",), nearest_k=5)
    apart = evaluate_sharded(ref, cand, metrics=("prdc",), nearest_k=5, fused=False)
    assert list(fused) == ["precision", "recall", "density", "coverage"]
    assert fused == apart


# ----------------------------------------------------------------- 6. float64 rows through the filter
@pytest.mark.parametrize("fam,rows,rows2,dim,k,seed", [("randn", N, 6300, 768, 5, 41), ("unit", N, 6300, 1024, 10, 42), ("dups", N, N, 768, 5, 43)])
def test_f64_rows(probe, fam, rows, rows2, dim, k, seed):
    """tools/fuzz_f64.py's case body, as test_f64_slice runs it at D <= 128: radii to the rounding of two summation orders,
    counts and flags exactly."""
    import fuzz_f64
    ok_r, ok_c, line = fuzz_f64.run_case(fam, rows, rows2, dim, k, seed)
    print(line)
    assert ok_r and ok_c, line


# ----------------------------------------------------------------- 7. the oracle itself at these widths, against float64 on the CPU
def d2_f64(x, y):
    """|x|^2 + |y|^2 - 2 x y^T in float64 on the CPU, and the two vectors of squared norms"""
    xd, yd = x.cpu().double(), y.cpu().double()
    nx, ny = xd.square().sum(1), yd.square().sum(1)
    d2 = xd @ yd.T
    d2.mul_(-2.0).add_(nx[:, None]).add_(ny[None, :]).clamp_(min=0.0)
    return d2, nx, ny


def test_exact_radii_against_float64(sets, exact):
    """An f32 squared distance of the exact kernels (fma(-2, <x, y>, |x|^2 + |y|^2), every sum a chain of D f32 roundings at
    the most) lies within delta_ij = 2 (D + 2) 2^-24 (|x_i|^2 + |x_j|^2) of the float64 one, and an order statistic moves by at
    most the largest perturbation in its row: |r32^2 - r64^2| <= max_j delta_ij + one ulp of r32^2 for the square root."""
    d, k = 768, 5
    key = ("randn", N, 64, d, 7)
    r32 = exact(key, k).cpu()
    x = sets(*key)[0]
    d2, nx, _ = d2_f64(x, x)
    r64sq = torch.kthvalue(d2, k + 1, dim=1).values
    delta = 2.0 * (d + 2) * 2.0 ** -24 * (nx + nx.max())
    sq32 = r32 * r32
    ulp = (torch.nextafter(sq32, torch.full_like(sq32, float("inf"))) - sq32).double()
    err = (r32.double().square() - r64sq).abs()
    print(f"exact radii, 6411 x 768: largest |r32^2 - r64^2| / bound = {float((err / (delta + ulp)).max()):.4f}")
    assert bool((err <= delta + ulp).all())


def test_exact_counts_against_float64(probe, count_sets):
    """sure_j <= col_count_j <= maybe_j with T_i = r_i^2: sure counts the pairs with d2_64 < T_i - delta_ij, maybe those with
    d2_64 <= T_i + delta_ij (delta as above)."""
    d = 768
    x, y, r, r2 = count_sets("wide_counts_randn_768")
    col = probe.exact_counts(x, y, r, r2)[0].cpu().long()
    d2, nx, ny = d2_f64(x, y)
    delta = 2.0 * (d + 2) * 2.0 ** -24 * (nx[:, None] + ny[None, :])
    thr = r.cpu().double().square()[:, None]
    sure = (d2 < thr - delta).sum(0)
    maybe = (d2 <= thr + delta).sum(0)
    print(f"exact counts, 4111 x 4203 x 768: sure {int(sure.sum())} <= counted {int(col.sum())} <= maybe {int(maybe.sum())}")
    assert int(col.sum()) > 0
    assert bool((sure <= col).all()) and bool((col <= maybe).all())
