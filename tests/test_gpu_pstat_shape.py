"""The stationary f16 filter engine at the widths whose kernels may run on the 16x16x32 MFMA (csrc/pstat_engine.h,
Pstat16Body; which instantiation takes it: PstatEng in csrc/pairwise_pstat.hip), and at the one width with exactly ONE slab
of the P rows in LDS (KSLABS = 7, D = 385 ... 448): there the engine's two-entry ring of LDS P fragments alternates between a
register slab and the LDS slab at the boundary.

Another MFMA shape means another register-to-(row, column) mapping in the epilogues and another accumulation order: the
approximate values and the queued pairs change, the results behind the exact re-evaluation may not.  Shapes are the smallest
that reach the kernels: 6411 rows (above the 6144-row threshold of D >= 256; the last row block holds 11 rows, so one 16-row
tile is partial and every other tile of that block is empty) for the radii, 4111 x 4203 (>= 2^24 pairs) for the membership
counts.  Random neighbours land on every one of the 64 x 32 (Q position, P position) slots of an accumulator tile pair about
19 times at these sizes, so a wrong mapping shows as a bit difference.  Exact values: tools/route_probe.py."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

WIDTHS = [512, 500]            # KSLABS = 8: two slabs of the P rows in LDS; 500 is padded to 512
WIDTHS7 = [448, 440]           # KSLABS = 7: one slab in LDS; 440 is padded to 448
N_RADII = 6411
NR, NC = 4111, 4203


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
    """(family, width) -> (reference set, candidate set, their exact k = 5 radii), built once."""
    cache = {}

    def get(fam, d):
        if (fam, d) not in cache:
            x, y = probe.make(fam, NR, d, 31), probe.make(fam, NC, d, 131)
            cache[(fam, d)] = (x, y, probe.ops.knn_radii(x, 5), probe.ops.knn_radii(y, 5))
        return cache[(fam, d)]
    return get


@pytest.mark.parametrize("k", [5, 10])
@pytest.mark.parametrize("d", WIDTHS + WIDTHS7)
@pytest.mark.parametrize("fam", ["randn", "unit"])
def test_radii(probe, fam, d, k):
    ops = probe.ops
    x = probe.make(fam, N_RADII, d, 7)
    assert ops.knn_path(N_RADII, N_RADII, d, k) == 3
    ops.filter_stats_read("cuda:0")
    r = ops.knn_radii(x, k)
    s = ops.filter_stats_read("cuda:0")
    print(f"{fam} {d} k={k}: queued {s['knn_queued']}, |a - t| / bound <= {s['bound_ratio_max']:.3f} over {s['bound_pairs']} pairs")
    assert s["knn_fallback_rows"] == 0, s
    assert torch.equal(r.view(torch.int32), probe.exact_radii(x, k).view(torch.int32)), "radii differ from the exact kernel's"
    assert s["bound_ratio_max"] <= 1.0, s


@pytest.mark.parametrize("want_min", [False, True])
@pytest.mark.parametrize("d", WIDTHS + WIDTHS7[:1])
@pytest.mark.parametrize("fam", ["randn", "unit"])
def test_membership_counts(probe, sets, fam, d, want_min):
    ops = probe.ops
    x, y, r, r2 = sets(fam, d)
    assert ops.prdc_path(NR, NC, d) == 3
    ops.filter_stats_read("cuda:0")
    got = ops.prdc_counts(x, y, r, r2, want_min=want_min)
    s = ops.filter_stats_read("cuda:0")
    print(f"{fam} {d} want_min={want_min}: queued {s['prdc_queued']}")
    assert s["prdc_fallback_calls"] == 0, s
    want = probe.exact_counts(x, y, r, r2, want_min)
    assert len(got) == len(want) == (4 if want_min else 3)
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
