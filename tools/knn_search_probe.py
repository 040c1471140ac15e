"""Timing probe of the nearest-neighbour search on one GPU (HIP events, warm): am_knn_search_f32 beside am_knn_radii_f32 on
the same two DISTINCT sets - the exact general kernel doing the same Gram work with value-only lists - alternating, so that
the ratio shows what carrying the column through the lists costs.

    python tools/knn_search_probe.py > profiles/knn_search/probe.txt
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audio_metrics_amd as am                                          # noqa: E402
from audio_metrics_amd import hip_ops as ops                            # noqa: E402

DEV = torch.device("cuda", 0)
F32_MFMA_PEAK = 157.3e12                                                # flop/s, dense f32 matrix cores of one MI355X


def rows(seed, n, d, shift):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    x = torch.randn((n, d), generator=g, device=DEV) + shift
    return x / x.norm(dim=1, keepdim=True)                              # CLAP-like: offset Gaussian, unit norm


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--small", type=int, default=1_000)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of (radii, search); the median is printed")
    ap.add_argument("--min-ms", type=float, default=200.0, help="least work per timed window")
    args = ap.parse_args()
    lib = am._lib.load()
    print(f"# {torch.cuda.get_device_name(0)}; HIP events, warm, median of {args.rounds} alternating windows of >= {args.min_ms:.0f} ms")
    print("# radii: am_knn_radii_f32(X, Y != X, nearest_k = k) - exact general kernel, k + 1 float list slots (6 / 11 / 16 / 32)")
    print("# search: am_knn_search_f32(X, Y, k) - the same Gram work, k key slots (8 / 16 / 32), distances and indices")
    for d in (512, 128):
        y = rows(1, args.rows, d, 0.5)
        for n in (args.rows, args.small):
            x = rows(2, n, d, 0.55)
            m = y.shape[0]
            flop = 2.0 * n * m * d
            for k in (1, 5, 16):
                radii = torch.empty(n, dtype=torch.float32, device=DEV)
                dist = torch.empty((n, k), dtype=torch.float32, device=DEV)
                idx = torch.empty((n, k), dtype=torch.int64, device=DEV)
                nb_r, nb_s = lib.am_knn_workspace_bytes(n, m, d, k), lib.am_knn_search_workspace_bytes(n, m, d, k)
                ws_r, ws_s = ops._workspace(nb_r, DEV), ops._workspace(nb_s, DEV)
                assert ops.knn_path(n, m, d, k, self_distance=False) == 0          # the exact general kernel

                def run_radii():
                    ops._call(lib, "am_knn_radii_f32", DEV, ops._ptr(x), n, ops._ld(x), ops._ptr(y), m, ops._ld(y), d, k,
                              ops._ptr(radii), ops._ptr(ws_r), nb_r)

                def run_search():
                    ops._call(lib, "am_knn_search_f32", DEV, ops._ptr(x), n, ops._ld(x), ops._ptr(y), m, ops._ld(y), d, k, -1, 0,
                              ops._ptr(dist), ops._ptr(idx), ops._ptr(ws_s), nb_s)
                run_radii()                                                         # warm both
                run_search()
                torch.cuda.synchronize()
                reps = max(2, int(args.min_ms / max(event_ms(run_radii, 2), 1e-3)) + 1)
                tr, ts = [], []
                for _ in range(args.rounds):
                    tr.append(event_ms(run_radii, reps))
                    ts.append(event_ms(run_search, reps))
                t_r, t_s = sorted(tr)[len(tr) // 2], sorted(ts)[len(ts) // 2]
                # same values: the k-th column of a k-search is the radius of nearest_k = k - 1; here the (k+1)-th is not kept,
                # so compare what both hold - the search's last column against the radii of nearest_k = k - 1 when k > 1
                agree = ""
                if k > 1:
                    r_prev = ops.knn_radii(x, k - 1, columns=y)
                    agree = f"  last column == radii(k - 1): {bool(torch.equal(dist[:, k - 1].view(torch.int32), r_prev.view(torch.int32)))}"
                print(f"{n:7d} x {d} against {m} x {d}, k = {k:2d}: radii {t_r:8.3f} ms ({min(tr):.3f} .. {max(tr):.3f})  "
                      f"search {t_s:8.3f} ms ({min(ts):.3f} .. {max(ts):.3f})  ratio {t_s / t_r:5.2f}  "
                      f"search at {100 * flop / F32_MFMA_PEAK / (t_s * 1e-3):.0f} % of the f32 matrix peak, "
                      f"{lib.am_knn_search_chunks(n, m, d, k)} column chunks, {reps} calls per window{agree}")
            del x
        del y


if __name__ == "__main__":
    main()
