"""Timing probe of the retrieval ranks on one GPU (HIP events, warm, the median of alternating calls):

  am_retrieval_ranks_f32 (norms, weights, positives pass, sweep, merge: the whole entry) at 100 000 x 100 000 rows of 512 and
  128 columns, paired, cosine, beside
    torch     a blocked torch composition of the same counts in the same run:
              ((q_blk @ g.T) * w > t_blk[:, None]).sum(1) plus the == count, 4096 query rows per block.  The bar: the
              library is not slower
    psr       am_psr_f32 on the same matrices (the neighbouring epilogue of the same engine), for information

    python tools/retrieval_probe.py            # writes profiles/retrieval/probe.txt
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_metrics_amd as am                                          # noqa: E402
from audio_metrics_amd import hip_ops as ops                            # noqa: E402

DEV = torch.device("cuda", 0)
F32_MFMA_PEAK = 157.3e12                                                # flop/s, dense f32 matrix cores of one MI355X
SHAPES = ((100_000, 100_000, 512), (100_000, 100_000, 128))
BLOCK = 4096


def paired_rows(seed, n, d):
    """Queries and a gallery whose row i leans towards query i: ranks spread from 1 to thousands."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    q = torch.randn((n, d), generator=gen, device=DEV)
    g = torch.randn((n, d), generator=gen, device=DEV)
    a = torch.linspace(0.0, 0.5, n, device=DEV)[:, None]
    return q, a * q + (1.0 - a) * g


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(fns, calls):
    """Median (and range) per call of several functions timed call by call, in turn."""
    for _ in range(2):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(calls):
        for t, fn in zip(times, fns):
            t.append(event_ms(fn))
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in times]


def library_call(lib, q, g):
    n, d = q.shape
    m = g.shape[0]
    start = torch.arange(n, dtype=torch.int64, device=DEV)
    count = torch.ones(n, dtype=torch.int64, device=DEV)
    out = [torch.empty(n, dtype=t, device=DEV) for t in (torch.int32, torch.int32, torch.float32, torch.int64, torch.int32, torch.int32)]
    nb = lib.am_retrieval_workspace_bytes(n, m, d)
    ws = ops._workspace(nb, DEV)

    def run():
        ops._call(lib, "am_retrieval_ranks_f32", DEV, ops._ptr(q), n, ops._ld(q), ops._ptr(g), m, ops._ld(g), d, 1, ops._ptr(start),
                  ops._ptr(count), ops._ptr(start), n, None, None, *(ops._ptr(t) for t in out), ops._ptr(ws), nb)
    return run, out, nb, (start, count, ws)


def torch_call(q, g):
    n = q.shape[0]
    better = torch.empty(n, dtype=torch.int64, device=DEV)
    tied = torch.empty(n, dtype=torch.int64, device=DEV)

    def run():
        w = 1.0 / torch.linalg.vector_norm(g, dim=1)
        for s in range(0, n, BLOCK):
            u = (q[s:s + BLOCK] @ g.T) * w
            tb = torch.diagonal(u, offset=s)[:, None]                   # the block's own positives: the GEMM's bits, as the compare needs
            better[s:s + BLOCK] = (u > tb).sum(1)
            tied[s:s + BLOCK] = (u == tb).sum(1) - 1                    # (the positive itself)
    return run, better, tied


def psr_call(lib, x, y, radius):
    n, d = x.shape
    m = y.shape[0]
    psr = torch.empty(n, dtype=torch.float64, device=DEV)
    count = torch.empty(n, dtype=torch.int32, device=DEV)
    nb = lib.am_psr_workspace_bytes(n, m, d)
    ws = ops._workspace(nb, DEV)

    def run():
        ops._call(lib, "am_psr_f32", DEV, ops._ptr(x), n, ops._ld(x), ops._ptr(y), m, ops._ld(y), d, float(radius), ops._ptr(psr),
                  ops._ptr(count), None, ops._ptr(ws), nb)
    return run, (psr, count, ws)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=11, help="timed calls per function; the median is printed")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "retrieval"))
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    lib = am._lib.load()
    lines = [f"# {torch.cuda.get_device_name(0)}; HIP events, warm, median of {args.calls} alternating calls, one process; paired rows, "
             f"cosine; torch = ((q_blk @ g.T) * w > t_blk[:, None]).sum(1) and the == count, {BLOCK} query rows per block; bar: "
             "library / torch <= 1"]
    for n, m, d in SHAPES:
        q, g = paired_rows(n + d, n, d)
        run_l, out, nb, keep_l = library_call(lib, q, g)
        run_t, better_t, tied_t = torch_call(q, g)
        run_p, keep_p = psr_call(lib, q, g, 0.5 * (2.0 * d) ** 0.5)         # few pairs in range: the compare-only epilogue
        (t_l, lo_l, hi_l), (t_t, lo_t, hi_t), (t_p, lo_p, hi_p) = alternate([run_l, run_t, run_p], args.calls)
        better = out[0].to(torch.int64)
        agree = float((better == better_t).double().mean())                # torch's GEMM rounds otherwise: close, not equal
        flop = 2.0 * n * m * d
        line = (f"{n} x {m} x {d}: am_retrieval_ranks_f32 {t_l:9.3f} ms ({lo_l:.3f} .. {hi_l:.3f})  torch {t_t:9.3f} ms "
                f"({lo_t:.3f} .. {hi_t:.3f})  library / torch {t_l / t_t:5.3f} (bar <= 1)  am_psr_f32 {t_p:9.3f} ms "
                f"({lo_p:.3f} .. {hi_p:.3f})  library / psr {t_l / t_p:5.3f}  library at "
                f"{100 * flop / F32_MFMA_PEAK / (t_l * 1e-3):.0f} % of the f32 matrix peak, {lib.am_retrieval_chunks(n, m, d)} column "
                f"chunks, workspace {nb / 2 ** 20:.1f} MiB; median rank {int(better.median()) + 1}, recall@1 "
                f"{float((better == 0).double().mean()):.4f}, ties {int(out[1].sum())}, rows with torch's count {agree:.4f}")
        lines.append(line)
        print(line, flush=True)
        del q, g, keep_l, keep_p, out, better_t, tied_t
        torch.cuda.empty_cache()
    with open(os.path.join(args.out_dir, "probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
