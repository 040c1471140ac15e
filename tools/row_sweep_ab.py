"""A/B of the row-sweep entry points between two builds of the library, one build per process.

    AM_HIP_LIBRARY=libam_parent.so python tools/row_sweep_ab.py run --out parent_1.json
    python tools/row_sweep_ab.py run --out change_1.json                     # ... and once more each, alternating
    python tools/row_sweep_ab.py run --edge --out change_edge.json           # the row-block / inner-tail edge shapes
    python tools/row_sweep_ab.py compare --parent parent_1.json parent_2.json --change change_1.json change_2.json \\
        --edge parent_edge.json change_edge.json --out-dir profiles/row_sweep

`run` loads the library AM_HIP_LIBRARY names (audio_metrics_amd._lib) and calls every entry point whose kernels or host
side go through csrc/row_sweep.h - the search at k = 5, 16 and 32 (the three list lengths), the k-means assign, the
per-sample scores, the soft-min, the scoring rule, both sweeps of the feature likelihood divergence (the gradient on the same
rows against the same centres), the sliced projection and the random Fourier features - on seeded rows: 13 calls each, the
last 11 timed with HIP events, and a SHA-256 of every output buffer.  Never two builds in one process: they export the
same symbols.  Both builds must see the same environment (the chunk plan decides the last bits of the f64 sums).

`compare` checks that every hash of the change equals the parent's and holds the change's medians against the bar
median(change) <= median(parent) (1 + s), s = the larger of the relative gap between the two parent processes' medians
and the parent's (max - min) / median inside a process: the parent's own spread."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BIG = ((100_000, 100_000, 512), (100_000, 100_000, 128))
EDGE = ((130, 300, 40), (257, 130, 64), (129, 257, 40), (130, 4000, 40))
WARM, TIMED = 2, 11
PROJECTIONS = 256                                                        # directions / frequencies of the two store-only sweeps


def run(args):
    import torch
    import audio_metrics_amd as am
    from audio_metrics_amd import hip_ops as ops

    dev = torch.device("cuda", 0)
    am._lib.load()
    result = {"library": am._lib.library_path(), "device": torch.cuda.get_device_name(0), "timed_calls": TIMED, "cases": {}}

    def randn(seed, *shape):
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        return torch.randn(shape, generator=g, device=dev)

    def sha(t):
        return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()

    def measure(name, shape, fn):
        out = None
        for _ in range(WARM):
            out = fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(TIMED):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        out = out if isinstance(out, (tuple, list)) else (out,)
        key = f"{name} {shape[0]} x {shape[1]} x {shape[2]}"
        result["cases"][key] = {"median_ms": sorted(ms)[TIMED // 2], "min_ms": min(ms), "max_ms": max(ms),
                                "sha256": [sha(t) for t in out if t is not None]}
        print(key, result["cases"][key]["median_ms"], flush=True)
        return out

    for shape in (EDGE if args.edge else BIG):
        n, m, d = shape
        x, y = randn(1, n, d), randn(2, m, d) + 0.25
        radii = ops.knn_radii(y, 5) if m > 5 else torch.ones(m, device=dev)
        radius = 1.2 * float(radii.to(torch.float64).mean())
        g = randn(3, m).to(torch.float64) * d
        theta = (randn(4, m).to(torch.float64) * 0.5).clamp(-3.0, 3.0) + 1.0
        for k in (5, 16, 32):
            measure(f"am_knn_search_f32 k={k}", shape, lambda: ops.knn_search(x, y, k))
        measure("am_kmeans_assign_f32", shape, lambda: ops.kmeans_assign(x, y))
        measure("am_sample_scores_f32", shape, lambda: ops.sample_scores(x, y, radii))
        measure("am_softmin_f32", shape, lambda: ops.softmin(x, y, g, eps=float(d)))
        measure("am_psr_f32", shape, lambda: ops.psr_scores(x, y, radius))
        ll, stats = measure("am_fld_loglik_f32", shape, lambda: ops.fld_loglik(x, y, theta))
        zeros = torch.zeros(m, dtype=torch.float64, device=dev)
        measure("am_fld_grad_f32", shape, lambda: ops.fld_grad_step(y, x, theta, ll, stats[1:2], zeros, zeros, 1, 0.5, -10.0))
        w = randn(5, PROJECTIONS, d)
        measure("am_sliced_project_f32", (n, PROJECTIONS, d), lambda: ops.sliced_project(x, w))
        measure("am_rff_features_f32", (n, PROJECTIONS, d), lambda: ops.rff_features(x, w, inv_bw=1.0 / (2.0 * d) ** 0.5))
        del x, y, w
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


def compare(args):
    def load(path):
        with open(path) as f:
            return json.load(f)
    parents, changes = [load(p) for p in args.parent], [load(p) for p in args.change]
    assert len(parents) == 2 and len(changes) == 2, "two processes per build"
    os.makedirs(args.out_dir, exist_ok=True)
    ok = True

    pairs = [(parents[0], r) for r in (parents[1], *changes)]
    names = [f"{os.path.basename(args.parent[0])} = {os.path.basename(p)}" for p in (args.parent[1], *args.change)]
    if args.edge:
        pairs.append((load(args.edge[0]), load(args.edge[1])))
        names.append(f"{os.path.basename(args.edge[0])} = {os.path.basename(args.edge[1])}")
    bits = [f"# SHA-256 of every output buffer of every entry point and shape, build against build ({parents[0]['device']})",
            f"# parent library: {os.path.basename(parents[0]['library'])}   change library: {os.path.basename(changes[0]['library'])}"]
    for (a, b), name in zip(pairs, names):
        assert sorted(a["cases"]) == sorted(b["cases"]), name
        bad = [k for k in a["cases"] if a["cases"][k]["sha256"] != b["cases"][k]["sha256"]]
        buffers = sum(len(c["sha256"]) for c in a["cases"].values())
        bits.append(f"{name}: {len(a['cases'])} entry points x shapes, {buffers} buffers, " +
                    ("all equal" if not bad else "DIFFERENT: " + "; ".join(bad)))
        ok = ok and not bad
    with open(os.path.join(args.out_dir, "bits.txt"), "w") as f:
        f.write("\n".join(bits) + "\n")
    print("\n".join(bits))

    lines = [f"# {parents[0]['device']}; HIP events, {parents[0]['timed_calls']} warm calls per entry point and process, four fresh "
             "processes in the order parent, change, parent, change",
             "# bar: median(change) <= median(parent) (1 + s); s = max(relative gap of the two parent processes' medians, the parent's "
             "(max - min) / median inside a process); medians of a build = the mean of its two processes' medians",
             f"# {'entry point and shape':46s} {'parent ms':>21s} {'change ms':>21s} {'ratio':>7s} {'s':>7s}  verdict"]
    for key in parents[0]["cases"]:
        p, c = [r["cases"][key] for r in parents], [r["cases"][key] for r in changes]
        pm, cm = [q["median_ms"] for q in p], [q["median_ms"] for q in c]
        gap = abs(pm[0] - pm[1]) / min(pm)
        spread = max((q["max_ms"] - q["min_ms"]) / q["median_ms"] for q in p)
        s = max(gap, spread)
        pmed, cmed = sum(pm) / 2, sum(cm) / 2
        inside = cmed <= pmed * (1.0 + s)
        ok = ok and inside
        lines.append(f"{key:48s} {pm[0]:10.3f} {pm[1]:10.3f} {cm[0]:10.3f} {cm[1]:10.3f} {cmed / pmed:7.4f} {s:7.4f}  "
                     f"{'inside' if inside else 'OUTSIDE'}")
    with open(os.path.join(args.out_dir, "timing.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    r = sub.add_parser("run")
    r.add_argument("--out", required=True)
    r.add_argument("--edge", action="store_true", help="the edge shapes in place of the two probe shapes")
    c = sub.add_parser("compare")
    c.add_argument("--parent", nargs=2, required=True)
    c.add_argument("--change", nargs=2, required=True)
    c.add_argument("--edge", nargs=2, help="parent and change runs at the edge shapes")
    c.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "row_sweep"))
    args = ap.parse_args()
    sys.exit(run(args) if args.mode == "run" else compare(args))


if __name__ == "__main__":
    main()
