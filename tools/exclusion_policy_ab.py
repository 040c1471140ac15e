"""Bits of the four entry points behind the exclusion policies (csrc/knn_search.hip, csrc/sample_scores.hip) between two
builds of the library, one build per process (they export the same symbols):

    AM_HIP_LIBRARY=/abs/path/libam_parent.so python tools/exclusion_policy_ab.py run --out parent.json
    python tools/exclusion_policy_ab.py run --out change.json
    python tools/exclusion_policy_ab.py compare parent.json change.json --out profiles/exclusion_policy/bits.txt

`run` calls am_knn_search_f32 (self_offset = 0) and am_knn_search_groups_f32 at k = 5, 16 and 32 (the three list lengths) and
am_sample_scores_f32 / am_sample_scores_groups_f32 on the seeded windowed rows of tools/knn_groups_probe.py and
tools/sample_scores_groups_probe.py - 100 000 rows in runs of 36 per song, in stored and in scattered order, at 512 and 128
columns and at 40 (the inner-dimension tail) - and writes a SHA-256 of every output buffer.  `compare` exits 0 iff every
hash of the second file equals the first's."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

WIDTHS = (512, 128, 40)
SEARCHES = ((5, True), (16, False), (32, True))                          # (k, squared)


def run(args):
    import numpy as np
    import torch
    import audio_metrics_amd as am
    from audio_metrics_amd import hip_ops as ops
    import knn_groups_probe as search_probe
    import sample_scores_groups_probe as scores_probe

    dev = torch.device("cuda", 0)
    am._lib.load()
    result = {"library": am._lib.library_path(), "device": torch.cuda.get_device_name(0), "cases": {}}

    def record(name, tensors):
        torch.cuda.synchronize()
        result["cases"][name] = [hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest() for t in tensors]
        print(name, len(tensors), "buffers", flush=True)

    for d in WIDTHS:
        n = search_probe.N
        rows, song = search_probe.windowed_rows(1, n, d)
        perm = torch.as_tensor(np.random.default_rng(2).permutation(n)).to(dev)
        for order, x, grp in (("runs", rows, song), ("scattered", ops.as_matrix(rows[perm]), song[perm].contiguous())):
            for k, squared in SEARCHES:
                record(f"knn_search {order} {n} x {n} x {d} k={k}", ops.knn_search(x, x, k, self_offset=0, squared=squared))
                record(f"knn_search_groups {order} {n} x {n} x {d} k={k}", ops.knn_search_groups(x, x, k, grp, grp, squared=squared))
        m = scores_probe.M
        y, gy = scores_probe.windowed_rows(1, 2, m, d)
        x, gx = scores_probe.windowed_rows(1, 3, m, d)
        radii = ops.knn_search_groups(y, y, scores_probe.K, gy, gy)[0][:, scores_probe.K - 1].contiguous()
        py = torch.as_tensor(np.random.default_rng(5).permutation(m)).to(dev)
        for order, xs, ys, rs, lx, ly in (("shared", x, y, radii, gx, gy),
                                          ("disjoint", x, y, radii, (gx + scores_probe.FAR).contiguous(), gy),
                                          ("scattered", ops.as_matrix(x[:1000]), ops.as_matrix(y[py]), radii[py].contiguous(),
                                           gx[:1000].contiguous(), gy[py].contiguous())):
            shape = f"{xs.shape[0]} x {m} x {d}"
            record(f"sample_scores {order} {shape}", ops.sample_scores(xs, ys, rs))
            record(f"sample_scores_groups {order} {shape}", ops.sample_scores_groups(xs, ys, rs, lx, ly))
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


def compare(args):
    with open(args.first) as f:
        a = json.load(f)
    with open(args.second) as f:
        b = json.load(f)
    lines = [f"# SHA-256 of every output buffer of am_knn_search_f32, am_knn_search_groups_f32, am_sample_scores_f32 and "
             f"am_sample_scores_groups_f32, build against build ({b['device']})",
             f"# first library: {os.path.basename(a['library'])}   second library: {os.path.basename(b['library'])}"]
    bad = sorted(set(a["cases"]) ^ set(b["cases"]))
    for name in sorted(set(a["cases"]) & set(b["cases"])):
        same = a["cases"][name] == b["cases"][name]
        bad += [] if same else [name]
        lines.append(f"{'equal ' if same else 'DIFFER'}  {name}: {len(a['cases'][name])} buffers")
    buffers = sum(len(v) for v in b["cases"].values())
    lines.append(f"{len(b['cases'])} calls, {buffers} buffers: " + ("all bits equal" if not bad else f"{len(bad)} call(s) DIFFER or are missing"))
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="command", required=True)
    r = sub.add_parser("run")
    r.add_argument("--out", required=True)
    c = sub.add_parser("compare")
    c.add_argument("first")
    c.add_argument("second")
    c.add_argument("--out")
    args = ap.parse_args()
    return run(args) if args.command == "run" else compare(args)


if __name__ == "__main__":
    sys.exit(main())
