"""The row-sharded evaluate with the REAL HIP kernels: two processes share cuda:0 and talk over
gloo (RCCL needs one GPU per rank, which the 1-GPU test box does not have).  Covers what the
CPU gloo test cannot: shard-vs-gathered-columns k-NN, cross counts on row shards, the collectives
on device tensors, unequal shard sizes."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import inputs as gi

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, n_ref, n_cand, d, k, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from audio_metrics_amd.distributed import evaluate_sharded, shard_bounds
    ref, cand = gi.pair("randn", 95, n_ref, n_cand, d)
    rl, rh = shard_bounds(n_ref, world, rank)
    cl, ch = shard_bounds(n_cand, world, rank)
    dev = torch.device("cuda:0")
    res = evaluate_sharded(torch.as_tensor(ref[rl:rh]).to(dev), torch.as_tensor(cand[cl:ch]).to(dev), nearest_k=k,
                           kid_subsets=8, kid_subset_size=300)
    out_q.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("n_ref,n_cand", [(2600, 2600), (2501, 2333)])
def test_sharded_evaluate_with_hip_kernels(n_ref, n_cand):
    import audio_metrics_amd as am
    from audio_metrics_amd.distributed import evaluate_sharded
    d, k, world = 96, 4, 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_ref, n_cand, d, k, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=240) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ref, cand = gi.pair("randn", 95, n_ref, n_cand, d)
    dev = torch.device("cuda:0")
    single = evaluate_sharded(torch.as_tensor(ref).to(dev), torch.as_tensor(cand).to(dev), nearest_k=k,
                              kid_subsets=8, kid_subset_size=300)
    assert results[0] == results[1]
    for key, w in single.items():
        if key in ("precision", "recall", "density", "coverage"):
            assert results[0][key] == w, key              # integer counts: identical whatever the sharding
        elif key == "fad":
            # the f32 product chains of the covariance kernel break at slab boundaries, which move with the
            # sharding: covariances agree to ~1e-7, and FAD amplifies that by trace/FAD
            assert abs(results[0][key] - w) <= 1e-5 * abs(w), (key, results[0][key], w)
        else:
            assert abs(results[0][key] - w) <= max(1e-9 * abs(w), 1e-12), (key, results[0][key], w)
    # and the single-process sharded path equals the object API
    a, b = am.AudioMetricsData(True), am.AudioMetricsData(True)
    a.add(torch.as_tensor(cand).to(dev))
    b.add(torch.as_tensor(ref).to(dev))
    assert am.prdc(b, a, k) == {key: single[key] for key in ("precision", "recall", "density", "coverage")}
    assert abs(am.frechet_distance(a, b) - single["fad"]) <= 1e-5 * abs(single["fad"])


@pytest.mark.parametrize("nparts,k,rows,path", [(2, 5, 9100, 3), (3, 10, 9100, 3), (8, 5, 9100, 3),
                                                (2, 5, 33100, 3), (5, 10, 33100, 3), (3, 20, 9100, 2)])
def test_partitioned_symmetric_knn_bit_identical(nparts, k, rows, path):
    """The multi-GPU form of the symmetric k-NN, emulated on one GPU: every part computed in turn, lists
    stacked as the all-gather would, then merged - bit-identical to the single-GPU result.  Both sizes take the f16 filter
    sweep + exact verification (path 3 on the 256-row engine; k = 20 needs 32-slot lists: the 128-row engine, path 2); the
    partitioned form of the EXACT symmetric kernel is covered by test_partitioned_exact_symmetric_kernel below."""
    import numpy as np
    from audio_metrics_amd import hip_ops as ops
    x = torch.as_tensor(gi.randn(97, rows, 136)).to("cuda:0")
    n = x.shape[0]
    assert ops.knn_sym_eligible(n, x.shape[1], k)
    assert ops.knn_path(n, n, x.shape[1], k) == path
    want = ops.knn_radii(x, k).cpu().numpy()
    bounds = torch.cat([ops.knn_bounds(x, k, lo, hi - lo) for lo, hi in
                        [(n * p // nparts, n * (p + 1) // nparts) for p in range(nparts)]])
    lists = torch.stack([ops.knn_sym_part(x, k, p, nparts, bounds) for p in range(nparts)])
    got = ops.knn_lists_finish(lists, x, k).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # a flagged row (NaN marker from any rank) is recomputed exactly
    lists[0, 17, 0] = float("nan")
    lists[nparts - 1, 4000, 0] = float("nan")
    got = ops.knn_lists_finish(lists, x, k).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("flagged", [1, 3, 31, 40, 300])
def test_few_flagged_rows_are_split_among_workgroups(flagged):
    """One workgroup streaming the whole set for ONE flagged row took 10 ms at 100 000 x 512 (100 ms at 1M): fewer flagged rows
    than the fix-up's grid has workgroups are split by columns among them (1 row: 256 slices, 3 rows: 85 each - a row count
    that does not divide - 31: 8 each); from 32 rows on the batched form takes over, a few hundred stay one workgroup each
    there.  Same radii as the one-GPU call, bit for bit, and the time of one row stays far below the single-workgroup form's."""
    import time
    import numpy as np
    from audio_metrics_amd import hip_ops as ops
    k, rows, d, nparts = 5, 20011, 200, 2
    x = torch.as_tensor(gi.randn(77, rows, d)).to("cuda:0")
    want = ops.knn_radii(x, k).cpu().numpy()
    bounds = torch.cat([ops.knn_bounds(x, k, lo, hi - lo) for lo, hi in
                        [(rows * p // nparts, rows * (p + 1) // nparts) for p in range(nparts)]])
    lists = torch.stack([ops.knn_sym_part(x, k, p, nparts, bounds) for p in range(nparts)])
    pick = np.random.default_rng(flagged).choice(rows, flagged, replace=False)
    lists[flagged % nparts, torch.as_tensor(pick, device="cuda:0"), 0] = float("nan")
    got = ops.knn_lists_finish(lists, x, k).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("kind,nparts", [("block", 3), ("hub", 4), ("flag_everything", 2)])
def test_partitioned_knn_with_identical_rows(kind, nparts):
    """Blocks of identical rows in the partitioned form: their rows overflow the ranks' candidate buffers and come back flagged.
    A moderate number goes through the batched fix-up (gathered copy + exact general kernel); more than N / 8 flagged rows -
    a low-norm block that is every row's nearest neighbour at one distance, or every row flagged by hand - through the exact
    general kernel over all rows.  Either way the radii are the single-GPU call's bits."""
    import numpy as np
    from audio_metrics_amd import hip_ops as ops
    k, rows, d = 5, 16500, 128
    x = gi.randn(31, rows, d)
    rng = np.random.default_rng(5)
    if kind == "block":
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        dup = rng.choice(rows, 700, replace=False)
        x[dup] = x[dup[0]]
    elif kind == "hub":
        dup = rng.choice(rows, 600, replace=False)
        x[dup] = 0.05 * x[dup[0]]
    x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).to("cuda:0")
    assert ops.knn_path(rows, rows, d, k) == 3
    want = ops.knn_radii(x, k).cpu().numpy()
    bounds = torch.cat([ops.knn_bounds(x, k, lo, hi - lo) for lo, hi in
                        [(rows * p // nparts, rows * (p + 1) // nparts) for p in range(nparts)]])
    lists = torch.stack([ops.knn_sym_part(x, k, p, nparts, bounds) for p in range(nparts)])
    flagged = int(torch.isnan(lists[:, :, 0]).any(dim=0).sum())
    if kind == "block":
        assert 32 < flagged <= rows // 8, flagged                 # enough for the batched route, few enough for its copy
    elif kind == "hub":
        assert flagged > 600, flagged
    else:
        lists[0, :, 0] = float("nan")
    got = ops.knn_lists_finish(lists, x, k).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_partitioned_exact_symmetric_kernel():
    """The partitioned form of the exact symmetric kernel (what the library takes where the f16 filter sweep does not apply:
    D > 4096, or the A/B build with AM_KNN_FAST=0) - in a subprocess, the knob is process-wide."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys, numpy as np, torch\n"
        f"sys.path.insert(0, {root!r}); sys.path.insert(0, {os.path.join(root, 'tests', 'golden')!r})\n"
        "import inputs as gi\n"
        "from audio_metrics_amd import hip_ops as ops\n"
        "x = torch.as_tensor(gi.randn(97, 9100, 136)).to('cuda:0')\n"
        "n, k = x.shape[0], 5\n"
        "assert ops.knn_path(n, n, 136, k) == 1 and ops.knn_sym_eligible(n, 136, k)\n"
        "want = ops.knn_radii(x, k).cpu().numpy()\n"
        "for nparts in (2, 3, 8):\n"
        "    bounds = torch.cat([ops.knn_bounds(x, k, n * p // nparts, n * (p + 1) // nparts - n * p // nparts) for p in range(nparts)])\n"
        "    lists = torch.stack([ops.knn_sym_part(x, k, p, nparts, bounds) for p in range(nparts)])\n"
        "    got = ops.knn_lists_finish(lists, x, k).cpu().numpy()\n"
        "    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), nparts\n"
        "print('partitioned exact ok')\n")
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, AM_HIP_LIBRARY="dev", AM_KNN_FAST="0"),
                         capture_output=True, text=True, timeout=600)
    assert "partitioned exact ok" in res.stdout, res.stdout + res.stderr


def test_sharded_evaluate_takes_symmetric_path():
    """2 ranks on cuda:0 over gloo with sets large and wide enough for the partitioned symmetric kernel."""
    from audio_metrics_amd.distributed import evaluate_sharded
    n_ref, n_cand, d, k, world = 8300, 8200, 128, 4, 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_ref, n_cand, d, k, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=240) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ref, cand = gi.pair("randn", 95, n_ref, n_cand, d)
    dev = torch.device("cuda:0")
    single = evaluate_sharded(torch.as_tensor(ref).to(dev), torch.as_tensor(cand).to(dev), nearest_k=k,
                              kid_subsets=8, kid_subset_size=300)
    assert results[0] == results[1]
    for key in ("precision", "recall", "density", "coverage"):
        assert results[0][key] == single[key], key


@pytest.mark.parametrize("ranks,rows,dim,plain", [(2, 3000, 64, False), (2, 3000, 64, True), (2, 9000, 128, False),
                                                  (8, 66000, 128, True), (2, 9000, 128, "c-entry")])
def test_bench_multi_rank_launch(ranks, rows, dim, plain):
    """bench.py launched the way the driver launches it for N=2 (torch.distributed.run, one JSON line from
    rank 0) - and `plain`: invoked as `python bench.py --gpus N` with no launcher (it then starts the ranks itself).  Both ranks share cuda:0 over gloo (bench.py's AM_BENCH_* test hooks); 9000x128 is eligible for the
    partitioned symmetric k-NN, 3000x64 takes the general kernel on row shards.  The N-rank result must equal the
    1-rank result of the same command.  The 8-rank case at 66000 x 128 is the driver's 8-GPU launch in every respect but the
    transport: am_knn_path == 3 (the f16 filter sweep on the 256-row engine, partitioned eight ways), prepared sets shared
    by a rank's entry points, 8-way fused collectives, unequal shards (66000 / 8 = 8250 rows: 32.2 row blocks per rank)."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # --full: the schedules, roofline, exchange and process_cold records checked below are not part of a plain run
    common = ["--steps", "1", "--warmup", "1", "--rows", str(rows), "--dim", str(dim), "--full", "--no-cpu-baseline"]
    env = dict(os.environ, AM_BENCH_DEVICE="0", AM_BENCH_BACKEND="gloo")
    if plain == "c-entry":          # every rank's timed step = ONE library call (am_evaluate_sharded_f32), its collectives hooks over gloo
        common = common + ["--c-entry"]
    if plain:
        # `python bench.py --gpus N` with no launcher around it: bench.py starts its own ranks in a child process and
        # passes rank 0's line and the exit code through
        env.pop("WORLD_SIZE", None)
        two = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(ranks)] + common,
                             env=env, capture_output=True, text=True, timeout=900)
    else:
        two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks),
                              "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                              os.path.join(root, "bench.py"), "--gpus", str(ranks)] + common,
                             env=env, capture_output=True, text=True, timeout=900)
    assert two.returncode == 0, two.stderr[-2000:]
    lines = [l for l in two.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, two.stdout[-2000:]
    out2 = json.loads(lines[0])
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1"] + common,
                         capture_output=True, text=True, timeout=600)
    assert one.returncode == 0, one.stderr[-2000:]
    out1 = json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][0])
    assert out2["n_gpus"] == ranks and out1["n_gpus"] == 1
    assert ("am_evaluate_sharded_f32" in out2["config"]["schedule"]) == (plain == "c-entry"), out2["config"]["schedule"]
    assert out2["n_ranks_seen"] == ranks and out1["n_ranks_seen"] == 1      # what the process group connected, not what was asked for
    if rows >= 32768 and dim >= 128:
        assert out2["filter"]["knn_path"] == 3 and out2["filter"]["knn_fallback_rows"] == 0, out2["filter"]
    for key in ("metric", "value", "unit", "ms_per_step", "scaling", "roofline", "config"):
        assert key in out2
    assert out2["roofline"]["frac"] > 0
    # a multi-rank line carries BOTH exchange schedules (the first 8-GPU run then says which is faster),
    # a one-rank line the fresh-process time to the first result
    assert out2["c_entry_ms"] > 0 and out2["python_schedule_ms"] > 0, sorted(out2)
    assert (out2["c_entry_ms"] if plain == "c-entry" else out2["python_schedule_ms"]) == out2["ms_per_step"]
    cold = out1["process_cold"]
    assert "error" not in cold, cold
    assert cold["process_cold_ms"] >= cold["warm_step_ms"] > 0 and set(cold["split_ms"]) == {"first_launch_code_objects", "workspace_hipMalloc_and_kd_table", "step"}
    if rows >= 8192 and dim >= 128:
        tiles = [out2["roofline"], out2["other_tile_kernel"]]
        assert any(t["entry_point"] in ("am_knn_sym_part_f32", "am_knn_sym_part_prepared_f32") for t in tiles)
    for key in ("precision", "recall", "density", "coverage"):
        assert out2["result"][key] == out1["result"][key], key
    assert abs(out2["result"]["fad"] - out1["result"]["fad"]) <= 1e-5 * abs(out1["result"]["fad"])
    assert abs(out2["result"]["kernel_distance_mean"] - out1["result"]["kernel_distance_mean"]) <= 1e-9
    # the first real multi-GPU run explains itself: per-collective exposed time and volume, the
    # all-gather bandwidth measured alone, the scale model's prediction for this rank count where one is committed
    ex = out2["exchange"]
    names = [r["name"] for r in ex["collectives"]]
    for must in ("column_sums", "scatters", "reference_rows", "candidate_rows", "membership_counts", "kd_subsets"):
        assert must in names, names
    assert "radii" in names or ("knn_bounds" in names and "knn_lists" in names), names     # row shards / partitioned symmetric sweep
    assert all(r["bytes"] > 0 and r["exposed_ms"] >= 0.0 and r["kind"] in ("all_reduce", "all_gather") for r in ex["collectives"])
    assert ex["exchange_exposed_ms"] >= 0.0 and ex["backend"] == "gloo"
    if rows % ranks == 0:
        assert ex["gather_GBps"] > 0.0 and ex["gather_ms"] > 0.0
    assert "exchange" not in out1 and "scale_model" in out2          # (None unless profiles/scale_model.json covers this workload)


def test_overlapped_frechet_solve_gives_the_same_result():
    """evaluate_sharded enqueues the Frechet solve on a side stream under the PRDC kernels (am_frechet_enqueue_f64: no
    host polling, no helper thread); the synchronous entry point on the main stream must give the same bits, and the
    other metrics must not change either."""
    from audio_metrics_amd import hip_ops as ops
    from audio_metrics_amd.distributed import evaluate_sharded
    ref, cand = gi.pair("randn", 41, 6000, 5500, 96)
    dev = torch.device("cuda:0")
    r, c = torch.as_tensor(ref).to(dev), torch.as_tensor(cand).to(dev)
    with_overlap = [evaluate_sharded(r, c, nearest_k=3, kid_subsets=6, kid_subset_size=500, fused=False) for _ in range(3)]

    class SyncOps:                                  # the same library without the asynchronous entry point
        def __getattr__(self, name):
            if name == "frechet_async":
                raise AttributeError(name)
            return getattr(ops, name)
    without = evaluate_sharded(r, c, nearest_k=3, kid_subsets=6, kid_subset_size=500, ops=SyncOps(), fused=False)
    for res in with_overlap:
        assert res == without


_RCCL_ONE_RANK = r"""
import json, os, sys
import torch
import torch.distributed as dist
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests", "golden"))
import inputs as gi
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=sys.argv[2], RANK="0", WORLD_SIZE="1")
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
import audio_metrics_amd as am
from audio_metrics_amd import distributed as D
out = {}
for name, rows, dim, k in (("small", 2500, 96, 4), ("partitioned", 33000, 128, 5)):
    ref, cand = (torch.as_tensor(a).to(dev) for a in gi.pair("randn", 95, rows, rows - 37, dim))
    want = D.evaluate_sharded(ref, cand, nearest_k=k, kid_subsets=8, kid_subset_size=300)          # one fused library call
    D.COLLECTIVES_AT_WORLD_ONE = True
    for comms in (1, 2):                                    # the default single communicator, then the optional second one
        if comms == 2:
            assert D.enable_bulk_communicator() is not None
        assert D.warm_up_communicators(dev) == 1            # (bench.py's call: one collective on every communicator; ranks seen)
        for rep in range(3):                                # repeated: stale buffers / stream-order slips show up as a changing result
            got = D.evaluate_sharded(ref, cand, nearest_k=k, kid_subsets=8, kid_subset_size=300)
            out[f"{name}_{comms}c_{rep}"] = {"want": want, "got": got}
    D.disable_bulk_communicator()
    # the one-call-per-rank form (am_evaluate_sharded_f32) with its hooks over THIS RCCL group: equal shares -> ONE
    # all_gather_into_tensor per row gather, in place in the library's buffer (VERDICT r5 next-5a)
    got_c = D.evaluate_sharded(ref, cand, nearest_k=k, kid_subsets=8, kid_subset_size=300, c_entry=True)
    coll = D.LAST_C_ENTRY_COLLECTIVES
    out[f"{name}_c_entry"] = {"want": want, "got": got_c, "gather_form": coll.gather_form, "calls": [n_ for n_, _ in coll.calls]}
    # the stats-only front end: (n, mean, cov) triples through the all-gather
    data = am.AudioMetricsData(store_embeddings=False); data.add(ref)
    merged = D.merged_stats(data)
    out[f"{name}_stats"] = {"n": int(merged.n), "mean_diff": float((merged.mean - data.mean).abs().max()),
                            "cov_diff": float((merged.cov - data.cov).abs().max())}
    assert D.global_count(rows, dev) == rows
    # the statistics the row-sharded PCA fit consumes (n_pca under a process group): two all-reduces over RCCL
    n_g, mean_g, cov_g = D.global_stats(ref)
    out[f"{name}_global_stats"] = {"n": int(n_g), "mean_diff": float((mean_g - data.mean).abs().max()),
                                   "cov_diff": float((cov_g - data.cov).abs().max() / data.cov.abs().max())}
    D.COLLECTIVES_AT_WORLD_ONE = False
torch.cuda.synchronize()
dist.barrier()
dist.destroy_process_group()
print("RCCL1 " + json.dumps(out))
"""


def test_collectives_over_rccl_in_a_group_of_one():
    """The RCCL branch of distributed.py (all_gather_into_tensor, asynchronous work handles waited on the compute stream, the
    fused all-reduces, the partitioned k-NN with its two all-gathers) executed on the real transport library: a process
    group of ONE rank over "nccl" with the module's test hook forcing every collective.  Two RCCL ranks cannot share the
    1-GPU box, so this is everything of the multi-GPU launch but the wire."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _RCCL_ONE_RANK, root, str(_free_port())], capture_output=True, text=True,
                         timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    line = [l for l in res.stdout.splitlines() if l.startswith("RCCL1 ")][0]
    out = json.loads(line[len("RCCL1 "):])
    for name, rec in out.items():
        if name.endswith("_global_stats"):
            assert rec["n"] in (2500, 33000) and rec["mean_diff"] <= 1e-12 and rec["cov_diff"] <= 1e-9, (name, rec)
            continue
        if name.endswith("_stats"):
            assert rec["n"] in (2500, 33000) and rec["mean_diff"] == 0.0 and rec["cov_diff"] == 0.0, (name, rec)
            continue
        want, got = rec["want"], rec["got"]
        if name.endswith("_c_entry"):
            assert rec["gather_form"] == "all_gather_into_tensor, in place" and rec["calls"].count("all_gather_v") == 2, rec
        for key in ("precision", "recall", "density", "coverage"):
            assert got[key] == want[key], (name, key)
        assert abs(got["fad"] - want["fad"]) <= 1e-5 * abs(want["fad"]), (name, got["fad"], want["fad"])
        assert abs(got["kernel_distance_mean"] - want["kernel_distance_mean"]) <= 1e-9, name
        assert abs(got["kernel_distance_std"] - want["kernel_distance_std"]) <= 1e-9, name


def _f64_worker(rank, world, port, n_ref, n_cand, d, k, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from audio_metrics_amd import distributed as dmod
    ref, cand = gi.pair64("randn", 97, n_ref, n_cand, d)
    rl, rh = dmod.shard_bounds(n_ref, world, rank)
    cl, ch = dmod.shard_bounds(n_cand, world, rank)
    dev = torch.device("cuda:0")
    dmod.exchange_log_begin()
    res = dmod.evaluate_sharded(torch.as_tensor(ref[rl:rh]).to(dev), torch.as_tensor(cand[cl:ch]).to(dev), nearest_k=k,
                                kid_subsets=8, kid_subset_size=300)
    names = [r["name"] for r in dmod.exchange_log_end()]
    out_q.put((rank, res, names))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_evaluate_of_float64_rows():
    """float64 row shards on two ranks (sharing cuda:0 over gloo): every stage in float64; at these sizes each rank computes the
    gathered sets' radii on the f16 filter route with the f64 evaluation - no radius exchange - and its share of the membership
    counts the same way.  Equal to the one-rank result."""
    from audio_metrics_amd.distributed import evaluate_sharded
    n_ref, n_cand, d, k, world = 16500, 16400, 48, 4, 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_f64_worker, args=(r, world, port, n_ref, n_cand, d, k, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    results = {rank: res for rank, res, _ in got}
    names = got[0][2]
    assert "radii" not in names and "knn_lists" not in names, names           # nothing exchanged for the radii
    ref, cand = gi.pair64("randn", 97, n_ref, n_cand, d)
    dev = torch.device("cuda:0")
    single = evaluate_sharded(torch.as_tensor(ref).to(dev), torch.as_tensor(cand).to(dev), nearest_k=k, kid_subsets=8, kid_subset_size=300)
    assert results[0] == results[1]
    for key, w in single.items():
        if key in ("precision", "recall", "density", "coverage"):
            assert results[0][key] == w, key
        else:
            assert abs(results[0][key] - w) <= 1e-9 * abs(w) + 1e-13, (key, results[0][key], w)
