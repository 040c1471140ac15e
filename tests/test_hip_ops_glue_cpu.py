"""The C arguments of every hip_ops operation, without a device: each public operation that reaches the library through
hip_ops._call is run on CPU tensors with _require_cuda, _call and _workspace replaced (the _Recorder of
test_groups_glue_cpu.py), and every recorded call must fit _lib.SIGNATURES - the argument count, a pointer in every pointer
slot, a float in every double slot, an int in every integer slot - with, where the entry point takes a workspace, the
workspace pointer and exactly the answer of its workspace query for the sample's shapes as the last two arguments.  ctypes
itself would not notice an argument slipped by one position: it accepts an int where a pointer is declared."""
import ctypes
import inspect
import re

import pytest
import torch

from test_groups_glue_cpu import _Recorder

N, M, D = 300, 200, 20
_gen = torch.Generator().manual_seed(7)


def _randn(*shape, dtype=torch.float32):
    return torch.randn(*shape, generator=_gen, dtype=dtype)


X, Y = _randn(N, D), _randn(M, D)
X64, Y64 = X.double(), Y.double()
X19, Y19 = _randn(N, 19), _randn(M, 19)                      # D % 4 != 0: as_matrix pads the row stride
XV = _randn(N, 2 * D)[:, ::2]                                # a strided view: as_matrix copies
X2, Y12 = _randn(N, D), _randn(N, 12)
IDX, OFFS = torch.arange(9, dtype=torch.int64) * 7, [0, 5, 9]        # two groups, 9 listed rows
MU, COV = _randn(D, dtype=torch.float64), torch.eye(D, dtype=torch.float64)
TAB = torch.arange(40, dtype=torch.int64).reshape(4, 10)     # kernel-distance index tables: S = 4, m = 10
XL, YL = (torch.arange(N) % 5).to(torch.int32), (torch.arange(M) % 5).to(torch.int32)
R_Y = torch.ones(M)
THETA, MOM, LSE = torch.zeros(M, dtype=torch.float64), torch.zeros(M, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
CENTROIDS, DIRECTIONS, FREQS = _randn(8, D), _randn(6, D), _randn(16, D)
ZX, ZY = _randn(6, N), _randn(6, M)
POS = torch.arange(N, dtype=torch.int64)
STATS_Q, STATS64_Q = "am_stats_workspace_bytes", "am_stats_f64_workspace_bytes"
GROUPS_Q = (9, 2, D)


def _prepared(ops, x):
    return ops.prepare(x)


def _lists(ops, k):
    return torch.zeros((2, N, ops._lib.load().am_knn_list_width(k)))


PREPARE = ("am_prepare_set_f32", None, None)

# (operation, what the sample varies, call(ops), [(entry point, workspace query or None, the query's arguments)] in call order)
SAMPLES = [
    ("stats", "f32", lambda o: o.stats(X), [("am_stats_f32", STATS_Q, (N, D))]),
    ("stats", "D % 4 != 0", lambda o: o.stats(X19), [("am_stats_f32", STATS_Q, (N, 19))]),
    ("stats", "strided view", lambda o: o.stats(XV), [("am_stats_f32", STATS_Q, (N, D))]),
    ("stats", "f64", lambda o: o.stats(X64), [("am_stats_f64", STATS64_Q, (N, D))]),
    ("stats_f64", "f64", lambda o: o.stats_f64(X64), [("am_stats_f64", STATS64_Q, (N, D))]),
    ("stats_f64", "f64 strided view", lambda o: o.stats_f64(XV.double()), [("am_stats_f64", STATS64_Q, (N, D))]),
    ("stats_gather", "f32", lambda o: o.stats_gather(X, IDX, OFFS), [("am_stats_gather_f32", "am_stats_gather_workspace_bytes", GROUPS_Q)]),
    ("stats_gather", "f64, deferred check", lambda o: o.stats_gather(X64, IDX, OFFS, defer_check=True),
     [("am_stats_gather_f64", "am_stats_gather_workspace_bytes", GROUPS_Q)]),
    ("colsum", "f32", lambda o: o.colsum(X19), [("am_colsum_f32", STATS_Q, (N, 19))]),
    ("colsum", "f64", lambda o: o.colsum(X64), [("am_colsum_f64", STATS64_Q, (N, D))]),
    ("scatter", "f32", lambda o: o.scatter(XV, MU), [("am_scatter_f32", STATS_Q, (N, D))]),
    ("scatter", "f64", lambda o: o.scatter(X64, MU), [("am_scatter_f64", STATS64_Q, (N, D))]),
    ("stats_merge", "fresh outputs", lambda o: o.stats_merge(N, MU, COV, M, MU, COV), [("am_stats_merge_f64", None, None)]),
    ("stats_merge", "in place", lambda o: o.stats_merge(N, MU.clone(), COV.clone(), M, MU, COV, inplace=True),
     [("am_stats_merge_f64", None, None)]),
    ("eigh_descending", "", lambda o: o.eigh_descending(COV), [("am_eigh_sym_f64", "am_eigh_workspace_bytes", (D,))]),
    ("project", "f32", lambda o: o.project(X, MU, COV[:5]), [("am_project_f64", None, None)]),
    ("project", "f64", lambda o: o.project(X64, MU, COV[:5]), [("am_project_rows_f64", None, None)]),
    ("frechet", "", lambda o: o.frechet(MU, COV, MU, COV), [("am_frechet_f64", "am_frechet_workspace_bytes", (D,))]),
    ("frechet_maps", "", lambda o: o.frechet_maps(MU, COV, MU, COV), [("am_frechet_maps_f64", "am_frechet_maps_workspace_bytes", (D,))]),
    ("frechet_influence", "f32", lambda o: o.frechet_influence(X, MU, COV, MU, 0.5),
     [("am_frechet_influence_f32", "am_frechet_influence_workspace_bytes", (N,))]),
    ("frechet_influence", "f64", lambda o: o.frechet_influence(X64, MU, COV, MU, 1),
     [("am_frechet_influence_f64", "am_frechet_influence_workspace_bytes", (N,))]),
    ("logit_pass", "f32", lambda o: o.logit_pass(X, XL, 1, torch.zeros((3, D + 1), dtype=torch.float64)),
     [("am_logit_pass_f32", "am_logit_pass_workspace_bytes", (N, D, 3))]),
    ("logit_pass", "f64, no z", lambda o: o.logit_pass(X64, XL, 0, torch.zeros((3, D + 1), dtype=torch.float64), want_z=False),
     [("am_logit_pass_f64", "am_logit_pass_workspace_bytes", (N, D, 3))]),
    ("frechet_batch", "shared reference", lambda o: o.frechet_batch(MU.repeat(3, 1), COV.repeat(3, 1, 1), MU, COV,
                                                                    out=torch.zeros((3, 5), dtype=torch.float64)),
     [("am_frechet_batch_f64", "am_frechet_batch_workspace_bytes", (3, D))]),
    ("frechet_batch", "one reference per set", lambda o: o.frechet_batch(MU.repeat(3, 1), COV.repeat(3, 1, 1), MU.repeat(3, 1),
                                                                         COV.repeat(3, 1, 1), out=torch.zeros((3, 5), dtype=torch.float64)),
     [("am_frechet_batch_f64", "am_frechet_batch_workspace_bytes", (3, D))]),
    ("frechet_groups", "f32, index list", lambda o: o.frechet_groups(X, IDX, OFFS, MU, COV),
     [("am_frechet_groups_f32", "am_frechet_groups_workspace_bytes", GROUPS_Q)]),
    ("frechet_groups", "f64, stored order, out given", lambda o: o.frechet_groups(X64, None, OFFS, MU, COV,
                                                                                  out=torch.zeros((2, 5), dtype=torch.float64)),
     [("am_frechet_groups_f64", "am_frechet_groups_workspace_bytes", GROUPS_Q)]),
    ("vendi_groups", "f32 cosine", lambda o: o.vendi_groups(X, IDX, OFFS), [("am_vendi_groups_f32", "am_vendi_groups_workspace_bytes", GROUPS_Q)]),
    ("vendi_groups", "f64 gaussian, stored order", lambda o: o.vendi_groups(X64, None, OFFS, kernel="gaussian", gamma=0.25),
     [("am_vendi_groups_f64", "am_vendi_groups_workspace_bytes", GROUPS_Q)]),
    ("vendi_gram", "f32, index list", lambda o: o.vendi_gram(X19, IDX), [("am_vendi_gram_f32", "am_vendi_gram_workspace_bytes", (9, 19))]),
    ("vendi_gram", "f64 gaussian, all rows", lambda o: o.vendi_gram(X64[:50], kernel="gaussian", gamma=2),
     [("am_vendi_gram_f64", "am_vendi_gram_workspace_bytes", (50, D))]),
    ("vendi_moment", "f32", lambda o: o.vendi_moment(X), [("am_vendi_moment_f32", "am_vendi_moment_workspace_bytes", (N, D))]),
    ("vendi_moment", "f64", lambda o: o.vendi_moment(X64), [("am_vendi_moment_f64", "am_vendi_moment_workspace_bytes", (N, D))]),
    ("kd_poly", "f32", lambda o: o.kd_poly(X, Y, TAB, TAB, 1.0 / D, 1, 3), [("am_kd_poly_f32", "am_kd_poly_workspace_bytes", (4, 10, D))]),
    ("kd_poly", "one side f64", lambda o: o.kd_poly(X, Y64, TAB, TAB, 1.0 / D, 1.0, 3), [("am_kd_poly_f64", "am_kd_f64_workspace_bytes", (4, 10))]),
    ("kd_rbf", "f32, D % 4 != 0", lambda o: o.kd_rbf(X19, Y19, TAB, TAB, 10), [("am_kd_rbf_f32", "am_kd_rbf_workspace_bytes", (4, 10))]),
    ("kd_rbf", "f64", lambda o: o.kd_rbf(X64, Y64, TAB, TAB, 10.0), [("am_kd_rbf_f64", "am_kd_f64_workspace_bytes", (4, 10))]),
    ("pairwise_select_sq", "f32 median", lambda o: o.pairwise_select_sq(X),
     [("am_pairwise_select_f32", "am_pairwise_select_workspace_bytes", (N, D))]),
    ("pairwise_select_sq", "f64 rank", lambda o: o.pairwise_select_sq(X64, rank=17),
     [("am_pairwise_select_f64", "am_pairwise_select_f64_workspace_bytes", (N, D))]),
    ("mmd_rbf_sums", "f32 gamma", lambda o: o.mmd_rbf_sums(X, Y, gamma=1), [("am_mmd_rbf_f32", "am_mmd_rbf_workspace_bytes", (N, M, D, 7))]),
    ("mmd_rbf_sums", "f32 device bandwidth", lambda o: o.mmd_rbf_sums(XV, Y, bw2=torch.ones(()), blocks=o.MMD_XY),
     [("am_mmd_rbf_f32", "am_mmd_rbf_workspace_bytes", (N, M, D, 4))]),
    ("mmd_rbf_sums", "f64", lambda o: o.mmd_rbf_sums(X64, Y64, gamma=0.5), [("am_mmd_rbf_f64", "am_mmd_rbf_f64_workspace_bytes", (N, M, D, 7))]),
    ("mmd_rbf_row_sums", "all blocks", lambda o: o.mmd_rbf_row_sums(X, Y, gamma=0.5),
     [("am_mmd_rbf_rows_f32", "am_mmd_rbf_rows_workspace_bytes", (N, M, D, 7))]),
    ("mmd_rbf_row_sums", "one side only", lambda o: o.mmd_rbf_row_sums(X19, Y19, bw2=torch.ones(()), blocks=o.MMD_XX),
     [("am_mmd_rbf_rows_f32", "am_mmd_rbf_rows_workspace_bytes", (N, M, 19, 1))]),
    ("mmd_rbf_cell_sums", "stored order", lambda o: o.mmd_rbf_cell_sums(X, Y, gamma=0.5),
     [("am_mmd_rbf_cells_f32", "am_mmd_rbf_cells_workspace_bytes", (N, M, D, 7))]),
    ("mmd_rbf_cell_sums", "index list, units, two blocks", lambda o: o.mmd_rbf_cell_sums(X, Y, idx_x=torch.arange(64), units_x=[0, 1, 2],
                                                                                        blocks=o.MMD_XX | o.MMD_XY, bw2=torch.ones(())),
     [("am_mmd_rbf_cells_f32", "am_mmd_rbf_cells_workspace_bytes", (64, M, D, 5))]),
    ("mmd_multi_sums", "two scales", lambda o: o.mmd_multi_sums(X, Y, "gaussian", [1, 2.0], bw2=3),
     [("am_mmd_multi_f32", "am_mmd_multi_workspace_bytes", (N, M, D, 2, 7))]),
    ("mmd_multi_sums", "five scales in two calls, device bandwidth", lambda o: o.mmd_multi_sums(X, Y, "laplacian", [1, 2, 3, 4, 5],
                                                                                               bw2=torch.ones(()), blocks=3),
     [("am_mmd_multi_f32", "am_mmd_multi_workspace_bytes", (N, M, D, 4, 3)), ("am_mmd_multi_f32", "am_mmd_multi_workspace_bytes", (N, M, D, 1, 3))]),
    ("mmd_multi_sums", "energy", lambda o: o.mmd_multi_sums(X, Y, "energy", [1.0]),
     [("am_mmd_multi_f32", "am_mmd_multi_workspace_bytes", (N, M, D, 1, 7))]),
    ("pair_dependence", "energy", lambda o: o.pair_dependence(X, Y12, "energy"),
     [("am_pair_dependence_f32", "am_pair_dependence_workspace_bytes", (N, D, 12))]),
    ("pair_dependence", "gaussian, permuted", lambda o: o.pair_dependence(X, Y12, "gaussian", bw2x=2, bw2y=torch.ones(()), perm=POS.flip(0)),
     [("am_pair_dependence_f32", "am_pair_dependence_workspace_bytes", (N, D, 12))]),
    ("mmd_rbf_group_sums", "f32, index list", lambda o: o.mmd_rbf_group_sums(X, IDX, OFFS, Y, gamma=0.5),
     [("am_mmd_rbf_groups_f32", "am_mmd_rbf_groups_workspace_bytes", (9, 2, M, D))]),
    ("mmd_rbf_group_sums", "f64, stored order, row sums", lambda o: o.mmd_rbf_group_sums(X64, None, OFFS, Y64, gamma=0.5, rows=True),
     [("am_mmd_rbf_groups_f64", "am_mmd_rbf_groups_f64_workspace_bytes", (9, 2, M, D))]),
    ("prepare", "", lambda o: o.prepare(X19), [PREPARE]),
    ("PreparedSet", "a row shard's struct", lambda o: o.prepare(X).rows(10, 20).struct(), [PREPARE]),
    ("knn_radii", "self distance", lambda o: o.knn_radii(X, 5), [("am_knn_radii_f32", "am_knn_workspace_bytes", (N, N, D, 5))]),
    ("knn_radii", "against columns", lambda o: o.knn_radii(XV, 5, columns=Y), [("am_knn_radii_f32", "am_knn_workspace_bytes", (N, M, D, 5))]),
    ("knn_radii", "prepared", lambda o: o.knn_radii(X, 5, prepared=_prepared(o, X)),
     [PREPARE, ("am_knn_radii_prepared_f32", "am_knn_workspace_bytes", (N, N, D, 5))]),
    ("knn_radii", "f64 columns", lambda o: o.knn_radii(X, 5, columns=Y64), [("am_knn_radii_f64", "am_knn_f64_workspace_bytes", (N, M, D, 5))]),
    ("knn_search", "", lambda o: o.knn_search(X, Y, 3), [("am_knn_search_f32", "am_knn_search_workspace_bytes", (N, M, D, 3))]),
    ("knn_search", "itself, squared", lambda o: o.knn_search(X19, X19, 3, self_offset=0, squared=True),
     [("am_knn_search_f32", "am_knn_search_workspace_bytes", (N, N, 19, 3))]),
    ("knn_search_groups", "", lambda o: o.knn_search_groups(X, Y, 3, XL, YL),
     [("am_knn_search_groups_f32", "am_knn_search_groups_workspace_bytes", (N, M, D, 3))]),
    ("sample_scores", "", lambda o: o.sample_scores(X, Y, R_Y), [("am_sample_scores_f32", "am_sample_scores_workspace_bytes", (N, M, D))]),
    ("sample_scores_groups", "", lambda o: o.sample_scores_groups(XV, Y, R_Y, XL, YL),
     [("am_sample_scores_groups_f32", "am_sample_scores_groups_workspace_bytes", (N, M, D))]),
    ("psr_scores", "", lambda o: o.psr_scores(X, Y, 2), [("am_psr_f32", "am_psr_workspace_bytes", (N, M, D))]),
    ("psr_scores", "itself, no sums", lambda o: o.psr_scores(X19, X19, 2.5, sums=False), [("am_psr_f32", "am_psr_workspace_bytes", (N, N, 19))]),
    ("retrieval_ranks", "", lambda o: o.retrieval_ranks(X, Y, POS % M, torch.ones(N, dtype=torch.int64), torch.arange(M)),
     [("am_retrieval_ranks_f32", "am_retrieval_workspace_bytes", (N, M, D))]),
    ("retrieval_ranks", "groups, dot, no positives", lambda o: o.retrieval_ranks(X, Y, POS * 0, POS * 0, torch.zeros(0, dtype=torch.int64),
                                                                                 cosine=False, groups=(XL, YL)),
     [("am_retrieval_ranks_f32", "am_retrieval_workspace_bytes", (N, M, D))]),
    ("kmeans_assign", "", lambda o: o.kmeans_assign(X, CENTROIDS), [("am_kmeans_assign_f32", "am_kmeans_assign_workspace_bytes", (N, 8, D))]),
    ("kmeans_update", "", lambda o: o.kmeans_update(X, POS % 8, CENTROIDS), [("am_kmeans_update_f32", "am_kmeans_update_workspace_bytes", (N, 8, D))]),
    ("softmin", "", lambda o: o.softmin(X, Y, eps=0.5), [("am_softmin_f32", "am_softmin_workspace_bytes", (N, M, D))]),
    ("softmin", "potentials, damped", lambda o: o.softmin(X, Y, g=THETA, eps=1, prev=LSE, damping=0.5),
     [("am_softmin_f32", "am_softmin_workspace_bytes", (N, M, D))]),
    ("fld_loglik", "", lambda o: o.fld_loglik(X, Y, THETA), [("am_fld_loglik_f32", "am_fld_loglik_workspace_bytes", (N, M, D))]),
    ("fld_loglik", "stats given", lambda o: o.fld_loglik(X19, Y19, THETA, stats=torch.zeros(3, dtype=torch.float64)),
     [("am_fld_loglik_f32", "am_fld_loglik_workspace_bytes", (N, M, 19))]),
    ("fld_grad_step", "", lambda o: o.fld_grad_step(Y, X, THETA, LSE, torch.ones(1, dtype=torch.float64), MOM, MOM, 1, 0.1, -5),
     [("am_fld_grad_f32", "am_fld_grad_workspace_bytes", (M, N, D))]),
    ("sliced_project", "", lambda o: o.sliced_project(X, DIRECTIONS), [("am_sliced_project_f32", None, None)]),
    ("sort_rows", "", lambda o: o.sort_rows(ZX), [("am_sort_rows_f32", "am_sort_rows_workspace_bytes", (6, N))]),
    ("sort_rows", "in place", lambda o: o.sort_rows(ZY, out=ZY), [("am_sort_rows_f32", "am_sort_rows_workspace_bytes", (6, M))]),
    ("sliced_w", "", lambda o: o.sliced_w(ZX, ZY, p=1), [("am_sliced_w_f32", "am_sliced_w_workspace_bytes", (6, N, M))]),
    ("rff_features", "all rows", lambda o: o.rff_features(X, FREQS, inv_bw=0.5), [("am_rff_features_f32", "am_rff_features_workspace_bytes", (N,))]),
    ("rff_features", "a row range into out, device bandwidth, check", lambda o: o.rff_features(
        X, FREQS, bw2=torch.ones(()), row0=10, nrows=50, out=torch.zeros((32, 64), dtype=torch.float64), return_check=True),
     [("am_rff_features_f32", "am_rff_features_workspace_bytes", (50,))]),
    ("rff_moment", "", lambda o: o.rff_moment(X, FREQS, inv_bw=1), [("am_rff_moment_f32", "am_rff_moment_workspace_bytes", (N, D, 16))]),
    ("class_group_scores", "f32, index list, rows", lambda o: o.class_group_scores(X, IDX, OFFS, return_rows=True),
     [("am_class_groups_f32", "am_class_groups_workspace_bytes", GROUPS_Q)]),
    ("class_group_scores", "f64, stored order", lambda o: o.class_group_scores(X64, None, OFFS),
     [("am_class_groups_f64", "am_class_groups_workspace_bytes", GROUPS_Q)]),
    ("row_pair_scores", "f32", lambda o: o.row_pair_scores(X, X2, "cosine"), [("am_row_pairs_f32", "am_row_pairs_workspace_bytes", (N,))]),
    ("row_pair_scores", "f64, rows, eps", lambda o: o.row_pair_scores(X64, X2.double(), "kl_softmax", eps=1, return_rows=True),
     [("am_row_pairs_f64", "am_row_pairs_workspace_bytes", (N,))]),
    ("knn_bounds", "", lambda o: o.knn_bounds(X, 5, 10, 50), [("am_knn_bounds_f32", "am_knn_part_workspace_bytes", (N, D, 5))]),
    ("knn_bounds", "prepared", lambda o: o.knn_bounds(X, 5, 10, 50, prepared=_prepared(o, X)),
     [PREPARE, ("am_knn_bounds_prepared_f32", "am_knn_part_workspace_bytes", (N, D, 5))]),
    ("knn_sym_part", "", lambda o: o.knn_sym_part(X, 5, 1, 2, torch.ones(N)), [("am_knn_sym_part_f32", "am_knn_part_workspace_bytes", (N, D, 5))]),
    ("knn_sym_part", "prepared", lambda o: o.knn_sym_part(X, 5, 1, 2, torch.ones(N), prepared=_prepared(o, X)),
     [PREPARE, ("am_knn_sym_part_prepared_f32", "am_knn_part_workspace_bytes", (N, D, 5))]),
    ("knn_lists_finish", "", lambda o: o.knn_lists_finish(_lists(o, 5), X, 5),
     [("am_knn_lists_finish_f32", "am_knn_lists_finish_workspace_bytes", (N, D, 5))]),
    ("prdc_counts", "f32", lambda o: o.prdc_counts(X, Y, torch.ones(N), R_Y), [("am_prdc_counts_f32", "am_prdc_workspace_bytes", (N, M, D))]),
    ("prdc_counts", "prepared, row minimum", lambda o: o.prdc_counts(X, Y, torch.ones(N), R_Y, want_min=True, prepared_ref=_prepared(o, X),
                                                                     prepared_cand=_prepared(o, Y)),
     [PREPARE, PREPARE, ("am_prdc_counts_prepared_f32", "am_prdc_workspace_bytes", (N, M, D))]),
    ("prdc_counts", "one side f64, row minimum", lambda o: o.prdc_counts(X64, Y, torch.ones(N), R_Y, want_min=True),
     [("am_prdc_counts_f64", "am_prdc_f64_workspace_bytes", (N, M, D))]),
    ("prdc_reduce", "", lambda o: o.prdc_reduce(torch.zeros(M, dtype=torch.int32), torch.zeros(N, dtype=torch.uint8),
                                                torch.zeros(N, dtype=torch.uint8)), [("am_prdc_reduce", None, None)]),
]

# host queries: they name an entry point, answer a number and launch nothing
HOST_QUERIES = {
    "stats_push_max_rows": (), "frechet_groups_max_rows": (), "vendi_groups_max_rows": (), "vendi_gram_max_rows": (),
    "vendi_moment_chunks": (N, D), "apa_scalar": (1.0, 2.0, 3.0), "knn_search_chunks": (N, M, D, 3), "sample_scores_chunks": (N, M, D),
    "psr_chunks": (N, M, D), "retrieval_chunks": (N, M, D), "rff_max_features": (), "rff_moment_chunks": (N, 16), "knn_path": (N, M, D, 5),
    "prdc_path": (N, M, D), "kd_path": (N, D, M, D, D, 10), "filter_engine": (D,), "knn_sym_eligible": (N, D, 5),
}

# left out, each for the one admissible reason: the operation enters torch.cuda itself (streams, events, the current device)
# or hands the library a device state directly, so it cannot run without a device
NEEDS_A_DEVICE = {
    "upload_host_array": "copies on a side stream", "filter_stats_enable": "torch.cuda.device and a device buffer",
    "filter_stats_read": "reads the device buffer of filter_stats_enable", "kernel_clock_enable": "hipEvents inside the library",
    "kernel_clock_read": "waits for the hipEvents of kernel_clock_enable", "stats_push": "its own torch.cuda.device / current_stream call",
    "frechet_async": "FrechetJob", "FrechetJob": "side stream of its own", "evaluate": "streams and events around a direct library call",
    "evaluate_sharded_c": "streams around a direct library call",
}

INTEGERS = (ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_uint, ctypes.c_uint64)


@pytest.fixture(scope="module")
def am():
    import audio_metrics_amd
    return audio_metrics_amd


class Recorder(_Recorder):
    """_Recorder that also keeps, per recorded call, the workspace allocated for it (None: the call took none)."""

    def __init__(self, monkeypatch, ops):
        super().__init__(monkeypatch, ops)
        monkeypatch.setattr(ops, "_call", self._call)

    def _call(self, lib, name, dev, *args):
        self.calls.append((name, args, self.ws))
        self.ws = None


def check_call(am, lib, name, args, ws, query, query_args):
    """One recorded call against _lib.SIGNATURES[name] and against its workspace query."""
    argtypes = am._lib.SIGNATURES[name][1]
    assert len(args) == len(argtypes) - 1, f"{name}: {len(args)} arguments for {len(argtypes) - 1} (the stream is appended by _call)"
    for i, (a, t) in enumerate(zip(args, argtypes)):
        where = f"{name}: argument {i} = {a!r}"
        if t is ctypes.c_void_p:
            assert a is None or isinstance(a, ctypes.c_void_p) or type(a).__name__ == "CArgObject", f"{where} is no pointer"
        elif t is ctypes.c_double:
            assert type(a) is float, f"{where} is no float"
        else:
            assert t in INTEGERS, f"{name}: argument {i} has a type this test does not know"
            assert isinstance(a, int) and not isinstance(a, bool), f"{where} is no int"
    if query is None:
        assert ws is None, f"{name} takes no workspace, one was allocated"
        return
    assert argtypes[-3:] == [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    want = getattr(lib, query)(*query_args)
    assert want > 0, f"{query}{query_args} answers 0: the sample's shapes are not valid"
    assert ws is not None and args[-2].value == ws.data_ptr(), f"{name}: the workspace pointer is not the allocation's"
    assert args[-1] == want, f"{name}: workspace size {args[-1]}, {query}{query_args} answers {want}"
    assert ws.numel() == max(want, 16)


@pytest.mark.parametrize("op, what, call, entries", SAMPLES, ids=[f"{s[0]}[{s[1]}]" if s[1] else s[0] for s in SAMPLES])
def test_recorded_calls_fit_their_signatures(am, monkeypatch, op, what, call, entries):
    ops = am.hip_ops
    lib = am._lib.load()
    rec = Recorder(monkeypatch, ops)
    call(ops)
    assert [c[0] for c in rec.calls] == [e[0] for e in entries]
    for (name, args, ws), (_, query, query_args) in zip(rec.calls, entries):
        check_call(am, lib, name, args, ws, query, query_args)


@pytest.mark.parametrize("name", list(HOST_QUERIES))
def test_host_queries_launch_nothing(am, monkeypatch, name):
    ops = am.hip_ops
    rec = Recorder(monkeypatch, ops)
    answer = getattr(ops, name)(*HOST_QUERIES[name])
    assert isinstance(answer, (int, float)) and rec.calls == []


def test_every_operation_has_a_row(am):
    """A public callable of hip_ops that names an am_* entry point is in SAMPLES, in HOST_QUERIES or, with its reason, in
    NEEDS_A_DEVICE: the next operation cannot be added without a row."""
    ops = am.hip_ops
    named = set()
    for name, obj in vars(ops).items():
        if name.startswith("_") or not callable(obj) or getattr(obj, "__module__", None) != ops.__name__:
            continue
        if re.search(r"\bam_[a-z0-9_]+", inspect.getsource(obj)):
            named.add(name)
    sampled = {s[0] for s in SAMPLES}
    listed = sampled | set(HOST_QUERIES) | set(NEEDS_A_DEVICE)
    assert len(named) >= 70 and not sampled & set(HOST_QUERIES) and not (sampled | set(HOST_QUERIES)) & set(NEEDS_A_DEVICE)
    assert named <= listed, f"without a row: {sorted(named - listed)}"
    for name in listed - named:                       # (operations whose entry point is named by a helper they call)
        assert callable(getattr(ops, name)), name
    # every float64 entry point of the table is reached by some sample
    reached = {e[0] for s in SAMPLES for e in s[3]}
    wide = {n for n in am._lib.SIGNATURES if n.endswith("_f64") and am._lib.SIGNATURES[n][1][-3:-1] == [ctypes.c_void_p, ctypes.c_size_t]}
    assert wide - reached <= {"am_frechet_enqueue_f64"}, wide - reached
