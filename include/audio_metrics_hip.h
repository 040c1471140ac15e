/*
 * audio_metrics_hip.h - C ABI of the MI355X (gfx950) distribution-distance library.
 *
 * This is the drop-in boundary for the hot path of SonyCSLParis/audio-metrics
 * (reference v1.0.4): everything that happens between "N x D embedding matrix"
 * and "metric value".  The reference has no FFI for this path - its boundary
 * is the Python call surface of data.py and metrics/{fad,kd,prdc,apa}.py - so every entry point
 * below cites the reference function (file:line, relative to the reference
 * checkout) whose arithmetic it replaces.  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *  - plain C types only; no torch / HIP types in signatures (am_stream_t is a
 *    hipStream_t passed as void*; NULL = the default stream);
 *  - every data pointer is a DEVICE pointer owned by the caller unless the
 *    parameter is documented as "host"; matrices are row-major with an explicit
 *    leading dimension `ld` (elements), base pointers 16-byte aligned and
 *    ld % 4 == 0 for float matrices;
 *  - the library allocates nothing: scratch comes from a caller-provided
 *    workspace whose size is returned by the matching workspace-size query;
 *  - all work is enqueued on `stream`; functions return without synchronising
 *    unless documented otherwise; return value 0 = AM_OK, negative = am_status;
 *  - no exceptions cross the ABI; am_last_error() gives a thread-local message.
 */
#ifndef AUDIO_METRICS_HIP_H
#define AUDIO_METRICS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* am_stream_t;

typedef enum am_status {
    AM_OK = 0,
    AM_ERR_BAD_ARG = -1,          /* null pointer, misaligned base, ld % 4 != 0 ...           */
    AM_ERR_BAD_SHAPE = -2,        /* empty input, D < 1, k + 1 > N (torch.kthvalue would raise) */
    AM_ERR_UNSUPPORTED_K = -3,    /* nearest_k > AM_MAX_K in an entry point of the partitioned form */
    AM_ERR_WORKSPACE = -4,        /* workspace missing or too small                            */
    AM_ERR_NO_CONVERGENCE = -5,   /* Newton-Schulz produced a non-finite trace; Jacobi: non-finite A, or max_sweeps */
    AM_ERR_HIP = -6               /* a HIP runtime call failed (see am_last_error)             */
} am_status;

#define AM_MAX_K 31               /* largest nearest_k of the TILE kernels (k+1 <= 32 list slots); am_knn_radii_f32 takes any
                                     k < M and runs larger ones row by row (am_knn_path == 4)        */

const char* am_version(void);
const char* am_status_string(int status);
const char* am_last_error(void);

/* ---------------------------------------------------------------------------
 * A1/A2  per-set sufficient statistics        reference: data.py:37-47, 49-58
 *   mean[D]  = column means of X (f64 accumulation of the f32 inputs)
 *   cov[D*D] = unbiased covariance  sum (x-mean)(x-mean)^T / (N-1)   (f64 out;
 *              products on the f32 matrix cores in short chains, f64 across)
 *   N == 1 -> cov = 0 (data.py:40-42).  N == 0 -> AM_ERR_BAD_SHAPE.
 * am_colsum_f32 / am_scatter_f32 are the two halves (column sums; centred
 * scatter matrix, NOT divided) that a multi-GPU caller all-reduces in between.
 * ------------------------------------------------------------------------- */
size_t am_stats_workspace_bytes(int64_t N, int D);
int am_stats_f32(const float* X, int64_t N, int D, int64_t ld,
                 double* mean, double* cov,
                 void* ws, size_t ws_bytes, am_stream_t stream);
int am_colsum_f32(const float* X, int64_t N, int D, int64_t ld,
                  double* colsum, void* ws, size_t ws_bytes, am_stream_t stream);
int am_scatter_f32(const float* X, int64_t N, int D, int64_t ld, const double* mean,
                   double* scatter, void* ws, size_t ws_bytes, am_stream_t stream);
/* float64 rows: the reference computes an add()'s statistics in the dtype of the embeddings it is given (data.py:39-44; its
 * own test embedder and the output of its PCA projection are float64).  Same outputs, every step in f64 (column sums per row
 * block, centred scatter on the f64 matrix cores, fixed-order reductions).  ld in elements, no alignment requirement. */
size_t am_stats_f64_workspace_bytes(int64_t N, int D);
int am_stats_f64(const double* X, int64_t N, int D, int64_t ld,
                 double* mean, double* cov,
                 void* ws, size_t ws_bytes, am_stream_t stream);
/* the two halves of am_stats_f64 (column sums; centred scatter, NOT divided) for a multi-GPU caller, as am_colsum_f32 /
 * am_scatter_f32; same workspace query.  D <= 8192. */
int am_colsum_f64(const double* X, int64_t N, int D, int64_t ld,
                  double* colsum, void* ws, size_t ws_bytes, am_stream_t stream);
int am_scatter_f64(const double* X, int64_t N, int D, int64_t ld, const double* mean,
                   double* scatter, void* ws, size_t ws_bytes, am_stream_t stream);
/* Statistics of B index-gathered subsets of ONE stored matrix in one call (FAD-infinity: the subsets of a candidate set).
 * Subset b is the rows X[idx[offsets[b] + j]], j < n_b = offsets[b + 1] - offsets[b]; no gathered copy is made, the rows are
 * read whole through the index list, and the number of launches does not depend on B (the concatenated list is cut into
 * chunks that never straddle a subset).  Numerics contract of am_stats_f32 / am_stats_f64: f64 means; float32 rows centred
 * in f32, products on the f32 matrix cores in chains of 256 rows, f64 across (at every D: am_stats_f32 itself sums the
 * products in f64 when D < 128); float64 rows entirely in f64.  n_b == 1 ->
 * zero covariance; n_b == 0 -> AM_ERR_BAD_SHAPE.  Indices may repeat and come in any order.
 *   idx      DEVICE, offsets[B] int64 entries        offsets  HOST, B + 1 entries, offsets[0] == 0, increasing
 *   means    DEVICE [B][D]                            covs     DEVICE [B][D][D]
 * An index outside [0, N) is never dereferenced: the row is left out and the FIRST 8 BYTES OF `ws` (an unsigned 64-bit
 * word, zeroed by every call) receive 1 + the largest position in idx that held such an index; 0 = every index was valid.
 * The call itself is asynchronous and returns AM_OK; the caller reads the word with the results.  X as for the plain
 * entry points (float32: 16-byte aligned, ld % 4 == 0, and N * ld * 4 bytes below 4 GiB - the rows are addressed by 32-bit
 * element offsets -, else AM_ERR_BAD_SHAPE; float64: any ld >= D, D <= 8192).  One workspace query serves both. */
size_t am_stats_gather_workspace_bytes(int64_t n_total, int B, int D);
int am_stats_gather_f32(const float* X, int64_t N, int64_t ld, int D,
                        const int64_t* idx, const int64_t* offsets, int B,
                        double* means, double* covs,
                        void* ws, size_t ws_bytes, am_stream_t stream);
int am_stats_gather_f64(const double* X, int64_t N, int64_t ld, int D,
                        const int64_t* idx, const int64_t* offsets, int B,
                        double* means, double* covs,
                        void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * A3  Chan / pairwise merge of two (n, mean, cov) triples in f64
 *                                             reference: data.py:77-94
 *   out may alias the first operand (in-place update, as _update_stats does).
 * ------------------------------------------------------------------------- */
int am_stats_merge_f64(int64_t n1, const double* mean1, const double* cov1,
                       int64_t n2, const double* mean2, const double* cov2,
                       int D, double* out_mean, double* out_cov, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * A1 + A3 + A4 fused for the streaming pipeline   reference: data.py:37-47, 68-72, 77-94
 *   One launch per AudioMetricsData.add(batch) for batches of up to
 *   am_stats_push_max_rows() rows (the embedding pipeline adds <= 32 rows at a
 *   time, embed.py:231-236): batch mean / covariance, Chan merge into the running
 *   (n_old, mean, cov) and the row append.
 *     mean_in  [D]   running mean (ignored when n_old == 0)
 *     mean_out [D]   new mean; must not alias mean_in (other workgroups still read it)
 *     cov      [D,D] running covariance, updated in place (written when n_old == 0)
 *     rows_out       where row n_old of the stored matrix lives (row stride ld_out), or NULL
 *   E needs no alignment (any ld >= D).  Numerics as am_stats_f32: f64 means, f32-centred
 *   values, products summed in f64; merge in f64 with the reference's association.
 * ------------------------------------------------------------------------- */
int am_stats_push_max_rows(void);
int am_stats_push_f32(const float* E, int64_t b, int D, int64_t ld, int64_t n_old,
                      const double* mean_in, double* mean_out, double* cov,
                      float* rows_out, int64_t ld_out, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * A5  Frechet distance                         reference: fad.py:16-31
 *   fd = |mu_x-mu_y|^2 + tr(cov_x) + tr(cov_y) - 2 tr sqrt(cov_x cov_y)
 *   tr sqrt by a coupled Newton-Schulz iteration in f64 on the f64 matrix
 *   cores (the reference uses LAPACK eigvals); stops when |I - ZY|_F <
 *   tol*sqrt(D), when the trace stops growing (rank-deficient inputs) or at
 *   max_iter.  The stopping rule runs on the device; the solve is a stream-
 *   ordered chain of kernels with no host polling.
 *   am_frechet_f64          enqueues blocks of am_frechet_first_block() iterations until the device-side stop code
 *                           is set (one block for well-conditioned inputs) and SYNCHRONISES `stream` once per block.
 *                           out_host (HOST pointer, 4 doubles): { fd, tr_sqrt, iterations, final residual }.
 *   am_frechet_enqueue_f64  the asynchronous building block: enqueues iterations [first_iter, first_iter + n_iter)
 *                           (first_iter == 0 starts the solve; the state lives in `ws`, which the caller keeps alive
 *                           and passes again to continue) and a final kernel that writes out_dev (DEVICE pointer, 5
 *                           doubles): { fd, tr_sqrt, iterations, residual, stop code } - stop code 0 = still running
 *                           (enqueue the next block), 1 converged, 2 trace stalled, 3 zero product, 4 non-finite.
 *                           Never synchronises: a caller can put the solve on a side stream under other work and read
 *                           out_dev when it needs the value.
 * ------------------------------------------------------------------------- */
size_t am_frechet_workspace_bytes(int D);
int am_frechet_f64(const double* mu_x, const double* cov_x,
                   const double* mu_y, const double* cov_y, int D,
                   int max_iter, double tol, double* out_host,
                   void* ws, size_t ws_bytes, am_stream_t stream);
int am_frechet_first_block(void);
int am_frechet_enqueue_f64(const double* mu_x, const double* cov_x,
                           const double* mu_y, const double* cov_y, int D,
                           int first_iter, int n_iter, int max_iter, double tol, double* out_dev,
                           void* ws, size_t ws_bytes, am_stream_t stream);
/* The Frechet distance together with the Gaussian optimal-transport maps between the two sets.  The chain is that of
 * am_frechet_f64 - the same kernels in the same order - so out_host[0..3] (HOST, 5 doubles) equal am_frechet_f64's BIT FOR
 * BIT; out_host[4] is the stop code of am_frechet_enqueue_f64.  The solve's final Z is (cov_x cov_y / norm)^(-1/2), norm =
 * |cov_x cov_y|_F, and from it, in f64 on the matrix cores (the solver's own tile product),
 *   map_xy = sym(cov_y Z) / sqrt(norm)      the symmetric positive definite A with A cov_x A = cov_y
 *   map_yx = sym(Z cov_x) / sqrt(norm)      its inverse (= sym(cov_x Z^T) for a symmetric cov_x)
 * both DEVICE [D][D]; sym(B)_ij = (B_ij + B_ji) / 2 adds the same two numbers for (i, j) and (j, i): EXACTLY symmetric.
 * Hence d tr sqrt(cov_x cov_y) / d cov_x = map_xy / 2 and d / d cov_y = map_yx / 2: the first-order influence of a row
 * (am_frechet_influence_*).  The maps are defined for stop code 1 (converged) only - for any other stop code BOTH ARE
 * FILLED WITH NaN and the distance is still returned (stop code 4: the status is AM_ERR_NO_CONVERGENCE, as am_frechet_f64
 * gives it).  Their accuracy is that of the solve: |map_xy cov_x map_xy - cov_y|_F / |cov_y|_F is about cond(cov_x cov_y)
 * 2^-52.  Workspace: am_frechet_maps_workspace_bytes(D) (= am_frechet_workspace_bytes).  SYNCHRONISES `stream` once per
 * block of iterations, as am_frechet_f64 does; the maps are enqueued behind that and not waited for. */
size_t am_frechet_maps_workspace_bytes(int D);
int am_frechet_maps_f64(const double* mu_x, const double* cov_x,
                        const double* mu_y, const double* cov_y, int D,
                        int max_iter, double tol, double* out_host,
                        double* map_xy, double* map_yx,
                        void* ws, size_t ws_bytes, am_stream_t stream);
/* Per-row influence values  psi_i = c_i^T B c_i + lin^T c_i + c0,  c_i = x_i - mu,  for the N rows of X (row stride ld).
 *   mu [D], B [D][D] (symmetric), lin [D]   DEVICE f64;  c0 a number
 *   psi [N], sums [4]                        DEVICE f64;  sums = { sum psi, sum psi^2, finite psi, non-finite psi }
 * With B = I - map_xy, lin = 2 (mu_x - mu_y), c0 = -tr(B cov_x) over the candidate rows, and B = I - map_yx, lin =
 * -2 (mu_x - mu_y), c0 = -tr(B cov_y) over the reference rows, psi is the first-order influence of a row on the Frechet
 * distance: var(fd) ~ s^2(psi_x) / n + s^2(psi_y) / m.
 * Arithmetic, all in f64 for both entry points: float32 rows are converted on load (exact), so am_frechet_influence_f32
 * returns the SAME BITS as am_frechet_influence_f64 on the same values.  One workgroup owns 64 rows, forms T = C B on
 * v_mfma_f64_16x16x4_f64 column tile by column tile (k ascending) and folds (T_ij + lin_j) c_ij into the row's sum, columns
 * in a fixed order; T never reaches memory.  |psi_i - exact| <= (2 D + 8) 2^-53 (|c|^T |B| |c| + |lin|^T |c| + |c0|).  A row's
 * psi depends on that row alone (not on N, ld or its place in the tile).  A row with a NaN or inf element (or whose psi
 * overflows) gets psi = NaN, counts as non-finite and is left out of the two sums.  The sums are added in a fixed tree -
 * no floating-point atomics: two calls return the same bits.
 * Limits: N >= 1, 1 <= D <= 8192, ld >= D; float32 rows 16-byte aligned with ld % 4 == 0; else AM_ERR_BAD_SHAPE.
 * Workspace: 32 bytes per 64 rows.  Asynchronous. */
size_t am_frechet_influence_workspace_bytes(int64_t N);
int am_frechet_influence_f32(const float* X, int64_t N, int64_t ld, int D,
                             const double* mu, const double* B, const double* lin, double c0,
                             double* psi, double* sums, void* ws, size_t ws_bytes, am_stream_t stream);
int am_frechet_influence_f64(const double* X, int64_t N, int64_t ld, int D,
                             const double* mu, const double* B, const double* lin, double c0,
                             double* psi, double* sums, void* ws, size_t ws_bytes, am_stream_t stream);
/* B independent Frechet distances advancing together: every launch of the Newton-Schulz chain covers all B products (the set
 * index is a grid dimension), each set has its own state, stopping rule and stop code, and the workgroups of a set that has
 * stopped return at once.  Blocks of am_frechet_first_block() iterations are enqueued and `stream` is SYNCHRONISED once per
 * block for the whole batch, while some set's stop code is 0.  Per set the arithmetic is that of am_frechet_enqueue_f64
 * (same tile order, same fixed summation orders): out_dev[b] holds the same five doubles, bit for bit.
 *   mu_x [B][D], cov_x [B][D][D]   DEVICE
 *   mu_y, cov_y                    DEVICE; y_stride_sets == 0: one (mu_y[D], cov_y[D][D]) shared by all sets,
 *                                  y_stride_sets == 1: one per set, laid out as x
 *   out_dev                        DEVICE [B][5]: { fd, tr_sqrt, iterations, residual, stop code } per set
 * Returns AM_ERR_NO_CONVERGENCE naming the first set whose stop code is 4 (non-finite product); all B records are written
 * in that case too.  Workspace: about 6 * B * D * D * 8 bytes. */
size_t am_frechet_batch_workspace_bytes(int B, int D);
int am_frechet_batch_f64(const double* mu_x, const double* cov_x,
                         const double* mu_y, const double* cov_y, int64_t y_stride_sets,
                         int B, int D, int max_iter, double tol, double* out_dev,
                         void* ws, size_t ws_bytes, am_stream_t stream);
/* Per-group ("per-song") Frechet distance in the dual form: B small groups of rows of ONE stored matrix, each scored on its
 * own against one reference (mu_y, cov_y).  Group b is the rows X[idx[offsets[b] + j]], j < n_b; idx == NULL names the rows
 * in stored order (group b = rows offsets[b] .. offsets[b + 1] - 1).  With Xc the centred rows of a group, the non-zero
 * eigenvalues of cov_x cov_y are those of the symmetric n_b x n_b matrix M = Xc cov_y Xc^T / (n_b - 1), so
 *   fd = |mu_x - mu_y|^2 + |Xc|_F^2 / (n_b - 1) + tr cov_y - 2 sum_i sqrt(lambda_i(M))
 * and no D x D matrix is formed per group: the workspace is 2 * n_total * D doubles (Xc and Z = Xc cov_y) plus 32 bytes per
 * group.  The number of launches does not depend on B; the call is asynchronous and deterministic.
 *   idx      DEVICE or NULL                          offsets  HOST, B + 1 entries, offsets[0] == 0
 *   mu_y     DEVICE [D], cov_y DEVICE [D][D] (symmetric)
 *   out_dev  DEVICE [B][5]: { fd, tr_sqrt, sweeps, residual, stop code }; stop code 1 = converged, 2 = sweep cap reached,
 *            4 = non-finite input; residual = off-diagonal norm / |M|_F at the end
 * Every group needs 1 <= n_b <= am_frechet_groups_max_rows() (128: a 128 x 128 f64 matrix is 128 KiB of the CU's 160 KiB
 * LDS), else AM_ERR_BAD_SHAPE naming the group.  Arithmetic, all in f64 for both entry points: float32 rows are converted on
 * load (exact), so am_frechet_groups_f32 returns the SAME BITS as am_frechet_groups_f64 on the same values; column means are
 * added in list order; rows are centred in f64; Z and M come from v_mfma_f64_16x16x4_f64, the upper triangle of M is computed
 * and mirrored; the eigenvalues come from a cyclic Jacobi in LDS (round-robin ordering, eigenvalues only) that runs until
 * the off-diagonal norm is <= 2^-52 |M|_F or 30 sweeps have passed; eigenvalues <= 4 n_b 2^-52 lambda_max count as zero (a
 * centred group always has one exact null vector, duplicate rows add more); the square roots are added in index order.
 * n_b == 1: fd = |dmu|^2 + tr cov_y, tr_sqrt = 0, stop code 1 (one row has zero covariance).
 * An index outside [0, N) is never dereferenced: the row counts as zeros and the FIRST 8 BYTES OF `ws` receive 1 + the
 * largest position in idx that held such an index (0 = all valid), as am_stats_gather_* reports it; the records of the other
 * groups are unaffected.  X: the alignment, ld and 4 GiB rules of am_stats_gather_*. */
int am_frechet_groups_max_rows(void);
size_t am_frechet_groups_workspace_bytes(int64_t n_total, int B, int D);
int am_frechet_groups_f32(const float* X, int64_t N, int64_t ld, int D,
                          const int64_t* idx, const int64_t* offsets, int B,
                          const double* mu_y, const double* cov_y,
                          double* out_dev, void* ws, size_t ws_bytes, am_stream_t stream);
int am_frechet_groups_f64(const double* X, int64_t N, int64_t ld, int D,
                          const int64_t* idx, const int64_t* offsets, int B,
                          const double* mu_y, const double* cov_y,
                          double* out_dev, void* ws, size_t ws_bytes, am_stream_t stream);

/* The Vendi score (Friedman & Dieng 2023; orders q: Pasarkar & Dieng 2023): a reference-free diversity number, "the
 * effective number of distinct samples".  For n rows x_i with G = X X^T accumulated in f64 (float32 rows are converted on
 * load, which is exact: the _f32 and _f64 entry points return the SAME BITS on the same values):
 *   AM_VENDI_COSINE    K_ij = G_ij / (sqrt(G_ii) sqrt(G_jj))
 *   AM_VENDI_GAUSSIAN  K_ij = exp(-gamma max(G_ii + G_jj - 2 G_ij, 0)), gamma = 1 / (2 bw^2), the rows as they are
 * with K_ii = 1 exactly; M = K / n is symmetric PSD with trace 1 and eigenvalues lambda_i.  Eigenvalues <= zero_tol *
 * lambda_max count as zero, rank = the number that remain, and over those, in descending order,
 *   order 1: exp(-sum lambda ln lambda)     order inf: 1 / lambda_max     other q > 0: (sum lambda^q)^(1 / (1 - q)).
 * zero_tol DEPENDS ON THE ROUTE: the per-group Jacobi resolves null eigenvalues at rounding level and uses
 * 4 n_b 2^-52; the eigenvalues of the whole-set matrices come from am_eigh_sym_f64, whose pinned accuracy is 1e-10 lambda_0,
 * so callers of am_vendi_gram_* / am_vendi_moment_* use zero_tol = 1e-10.  The rule matters for q < 1: a null eigenvalue
 * left at 1e-17 contributes (1e-17)^0.1 = 0.02, and duplicate rows make exact null vectors.
 * gamma_dev != NULL (a float32 DEVICE scalar holding a median squared distance, as the KAD kernels take it): gamma =
 * 0.5 / (double)*gamma_dev, no host synchronisation; else the host double `gamma` (finite, > 0) is used.  Cosine ignores both.
 *
 * am_vendi_groups_*: B groups of rows of ONE stored matrix, the group-list protocol of am_frechet_groups_* (idx DEVICE or
 * NULL = stored order, offsets HOST; an index outside [0, N) is never dereferenced, counts as a zero row and is reported
 * through the first 8 bytes of `ws`), 1 <= n_b <= am_vendi_groups_max_rows() (128).  One workgroup per group: the rows are
 * gathered straight from X (no copy), the upper triangle of G comes from v_mfma_f64_16x16x4_f64 and is mirrored in LDS, the
 * kernel transform is applied there, and the cyclic Jacobi of am_frechet_groups_* (round-robin, stop at off-norm <= 2^-52
 * |M|_F, at most 30 sweeps) gives the eigenvalues.
 *   out_rec    DEVICE [B][8]: { vendi (order 1), entropy, rank, lambda_max, sweeps, residual, stop code, 0 }; stop codes as
 *              am_frechet_groups_*: 1 = converged, 2 = sweep cap, 4 = non-finite input
 *   out_evals  DEVICE [n_total]: each group's eigenvalues at its list positions, descending, thresholded ones as 0.0
 * n_b == 1: vendi = 1, entropy 0, rank 1, no sweeps, stop code 1.  A row of zero norm (cosine) or with a non-finite element:
 * NaN record and eigenvalues for ITS group, stop code 4; no other group is affected.  No floating-point atomics, fixed
 * reduction orders: a group's record does not depend on B, its neighbours, idx versus stored order, or the row type.
 *
 * am_vendi_gram_*: out_m DEVICE [n][n] = K / n for the rows idx[0..n) (idx == NULL: rows 0 .. n - 1), n <=
 * am_vendi_gram_max_rows() (2048, else AM_ERR_BAD_SHAPE): upper 64 x 64 tiles computed and mirrored (exactly symmetric),
 * diagonal exactly 1 / n, every element written once.
 * am_vendi_moment_*: out_s DEVICE [D][D] = (1 / n) sum_i x_i x_i^T / |x_i|^2 over all N rows - the cosine kernel's dual form:
 * K / n and S share their non-zero eigenvalues.  The rows are cut into am_vendi_moment_chunks(N, D) chunks whose partial
 * matrices are folded in chunk order; the upper triangle is computed and mirrored.
 * Both: `ws` opens with TWO flag words - [0] 1 + the position of an index outside [0, N), [1] 1 + the position of a row of
 * zero norm (cosine / moment) or with a non-finite element - or 0; such rows count as zeros. */
enum am_vendi_kernel { AM_VENDI_COSINE = 0, AM_VENDI_GAUSSIAN = 1 };
int am_vendi_groups_max_rows(void);
size_t am_vendi_groups_workspace_bytes(int64_t n_total, int B, int D);
int am_vendi_groups_f32(const float* X, int64_t N, int64_t ld, int D,
                        const int64_t* idx, const int64_t* offsets, int B,
                        int kernel, double gamma, const float* gamma_dev,
                        double* out_rec, double* out_evals, void* ws, size_t ws_bytes, am_stream_t stream);
int am_vendi_groups_f64(const double* X, int64_t N, int64_t ld, int D,
                        const int64_t* idx, const int64_t* offsets, int B,
                        int kernel, double gamma, const float* gamma_dev,
                        double* out_rec, double* out_evals, void* ws, size_t ws_bytes, am_stream_t stream);
int am_vendi_gram_max_rows(void);
size_t am_vendi_gram_workspace_bytes(int64_t n, int D);
int am_vendi_gram_f32(const float* X, int64_t N, int64_t ld, int D, const int64_t* idx, int64_t n,
                      int kernel, double gamma, const float* gamma_dev,
                      double* out_m, void* ws, size_t ws_bytes, am_stream_t stream);
int am_vendi_gram_f64(const double* X, int64_t N, int64_t ld, int D, const int64_t* idx, int64_t n,
                      int kernel, double gamma, const float* gamma_dev,
                      double* out_m, void* ws, size_t ws_bytes, am_stream_t stream);
int am_vendi_moment_chunks(int64_t n, int D);
size_t am_vendi_moment_workspace_bytes(int64_t n, int D);
int am_vendi_moment_f32(const float* X, int64_t N, int64_t ld, int D,
                        double* out_s, void* ws, size_t ws_bytes, am_stream_t stream);
int am_vendi_moment_f64(const double* X, int64_t N, int64_t ld, int D,
                        double* out_s, void* ws, size_t ws_bytes, am_stream_t stream);

/* A11 APA scalar combination (host arithmetic)  reference: apa.py:22-32 */
double am_apa_f64(double d_y_x, double d_y_xp, double d_x_xp);

/* ---------------------------------------------------------------------------
 * A6-A8  kernel distance, polynomial kernel     reference: kd.py:38-83,112-124,178-187
 *   For each subset s < S: rows idx1[s*m .. s*m+m) of X (features_1) and
 *   idx2[...] of Y (features_2) -> K = (x.y * gamma + coef0)^degree on the three
 *   m x m Gram blocks, unbiased MMD^2:
 *   out_mmd[s] = (sum offdiag Kxx + sum offdiag Kyy)/(m(m-1)) - 2 sum Kxy / m^2.
 *   Dot products in f32 on the matrix cores, kernel values and sums in f64.
 *   The index table is drawn by the caller (numpy PCG64, kd.py:176,185-186).
 * ------------------------------------------------------------------------- */
/*   Two forms, selected by the SHAPES alone (never by the buffer handed in):
 *     m >= 512, 128 <= D <= 8192, degree == 3: split-f16 form - every gathered row as two f16 planes, three f16 MFMA
 *       stages per 64-element slab on the 256 x 256 engine, error of a dot product <= ~3 * 2^-22 |x||y|;
 *     everything else (and the RBF kernel): f32 MFMA on the 128 x 128 engine.
 *   am_kd_poly_workspace_bytes(S, m, D) is right for every shape.
 *   DEPRECATED: am_kd_workspace_bytes(S, m) predates the split form and covers the f32 form only.  A caller that still sizes
 *   with it gets AM_ERR_WORKSPACE from am_kd_poly_f32 at the shapes of the split form (m >= 512, 128 <= D <= 8192,
 *   degree 3) - am_last_error() names the size am_kd_poly_workspace_bytes would have given - and never a silently different
 *   kernel: the form, and with it the bits, depend on the shapes alone.  Kept for the RBF entry point's callers of round 2;
 *   new code uses am_kd_poly_workspace_bytes / am_kd_rbf_workspace_bytes. */
size_t am_kd_workspace_bytes(int S, int m);
size_t am_kd_poly_workspace_bytes(int S, int m, int D);
int am_kd_poly_f32(const float* X, int64_t N1, int64_t ldx,
                   const float* Y, int64_t N2, int64_t ldy, int D,
                   const int64_t* idx1, const int64_t* idx2, int S, int m,
                   double gamma, double coef0, int degree,
                   double* out_mmd, void* ws, size_t ws_bytes, am_stream_t stream);

/* The subset index table of A8 (host arithmetic, host pointers): idx1[S][m], idx2[S][m] exactly as the reference draws
 * them - `rng = np.random.default_rng(seed)`; per subset `rng.choice(n1, m, replace=False)` then
 * `rng.choice(n2, m, replace=False)` (kd.py:176,185-186) - from the PCG64 state numpy seeds (state and increment as two
 * 64-bit halves each).  A restatement of numpy 2.x's Generator.choice (Floyd's algorithm / tail shuffle on Lemire-
 * bounded 32-bit draws); 200 draws take ~1 ms instead of ~10 ms of Python-level calls. */
int am_kd_draw_indices(uint64_t state_hi, uint64_t state_lo, uint64_t inc_hi, uint64_t inc_lo,
                       int64_t n1, int64_t n2, int S, int m, int64_t* idx1, int64_t* idx2);

/* RBF variant (reference kd.py:86-109, selected with kernel_type="rbf"): K = exp(-|x-y|^2 / (2 sigma^2)),
 * squared distances |x|^2 + |y|^2 - 2 x.y with f64 norms and the f32 matrix-core dot product. */
size_t am_kd_rbf_workspace_bytes(int S, int m);
int am_kd_rbf_f32(const float* X, int64_t N1, int64_t ldx,
                  const float* Y, int64_t N2, int64_t ldy, int D,
                  const int64_t* idx1, const int64_t* idx2, int S, int m, double sigma,
                  double* out_mmd, void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * Kernel Audio Distance (Chung et al. 2025): unbiased MMD^2 between two WHOLE sets with a Gaussian kernel whose
 * bandwidth is the median pairwise distance of the reference set.  Two building blocks (csrc/kad.hip, f32 tile engine):
 *
 * Squared distance of a pair, in both:  d2 = max((|a|^2 + |b|^2) - 2 dot(a, b), 0)  in f64, with f64 squared norms and
 * the f32 matrix-core dot product (the arithmetic of the RBF kernel distance above).
 *
 * am_pairwise_select_f32: *out_d2 (DEVICE) = the element of 0-based `rank` among the float32 keys rn32(d2(x_i, x_j)) of the
 *   N (N - 1) / 2 unordered pairs i < j in ascending order; rank < 0 = the lower median, rank (P - 1) / 2
 *   (torch.median's convention).  Rounding is monotone: the result equals the rounded f64 order statistic.  A pair whose
 *   d2 is NaN or +inf (a non-finite row) has key +inf.  Exact: a radix select in three histogram passes (11 / 10 / 10
 *   bits) over the recomputed upper-triangular tiles, bin totals in 64 bits; no N x N matrix exists at any time.  The
 *   whole call is stream-ordered, never synchronises with the host and returns no value to it.
 *   N < 2 or rank >= P -> AM_ERR_BAD_SHAPE; N * ld * 4 bytes >= 4 GiB -> AM_ERR_BAD_SHAPE (one buffer descriptor spans the
 *   matrix, as for the gathered statistics above).
 *
 * am_mmd_rbf_f32: out_sums (DEVICE, 3 doubles) = {Sxx, Syy, Sxy} of K = exp(-d2 gamma):  Sxx / Syy over the ordered pairs
 *   i != j of X / Y, Sxy over all N1 N2 pairs.  `blocks` is a mask of AM_MMD_XX | AM_MMD_YY | AM_MMD_XY; only the slots
 *   it names are written.  bw2_dev != NULL: the kernels read gamma = 0.5 / (double)*bw2_dev on the device and ignore the
 *   `gamma` argument - the output of the select feeds the sums with no host round trip.  Rows are read directly (no
 *   index lists), N1 != N2 allowed, any D >= 1.  Kernel values and every sum in f64; one partial per workgroup, summed in
 *   a fixed order: two calls on the same input give the same bits.  Size limit as for the select.
 *   unbiased MMD^2 = Sxx / (N1 (N1 - 1)) + Syy / (N2 (N2 - 1)) - 2 Sxy / (N1 N2)   (left to the caller).
 * ------------------------------------------------------------------------- */
enum am_mmd_block { AM_MMD_XX = 1, AM_MMD_YY = 2, AM_MMD_XY = 4 };
size_t am_pairwise_select_workspace_bytes(int64_t N, int D);
int am_pairwise_select_f32(const float* X, int64_t N, int64_t ld, int D, int64_t rank,
                           float* out_d2, void* ws, size_t ws_bytes, am_stream_t stream);
size_t am_mmd_rbf_workspace_bytes(int64_t N1, int64_t N2, int D, unsigned blocks);
int am_mmd_rbf_f32(const float* X, int64_t N1, int64_t ldx,
                   const float* Y, int64_t N2, int64_t ldy, int D,
                   const float* bw2_dev, double gamma, unsigned blocks,
                   double* out_sums, void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * Two-sided row sums of the three Gaussian kernel blocks (csrc/mmd_rows.hip, f32 tile engine): what the closed-form
 * standard error of the unbiased MMD^2 and the two-model comparison are built from, for the Gram and exp work of
 * am_mmd_rbf_f32.  With k = exp(-d2 gamma), d2 and gamma / bw2_dev as for am_mmd_rbf_f32:
 *   out_x  DEVICE [N1][2] doubles {w_i, c_i}:  w_i = sum_{j != i} k(x_i, x_j) (AM_MMD_XX),  c_i = sum_j k(x_i, y_j) (AM_MMD_XY)
 *   out_y  DEVICE [N2][2] doubles {v_j, r_j}:  v_j = sum_{l != j} k(y_j, y_l) (AM_MMD_YY),  r_j = sum_i k(x_i, y_j) (AM_MMD_XY)
 * `blocks` is a mask of AM_MMD_XX | AM_MMD_YY | AM_MMD_XY; the slots of blocks it does not name are not written, and out_x
 * (out_y) may be NULL when neither AM_MMD_XX (AM_MMD_YY) nor AM_MMD_XY is named.  sum w = Sxx, sum v = Syy, sum c = sum r =
 * Sxy of am_mmd_rbf_f32 up to the summation order.  Self pairs are excluded by INDEX: duplicated rows stay each other's
 * pairs with k = 1; a set of one row has w (v) = 0.
 * Every 128 x 128 tile is computed ONCE and summed along both axes of the accumulator: XX and YY sweep the upper-triangular
 * tiles (an off-diagonal tile feeds the sums of its P rows and of its Q rows, the diagonal tile its P rows only), XY every
 * tile once (P = X, Q = Y).  The P tiles are swept in bands of 64; after each band the band's Q-side partials are added to
 * running f64 sums in P-tile order, so the workspace holds 1 KiB per row of the larger set whatever the other's size
 * (100 000 x 100 000 rows: about 105 MiB).  No floating-point atomics: two calls give the same bits, and a block's outputs
 * do not depend on which other blocks share the call.  A non-finite row makes every sum it takes part in NaN - its own,
 * every w of its set and every cross sum of the other set - and no other.
 * X, Y, N1 != N2, ld, alignment, any D >= 1, the 4 GiB rule: as for am_mmd_rbf_f32.  A null X / Y or a null output of a named
 * block, a bad mask, alignment or ld, gamma < 0 without bw2_dev -> AM_ERR_BAD_ARG; N1, N2 or D < 1, a set of 4 GiB ->
 * AM_ERR_BAD_SHAPE; AM_ERR_WORKSPACE.  Validated before the first HIP call; stream-ordered, no host synchronisation.
 * ------------------------------------------------------------------------- */
size_t am_mmd_rbf_rows_workspace_bytes(int64_t N1, int64_t N2, int D, unsigned blocks);
int am_mmd_rbf_rows_f32(const float* X, int64_t N1, int64_t ldx,
                        const float* Y, int64_t N2, int64_t ldy, int D,
                        const float* bw2_dev, double gamma, unsigned blocks,
                        double* out_x,   /* DEVICE [N1][2] = {w_i, c_i} */
                        double* out_y,   /* DEVICE [N2][2] = {v_j, r_j} */
                        void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * Unit-pair sums of the three Gaussian kernel blocks (csrc/mmd_cells.hip, f32 tile engine): what a permutation test of the
 * unbiased MMD^2 is built from.  The MMD^2 of any relabelling of exchangeable units is a quadratic form in the matrix of
 * pair sums between units, so one Gram sweep prices any number of permutations.  k, d2, gamma / bw2_dev as for am_mmd_rbf_f32.
 *   Positions.  A set is a list of positions: position p of X is row idx_x[p] (DEVICE int64 [n1_pos]); idx_x == NULL names
 *     the rows in stored order and then n1_pos must equal N1.  An index outside [0, N1) marks an EMPTY position: it is never
 *     dereferenced, its squared norm counts as +inf (k = 0) and it contributes to no sum.  -1 is the padding marker; any other
 *     out-of-range value is empty too and the FIRST 8 BYTES OF `ws` receive 1 + the largest position (in its own list) that
 *     held one (0 = none), as am_mmd_rbf_groups_f32 reports it.  The same for Y.
 *   Cells.  Cell a of a set is its positions [32 a, 32 a + 32); C = ceil(n_pos / 32).  The value of the cell pair (a, b) is
 *     the sum of k(p, q) over its positions - inside one set without p == q, dropped by POSITION (duplicated rows stay each
 *     other's pairs).  Summed in a fixed order: the 16 values of a lane in register order, then one xor tree over the 64 lanes.
 *   Units.  units_x: HOST, U1 + 1 cell offsets, strictly increasing from 0 to C1 - unit u is the cells [units_x[u],
 *     units_x[u + 1]) - or NULL: every cell is a unit (U1 is ignored).  With offsets the cell sums stay in the workspace and
 *     out[u][v] is the sum of the unit pair's cells in row-major cell order, one thread per element.
 *   out_xx DEVICE [U1][U1], out_yy DEVICE [U2][U2], out_xy DEVICE [U1][U2] doubles, dense.  `blocks` is a mask of AM_MMD_XX |
 *     AM_MMD_YY | AM_MMD_XY; only the named outputs are written and the others may be NULL.
 * XX and YY sweep the upper-triangular tiles and store every cell value to [a][b] and [b][a] (of a diagonal tile the cells
 * a <= b): without unit offsets the output is exactly symmetric, one value written twice.  XY sweeps every tile once.  Both
 * operands are gathered through 32-bit byte-offset tables, dense input included - no gathered copy is made.  Every output
 * element is written exactly once: no partials, no atomics on floating-point data, two calls give the same bits, a block's
 * output does not depend on the other blocks of the call, and the result depends on the position lists only, not on where
 * the rows are stored.  A non-finite row makes exactly the cells (units) of its own cell (unit) row and column NaN.
 * Workspace: the tables, and one cell matrix per named block (8 C^2 bytes: 78 MB at 100 000 positions) for the unit fold.
 * X, Y, ld, alignment, any D >= 1, the 4 GiB rule: as for am_mmd_rbf_f32; 1 <= n_pos < 2^30.  A null X / Y or output of a
 * named block, a bad mask, offsets that do not run from 0 to C, gamma < 0 without bw2_dev -> AM_ERR_BAD_ARG; bad sizes, n_pos
 * != N without a list, an empty unit -> AM_ERR_BAD_SHAPE; AM_ERR_WORKSPACE.  Validated before the first HIP call;
 * stream-ordered, no host synchronisation.
 * ------------------------------------------------------------------------- */
#define AM_MMD_CELL 32
size_t am_mmd_rbf_cells_workspace_bytes(int64_t n1_pos, int64_t n2_pos, int D, unsigned blocks);
int am_mmd_rbf_cells_f32(const float* X, int64_t N1, int64_t ldx, const int64_t* idx_x, int64_t n1_pos,
                         const int64_t* units_x, int U1,      /* HOST, U1 + 1 cell offsets, or NULL: unit = cell */
                         const float* Y, int64_t N2, int64_t ldy, const int64_t* idx_y, int64_t n2_pos,
                         const int64_t* units_y, int U2,
                         int D, const float* bw2_dev, double gamma, unsigned blocks,
                         double* out_xx, double* out_yy, double* out_xy,   /* DEVICE [U1][U1], [U2][U2], [U1][U2] */
                         void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * Whole-set kernel sums under several kernels at once (csrc/mmd_multi.hip, f32 tile engine): the three sums of
 * am_mmd_rbf_f32 for up to AM_MMD_MULTI_MAX scales of one kernel family in ONE Gram pass - the tile work of a block is done
 * once and every scale is one more epilogue value on the same accumulator tile.  With d2 as above and the scales c_s:
 *   AM_MMD_GAUSSIAN   k = exp(-d2 g_s),        g_s = 0.5 / (bw2 * (c_s * c_s))
 *   AM_MMD_LAPLACIAN  k = exp(-sqrt(d2) h_s),  h_s = 1.0 / (c_s * sqrt(bw2))
 *   AM_MMD_ENERGY     k = -sqrt(d2)            nscales must be 1; bw2_dev, bw2 and the scale's value are ignored (the MMD^2
 *                                              of this kernel is the energy distance 2 E|x - y| - E|x - x'| - E|y - y'|)
 * the parameters formed in f64 in exactly that order.  bw2 = (double)*bw2_dev when bw2_dev != NULL (DEVICE float: the output
 * of the select feeds the call with no host round trip), else the `bw2` argument.
 *   out_sums  DEVICE [3][nscales] doubles: out_sums[b * nscales + s], b = 0 Sxx, 1 Syy, 2 Sxy (ordered pairs i != j / all
 *             pairs, as for am_mmd_rbf_f32); only the blocks named by `blocks` are written
 *   scales    HOST, nscales entries, each finite and > 0
 * Grid plan, upper-triangular sweep, f64 norms and summation order are those of am_mmd_rbf_f32, one running sum per scale:
 * the Gaussian sums of scale c equal those of am_mmd_rbf_f32 with gamma = 0.5 / (bw2 * (c * c)) bit for bit, a scale's sums
 * depend neither on the other scales of the call nor on their order, and two calls give the same bits (one f64 partial per
 * workgroup and scale, summed in a fixed order; no floating-point atomics).  A non-finite row makes the sums it takes part
 * in NaN.  X, Y, N1, N2, D, blocks, the 4 GiB rule: as for am_mmd_rbf_f32.  nscales outside 1 .. AM_MMD_MULTI_MAX (the
 * register file holds four scales without scratch memory; a longer grid is several calls) -> AM_ERR_BAD_SHAPE; an unknown
 * kernel, a scale that is not finite and positive, or bw2_dev == NULL with bw2 not finite and positive (except for the
 * energy kernel) -> AM_ERR_BAD_ARG.  Validated before the first HIP call; stream-ordered, no host synchronisation.
 * ------------------------------------------------------------------------- */
enum am_mmd_kernel { AM_MMD_GAUSSIAN = 0, AM_MMD_LAPLACIAN = 1, AM_MMD_ENERGY = 2 };
#define AM_MMD_MULTI_MAX 4
size_t am_mmd_multi_workspace_bytes(int64_t N1, int64_t N2, int D, int nscales, unsigned blocks);
int am_mmd_multi_f32(const float* X, int64_t N1, int64_t ldx,
                     const float* Y, int64_t N2, int64_t ldy, int D,
                     int kernel, const float* bw2_dev, double bw2,
                     const double* scales, int nscales, unsigned blocks,
                     double* out_sums, void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * Per-group Kernel Audio Distance (csrc/kad_groups.hip, f32 tile engine): the Gaussian kernel sums of B groups of rows of
 * one stored matrix X, each group on its own against the one reference set Y, in ONE call whose number of launches does not
 * depend on B.  Group b is the rows X[idx[offsets[b] + j]], j < n_b; idx == NULL names the rows in stored order.  With
 * k(a, b) = exp(-d2(a, b) gamma) in the arithmetic of am_mmd_rbf_f32 (f64 norms, f32 matrix-core dot product, exp in f64):
 *   row sums   c_i = sum_j k(x_i, y_j) over all N2 reference rows,   w_i = sum_{j in group(i), j != i} k(x_i, x_j)
 *   out_groups[b] = { Sxx_b = sum_{i in b} w_i,  Sxy_b = sum_{i in b} c_i }          (DEVICE [B][2])
 *   out_rows[p]   = { w_p, c_p } for list position p, i.e. in LIST order            (DEVICE [n_total][2], or NULL)
 *   unbiased MMD^2 of group b = Sxx_b / (n_b (n_b - 1)) + Syy / (N2 (N2 - 1)) - 2 Sxy_b / (n_b N2)   (left to the caller;
 *   Syy from am_mmd_rbf_f32(blocks = AM_MMD_YY); n_b == 1 has no unbiased estimate, its Sxx_b is 0).
 * The cross pass does the Gram work of one Sxy pass of am_mmd_rbf_f32 with the candidate rows gathered through the list (no
 * gathered copy is made); the within pass covers, per 128-position tile, the tiles of the tile's own groups, masked to equal
 * groups.  A lane keeps one f64 running sum per candidate row; a workgroup's sums are combined in a fixed order and written
 * to a slot of its own, a row's chunks are added in chunk order and a group's rows by strided sums and a tree: no atomics,
 * two calls on the same input give the same bits, and the result depends on the list order only - not on where the rows
 * are stored (idx == NULL on a group-ordered store and a permutation idx into a shuffled store give the same bits).
 *   idx      DEVICE or NULL                          offsets  HOST, B + 1 entries, offsets[0] == 0, strictly increasing
 *   bw2_dev  DEVICE float or NULL: gamma = 0.5 / (double)*bw2_dev is formed on the device and `gamma` is ignored
 * Any n_b >= 1 is allowed, with no upper bound (a group may span many tiles); n_total = offsets[B] < 2^30.
 * An index outside [0, N1) is never dereferenced: the row counts as zeros and the FIRST 8 BYTES OF `ws` receive 1 + the
 * largest position in idx that held such an index (0 = all valid), as am_stats_gather_* reports it; the records of the other
 * groups are unaffected.  A non-finite candidate row makes the sums of its own group NaN and touches no other group; a
 * non-finite reference row makes every Sxy_b NaN.  X, Y: the alignment, ld and 4 GiB rules of am_mmd_rbf_f32; N2 >= 2.
 * Everything is validated before the first HIP call (AM_ERR_BAD_ARG / AM_ERR_BAD_SHAPE name the argument, AM_ERR_WORKSPACE
 * the size wanted); the call is asynchronous.
 * ------------------------------------------------------------------------- */
size_t am_mmd_rbf_groups_workspace_bytes(int64_t n_total, int B, int64_t N2, int D);
int am_mmd_rbf_groups_f32(const float* X, int64_t N1, int64_t ldx,
                          const int64_t* idx, const int64_t* offsets, int B,
                          const float* Y, int64_t N2, int64_t ldy, int D,
                          const float* bw2_dev, double gamma,
                          double* out_groups, double* out_rows,
                          void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * Dependence of two PAIRED sets (csrc/pair_dependence.hip, f32 tile engine): the row sums from which distance covariance /
 * correlation and HSIC / CKA are formed, without an N x N matrix.  Row i of X (N x Dx) belongs to row i of Y (N x Dy); with
 * `perm` (DEVICE, N entries) to row perm[i] of Y, addressed through the list - no gathered copy is made.  For every ordered
 * pair i != j, dropped by INDEX (duplicated rows stay each other's pairs):
 *   a_ij = k(x_i, x_j), b_ij = k(y_perm[i], y_perm[j]), k by `kernel` in the arithmetic of am_mmd_multi_f32 at scale 1
 *     AM_MMD_ENERGY     +sqrt(d2)  (the distance: distance covariance; bandwidths ignored)
 *     AM_MMD_GAUSSIAN   exp(-d2 g),        g = 0.5 / bw2
 *     AM_MMD_LAPLACIAN  exp(-sqrt(d2) h),  h = 1.0 / sqrt(bw2)
 *   with bw2 = bw2x on the X side and bw2y on the Y side, each (double)*bw2?_dev when that DEVICE float is given.
 *   out_rows  DEVICE [N][5] doubles: A_i = sum_j a_ij, B_i = sum_j b_ij, H_i = sum_j a_ij b_ij, AA_i = sum_j a_ij^2,
 *             BB_i = sum_j b_ij^2 - product and sums in f64
 *   out_sums  DEVICE [8] doubles: sum A_i, sum B_i, sum H_i, sum AA_i, sum BB_i, sum A_i B_i, the number of finite rows, the
 *             number of non-finite rows
 * Both Grams of a 128 x 128 tile are formed in one workgroup, the X dot products parked as raw f32 accumulators while the Y
 * slabs run; the full square is swept (every ordered pair once).  A row's sums are held per lane, folded in a fixed order and
 * written per chunk of Q tiles (at most 16 chunks), the chunks added in chunk order: no floating-point atomics, two calls
 * give the same bits, swapping the sets swaps A / B and AA / BB exactly.  A row with a non-finite element on either side
 * makes every value it takes part in NaN and is counted in out_sums[7]; so is an entry of perm outside [0, N), which is
 * never dereferenced.  X, Y: 16-byte aligned, ld % 4 == 0, ld >= D, N * ld * 4 < 4 GiB each; N >= 4; any Dx, Dy >= 1.  A null
 * pointer, an unknown kernel, a misaligned set, or (Gaussian, Laplacian) a bandwidth that is neither given on the device nor
 * finite and positive -> AM_ERR_BAD_ARG; bad sizes -> AM_ERR_BAD_SHAPE; AM_ERR_WORKSPACE names the size wanted (the norms, the
 * offset table and 5 x chunks x 8 bytes per row: 64 MB at 100 000 rows).  Validated before the first HIP call;
 * stream-ordered, no host synchronisation.
 * ------------------------------------------------------------------------- */
size_t am_pair_dependence_workspace_bytes(int64_t N, int Dx, int Dy);
int am_pair_dependence_f32(const float* X, int64_t N, int64_t ldx, int Dx,
                           const float* Y, int64_t ldy, int Dy,
                           const int64_t* perm,            /* DEVICE [N] or NULL */
                           int kernel, const float* bw2x_dev, double bw2x, const float* bw2y_dev, double bw2y,
                           double* out_rows, double* out_sums,
                           void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * Kernel Audio Distance on float64 rows (csrc/kad_f64.hip, the f64 tile engine of the other *_f64 entry points: 64 x 64 tiles
 * on v_mfma_f64_16x16x4_f64).  The three calls above with `const double*` rows and the same argument lists; taken when BOTH
 * sets hold float64 rows.  Every step is f64: squared norms, the matrix-core dot product,
 *   select:  d2 = max(fma(-2, dot, |a|^2 + |b|^2), 0), a NaN distance (a non-finite row) carried as +inf
 *   sums:    the same d2 with a NaN left in place, k = exp(-d2 gamma): as in the f32 forms a non-finite row makes the sums
 *            it takes part in NaN.
 * Rows need no alignment (8-byte loads; any ld >= D) and no buffer descriptor spans a matrix: the 4 GiB rule of the f32
 * forms does not apply (N, N1, N2 < 2^31).
 *
 * am_pairwise_select_f64: the contract of am_pairwise_select_f32 - *out_d2 is a FLOAT32, rn32 of the f64 order statistic
 *   (rounding is monotone: select-then-round = round-then-select), keys bits(rn32(d2)) with NaN and overflow +inf, three
 *   radix passes of 11 / 10 / 10 bits over the upper-triangular tiles, bin totals in 64 bits, no host synchronisation.
 * am_mmd_rbf_f64: the contract of am_mmd_rbf_f32 (`blocks`, bw2_dev - still a DEVICE float: gamma = 0.5 / (double)*bw2_dev
 *   is formed on the device -, one f64 partial per workgroup summed in a fixed order: same input, same bits).
 * am_mmd_rbf_groups_f64: the contract of am_mmd_rbf_groups_f32 (list protocol, flag word in the first 8 bytes of `ws`, an
 *   out-of-range index counts as a zero row, out_groups / out_rows, results that depend on the list order only, same bits
 *   on every call); tiles hold 64 list positions; D <= 8192; n_total < 2^30; N2 >= 2.
 * ------------------------------------------------------------------------- */
size_t am_pairwise_select_f64_workspace_bytes(int64_t N, int D);
int am_pairwise_select_f64(const double* X, int64_t N, int64_t ld, int D, int64_t rank,
                           float* out_d2, void* ws, size_t ws_bytes, am_stream_t stream);
size_t am_mmd_rbf_f64_workspace_bytes(int64_t N1, int64_t N2, int D, unsigned blocks);
int am_mmd_rbf_f64(const double* X, int64_t N1, int64_t ldx,
                   const double* Y, int64_t N2, int64_t ldy, int D,
                   const float* bw2_dev, double gamma, unsigned blocks,
                   double* out_sums, void* ws, size_t ws_bytes, am_stream_t stream);
size_t am_mmd_rbf_groups_f64_workspace_bytes(int64_t n_total, int B, int64_t N2, int D);
int am_mmd_rbf_groups_f64(const double* X, int64_t N1, int64_t ldx,
                          const int64_t* idx, const int64_t* offsets, int B,
                          const double* Y, int64_t N2, int64_t ldy, int D,
                          const float* bw2_dev, double gamma,
                          double* out_groups, double* out_rows,
                          void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * A9  k-NN radii                                reference: prdc.py:4-14, data.py:60-66
 *   out_r[i] = (k+1)-th smallest Euclidean distance from row i of X to the M
 *   rows of Y (Y == X for the reference's self-distance use; a multi-GPU
 *   caller passes its row shard as X and the gathered set as Y).
 *   Distances follow torch.cdist's matmul form  sqrt(max(|x|^2+|y|^2-2x.y, 0))
 *   in f32; no N x M matrix is materialised.  1 <= k, k+1 <= M (k > AM_MAX_K: one row at a time on the vector ALUs,
 *   same values; a correctness path - the reference's evaluate() caps k at 10).
 *   Y == X with >= 6144 rows (D >= 256) / 8192 rows (128 <= D < 256) / 12000 rows (32 <= D < 128) / 16384 rows (D < 32), D <= 4096, runs as a scaled-f16 MFMA FILTER sweep over half of the tile pairs
 *   followed by an f32 evaluation - with the arithmetic of the exact kernel - of the pairs its error bound cannot
 *   rule out (csrc/pairwise_fast.h): the radii are bit-identical to the exact kernels', which remain the path for
 *   the other shapes and the automatic fallback - per row (a row whose buffers overflowed), or for the whole call when
 *   device-side checks find that the f16 values cannot separate the rows' neighbours (tightly clustered data) or that the
 *   operands cannot be scaled into f16 (non-finite values).  A row with a non-finite element is nobody's neighbour (its
 *   distances count as +inf, where torch carries NaN); its own radius is +inf.
 * ------------------------------------------------------------------------- */
size_t am_knn_workspace_bytes(int64_t N, int64_t M, int D, int k);
int am_knn_radii_f32(const float* X, int64_t N, int64_t ldx,
                     const float* Y, int64_t M, int64_t ldy, int D, int k,
                     float* out_r, void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * k-nearest-neighbour SEARCH (csrc/knn_search.hip, f32 tile engine)          no counterpart in the reference
 *   For every row i of X the k nearest rows of Y: out_dist[i * k + s] = the s-th smallest distance (ascending),
 *   out_idx[i * k + s] = the row of Y it belongs to (int64).  The radii above answer "how far"; this answers "which
 *   rows" - memorisation audits, per-sample inspection, nearest-neighbour ratio tests - without an N x M matrix.
 *   Arithmetic of a pair: exactly that of the exact k-NN kernel,  d2 = max(fmaf(-2, <x, y>, |x|^2 + |y|^2), 0)  in f32 with
 *   the same row norms and inner order, so every squared distance has the bits am_knn_radii_f32 works with:
 *   column k of a (k + 1)-search equals the radius of nearest_k = k bit for bit.  squared != 0: d2 itself; else sqrt_rn(d2).
 *   Order: by distance, ties by the SMALLEST row index of Y (one unsigned compare on the 64-bit key
 *   bits(d2) << 32 | column) - independent of chunking and launch geometry: two calls return the same bits.
 *   self_offset >= 0: column i + self_offset is skipped for row i (X a row shard of Y starting at row self_offset;
 *   0 for X == Y).  Exclusion is by INDEX, not by a zero distance: duplicates of a row remain its neighbours.
 *   self_offset < 0: nothing is skipped.
 *   Fewer than k finite candidates (M < k, M - 1 < k with exclusion, rows with non-finite elements - a NaN distance
 *   counts as +inf, as for the radii): the trailing entries are distance +inf, index -1.
 *   1 <= k <= 32 (else AM_ERR_BAD_SHAPE); M < 2^32 - 1; X, Y as for am_knn_radii_f32 (16-byte aligned, ld % 4 == 0,
 *   ld >= D).  Workspace: the row norms and uint64 [am_knn_search_chunks][N][8 / 16 / 32] partial lists.  Everything is
 *   validated before the first HIP call; the call is asynchronous.
 * ------------------------------------------------------------------------- */
size_t am_knn_search_workspace_bytes(int64_t N, int64_t M, int D, int k);
int am_knn_search_chunks(int64_t N, int64_t M, int D, int k);      /* column chunks the plan uses (tests, tools) */
int am_knn_search_f32(const float* X, int64_t N, int64_t ldx, const float* Y, int64_t M, int64_t ldy, int D, int k,
                      int64_t self_offset, int squared, float* out_dist, int64_t* out_idx,
                      void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * k-nearest-neighbour search that LEAVES A GROUP OUT (csrc/knn_search.hip)       no counterpart in the reference
 *   Every row of X and of Y carries one int32 label (the song a window was cut from).  For every row i of X the k nearest
 *   rows of Y whose label DIFFERS from x_group[i]: column j is skipped for row i iff x_group[i] == y_group[j], for any
 *   int32 values (labels are moved and compared for equality, never computed with).  There is no self offset: a set
 *   searched against itself with its own labels excludes each row through its own group.
 *   Everything else is am_knn_search_f32: the arithmetic of a pair and the bits of every distance, squared, the order
 *   (ties to the SMALLEST row index of Y, independent of chunking: two calls return the same bits), the chunk plan
 *   (am_knn_search_chunks), the partial lists and the merge kernel, (+inf, -1) where a row has fewer than k admissible
 *   finite candidates; a row with a non-finite element has no neighbours and is nobody's neighbour.
 *   x_group, y_group: device pointers, N and M values; null -> AM_ERR_BAD_ARG.  1 <= k <= 32 (else AM_ERR_BAD_SHAPE);
 *   M < 2^32 - 1; X, Y as for am_knn_search_f32.  Workspace (caller-owned; the library allocates nothing): the row norms
 *   and uint64 [am_knn_search_chunks][N][8 / 16 / 32] partial lists.  Everything is validated before the first HIP call;
 *   the call is asynchronous.
 * ------------------------------------------------------------------------- */
size_t am_knn_search_groups_workspace_bytes(int64_t N, int64_t M, int D, int k);
int am_knn_search_groups_f32(const float* X, int64_t N, int64_t ldx, const int32_t* x_group,
                             const float* Y, int64_t M, int64_t ldy, const int32_t* y_group,
                             int D, int k, int squared, float* out_dist, int64_t* out_idx,
                             void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * K-MEANS, the two halves of a Lloyd iteration (csrc/kmeans.hip)              no counterpart in the reference
 *   Every pointer below is a DEVICE pointer, `inertia` included: an iteration needs no read-back.  Everything is validated
 *   before the first HIP call; the calls are asynchronous.  No floating-point atomics: two calls return the same bits.
 *
 *   ASSIGN.  labels[i] = the nearest of the K rows of C (int64), d2[i] = its squared distance - the tile kernel and the
 *   arithmetic of am_knn_search_f32 at k = 1, squared: d2 = max(fmaf(-2, <x, c>, |x|^2 + |c|^2), 0) in f32 with the same
 *   row norms and inner order, the same bits.  Ties go to the SMALLEST centroid index whatever the chunking.  A row
 *   without a finite distance (a non-finite element in it, or in every centroid; a NaN distance counts as +inf) gets
 *   label -1 and d2 = +inf; a non-finite centroid is nobody's label.  *inertia = the sum of d2 over the rows that have a
 *   label, in f64, added in a fixed tree.  K < 2^32 - 1; X, C as for am_knn_search_f32 (16-byte aligned, ld % 4 == 0,
 *   ld >= D).  Workspace: the row norms, uint64 [column chunks][N] keys and one f64 per 256 rows.
 *
 *   UPDATE.  C_new[c] = the mean of the rows with label c: summed in f64 in the order of `order`, divided in f64, rounded
 *   to f32 once; counts[c] = their number.  A cluster without rows copies C_old[c] bit for bit and reports 0.
 *   order   int64 [N]      the row indices sorted by label, stable (rows of one cluster in ascending row order)
 *   offsets int64 [K + 1]  cluster c is order[offsets[c] .. offsets[c + 1]); rows with label -1 come FIRST, in
 *                          order[0 .. offsets[0]), and are not read
 *   labels  int64 [N]      the labels `order` and `offsets` were built from (the kernel looks the cluster of a position
 *                          up as labels[order[p]]); a label outside 0 .. K - 1 is skipped
 *   `order` is cut into segments of 64 positions; a cluster that crosses segments is summed per segment and the partial
 *   sums are added in segment order.  Every index taken from the three arrays is range-checked before it addresses
 *   memory.  C_new may be C_old.  Workspace: f64 [ceil(N / 64)][2][D rounded up to 4].
 * ------------------------------------------------------------------------- */
size_t am_kmeans_assign_workspace_bytes(int64_t N, int64_t K, int D);
int am_kmeans_assign_f32(const float* X, int64_t N, int64_t ldx, const float* C, int64_t K, int64_t ldc, int D,
                         int64_t* labels, float* d2, double* inertia,
                         void* ws, size_t ws_bytes, am_stream_t stream);
size_t am_kmeans_update_workspace_bytes(int64_t N, int64_t K, int D);
int am_kmeans_update_f32(const float* X, int64_t N, int64_t ldx, int D,
                         const int64_t* labels, const int64_t* order, const int64_t* offsets, int64_t K,
                         const float* C_old, int64_t ldc_old, float* C_new, int64_t ldc_new, int64_t* counts,
                         void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * SOFT-MIN, one log-domain Sinkhorn half-step (csrc/softmin.hip)              no counterpart in the reference
 *   For every row x_i of X against the M rows of Y, column potentials g (DEVICE double[M]; NULL = zeros) and a temperature
 *   eps (HOST double):
 *     T_i = -eps log( (1 / M) sum_j exp( (g_j - d2(x_i, y_j) / 2) / eps ) )
 *   One Gram pass on the exact f32 tile engine, no N x M matrix: the sweep and the d2 bits of am_kmeans_assign_f32 /
 *   am_knn_search_f32(squared) (f32 norms, same inner order, max(., 0), NaN -> +inf).  Per pair z = fmaf(-d2, (float)(0.5 /
 *   eps), (float)(g_j / eps)) in f32; per row an online log-sum-exp: a running f32 maximum of z and the f64 sum of
 *   exp(z - max), exp in f64.  eps log M is added once, in f64, at the end.  A column at distance +inf contributes exactly 0.
 *     out[i]   = damping * prev[i] + (1 - damping) * T_i       DEVICE double[N]; damping (HOST double) in [0, 1); damping == 0
 *                writes T_i itself.  prev: DEVICE double[N], may be NULL when damping == 0; out may be prev.
 *     stats    OPTIONAL (may be NULL) DEVICE double[2], overwritten: { max_i |out[i] - prev[i]| (prev NULL: |out[i]|),
 *                max_i |out[i]| } - the two numbers a Sinkhorn step's stop rule needs, so that a step reads nothing back
 *   Partial (max, sum) pairs of the lanes and of the column chunks are joined in a fixed order, the two maxima are integer
 *   maxima over bit patterns: no floating-point atomics, two calls return the same bits.  X may be Y (same pointer, rows and
 *   stride: the norms are computed once).  eps must be finite and > 0 with 0.5 / eps a normal float32 number.  X, Y as for
 *   am_knn_search_f32 (16-byte aligned, ld % 4 == 0, ld >= D).  Workspace: the row norms, one float per column and
 *   [column chunks][N] (float, double) partials.  Everything is validated before the first HIP call; the call is
 *   asynchronous.
 * ------------------------------------------------------------------------- */
size_t am_softmin_workspace_bytes(int64_t N, int64_t M, int D);
int am_softmin_f32(const float* X, int64_t N, int64_t ldx, const float* Y, int64_t M, int64_t ldy, int D,
                   const double* g, double eps, const double* prev, double damping, double* out, double* stats,
                   void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * FEATURE LIKELIHOOD of a mixture of isotropic Gaussians on the rows of G (csrc/fld.hip)   no counterpart in the reference
 *   The two sweeps of the feature likelihood divergence (Jiralerspong et al., NeurIPS 2023).  G: the M centres, theta:
 *   DEVICE double[M], theta_j = log sigma_j^2; h_j = 0.5 exp(-theta_j) and c_j = (D / 2) theta_j are rounded to f32 once per
 *   call.  Per pair, in f32 on the exact f32 tile engine, no N x M matrix in either direction:
 *     d2   = max(fmaf(-2, <x_i, g_j>, |x_i|^2 + |g_j|^2), 0), NaN -> +inf: the bits of am_knn_search_f32(squared)
 *     z_ij = fmaf(-d2, h_j, -c_j)        the same bits in both sweeps
 *   A centre with a non-finite element, or with a theta_j for which h_j is no normal float32 number, sits at distance +inf
 *   from every row: it contributes exactly 0 everywhere.
 *
 *   LOGLIK.  Rows are the evaluated points X, columns the centres.
 *     out_loglik[i] = logsumexp_j z_ij - log M - (D / 2) log 2 pi      DEVICE double[N]; the online log-sum-exp of
 *                     am_softmin_f32 (a running f32 maximum, the f64 sum of exp(z - max), exp in f64; the constants are added
 *                     once, in f64, at the end); -inf for a row with a non-finite element (every distance +inf)
 *     stats         = { sum of the finite out_loglik, rows with a finite one, rows without }   DEVICE double[3], overwritten
 *   Lane and chunk partials are joined in a fixed order and the sum over the rows is a fixed tree over blocks of 256 rows
 *   added in block order.
 *
 *   GRAD.  The swapped sweep - rows are the centres, columns the evaluated rows X - and one Adam step on theta.
 *     loglik        DEVICE double[N]: out_loglik of a LOGLIK call with the same G, theta and X (the column's log-sum-exp is
 *                   loglik + log M + (D / 2) log 2 pi, kept as two f32 halves); a column whose value is not finite and a
 *                   padded column add exactly 0 to both sums
 *     r_ij = exp(z_ij - lse_i) in f64,   A_j = sum_i r_ij,   B_j = sum_i r_ij d2_ij      f64, in a fixed order
 *     n_finite      DEVICE double[1]: stats[1] of that LOGLIK call (0: the gradient is 0)
 *     grad_j        = -(h_j B_j - (D / 2) A_j) / n_finite, h_j = 0.5 exp(-theta_j) in f64
 *     Adam, beta = (0.9, 0.999), eps = 1e-8, bias-corrected with 1 - beta^step (step >= 1, HOST):
 *       m <- 0.9 m + 0.1 grad;  v <- 0.999 v + 0.001 grad^2;  theta_out = clamp(theta - lr (m / bc1) / (sqrt(v / bc2) + eps),
 *       theta_min, 30), every operation rounded once, in this order.  adam_m, adam_v: DEVICE double[M], updated in place;
 *       theta_out: DEVICE double[M], may be theta.  theta_min (HOST) must be finite, at most 30, with 0.5 exp(-theta_min) a
 *       normal float32 number.
 *     out_a, out_b  OPTIONAL (may be NULL) DEVICE double[M]: A and B
 *   No floating-point atomics: two calls at the same shapes return the same bits.  X, G as for am_knn_search_f32 (16-byte
 *   aligned, ld % 4 == 0, ld >= D).  Workspace: the norms, three floats per column, and [column chunks][rows] partials
 *   ((float, double) in LOGLIK, two doubles in GRAD).  Everything is validated before the first HIP call; the calls are
 *   asynchronous and read nothing back.
 * ------------------------------------------------------------------------- */
size_t am_fld_loglik_workspace_bytes(int64_t N, int64_t M, int D);
int am_fld_loglik_f32(const float* X, int64_t N, int64_t ldx, const float* G, int64_t M, int64_t ldg, int D,
                      const double* theta, double* out_loglik, double* stats,
                      void* ws, size_t ws_bytes, am_stream_t stream);
size_t am_fld_grad_workspace_bytes(int64_t M, int64_t N, int D);
int am_fld_grad_f32(const float* G, int64_t M, int64_t ldg, const float* X, int64_t N, int64_t ldx, int D,
                    const double* theta, const double* loglik, const double* n_finite, double* adam_m, double* adam_v,
                    int64_t step, double lr, double theta_min, double* theta_out, double* out_a, double* out_b,
                    void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * LOGISTIC PROBES over the stored rows of one set (csrc/logit.hip)                    no counterpart in the reference
 *   The fused pass of the classifier two-sample test: K linear models evaluated on every row of X, all rows of ONE class.
 *     fold    DEVICE int32[N]: -1 = the row takes no part, 0..K-1 = held out of that model (it trains the other K - 1),
 *             K = trains every model; any other value counts as -1
 *     label   HOST: 1 or 0, the class of every row of X; s = +1 for 1, -1 for 0
 *     coef    DEVICE double[K][D + 1]: a_k[0..D-1] in ROW coordinates, then the intercept b_k
 *   Per row i and model k, all in f64 (float32 rows are converted on load, which is exact, so am_logit_pass_f32 returns the
 *   SAME BITS as am_logit_pass_f64 on the same values):
 *     z_ik = b_k + sum_d a_kd x_id  (the products summed first, in ascending groups of four columns on
 *            v_mfma_f64_16x16x4_f64, b_k added last),   t = s z,
 *     loss = max(-t, 0) + log1p(exp(-|t|)),   r = -s / (1 + exp(t))      (= p - y)
 *   Outputs, all overwritten:
 *     sums    DEVICE double[K][D + 2]: sum r x_d (d = 0..D-1), sum r, sum loss, over the rows that TRAIN model k - fold in
 *             0..K, fold != k, every element finite
 *     z_out   DEVICE double[N] or NULL: z under the model of the row's own fold; NaN for fold -1, fold K and for a row with
 *             a non-finite element
 *     counts  DEVICE double[2]: rows that took part (fold in 0..K, every element finite), rows with a non-finite element
 *             (whatever their fold)
 *   The kernel takes no weights: within one call the class weight is a constant the caller applies to the sums.
 *   One workgroup owns 64 rows at a time and takes the row blocks g, g + grid, ... in order, grid = min(ceil(N / 64), 256) -
 *   a function of N alone; its partial sums are written once and a second kernel adds the partials in workgroup order.  No
 *   floating-point atomics: two calls return the same bits.  A model's sums and a row's z do not depend on the other models
 *   of the call or on K, and z_out[i] depends on row i and its model alone - not on N, ld or the row's place in a tile.
 *   Limits: N >= 1, 1 <= D <= 8192, 1 <= K <= 16, ld >= D; float32 rows 16-byte aligned with ld % 4 == 0 (AM_ERR_BAD_SHAPE);
 *   a null pointer other than z_out or a label other than 0 / 1 is AM_ERR_BAD_ARG.  Workspace: [grid][K (D + 2) + 2]
 *   doubles.  Everything is validated before the first HIP call; the call is asynchronous and reads nothing back.
 * ------------------------------------------------------------------------- */
size_t am_logit_pass_workspace_bytes(int64_t N, int D, int K);
int am_logit_pass_f32(const float* X, int64_t N, int64_t ld, int D, const int32_t* fold, int label,
                      const double* coef, int K, double* sums, double* z_out, double* counts,
                      void* ws, size_t ws_bytes, am_stream_t stream);
int am_logit_pass_f64(const double* X, int64_t N, int64_t ld, int D, const int32_t* fold, int label,
                      const double* coef, int K, double* sums, double* z_out, double* counts,
                      void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * PER-SAMPLE realism, ball count and rarity on the PRDC manifold (csrc/sample_scores.hip)   no counterpart in the reference
 *   X: the samples (N rows), Y: the manifold set (M rows), r_y: device float[M], the k-NN radius of row j of Y (what
 *   am_knn_radii_f32(Y, Y) returns).  One Gram pass on the exact f32 tile engine, no N x M matrix.  Per pair, all in f32:
 *     d2      = max(fmaf(-2, <x_i, y_j>, |x_i|^2 + |y_j|^2), 0), NaN -> +inf: the bits of am_knn_search_f32(squared) and of
 *               the exact PRDC kernel (same row norms, same inner order)
 *     radius  one that is not > 0 (zero, negative, NaN) counts as 0: nobody's ball, ratio 0
 *     member  d2 < T(r_j)  <=>  sqrt_rn(d2) < r_j, the strict test of am_prdc_counts_f32
 *     ratio   q = fdiv_rn(fmul_rn(r_j, r_j), d2), correctly rounded; NaN (0 / 0, inf / inf) counts as 0; d2 == 0 with
 *             r_j > 0 gives +inf
 *   Outputs per row i of X, all overwritten:
 *     out_realism[i]     = sqrt_rn(max_j q)        (Kynkaanniemi et al. 2019: max_j r_j / |x_i - y_j|; >= 1: in some ball)
 *     out_realism_idx[i] = the j that attains it, ties to the SMALLEST j; -1 where the maximum is 0 (no row of Y with a
 *                          positive radius at a finite distance: a non-finite sample row, all radii 0)
 *     out_count[i]       = #{ j : member } - the bits of out_col_count of am_prdc_counts_f32(R = Y, C = X, r_ref = r_y, ..)
 *     out_rarity[i]      = min { r_j : member }   (Han et al. 2023), out_rarity_idx[i] = the j that attains it, ties to the
 *                          smallest j; 0.0f and -1 for a row outside every ball
 *   No floating-point atomics: two calls return the same bits, whatever the chunking.  X may be Y (nothing is skipped:
 *   every row then has realism +inf).  M < 2^32 - 1; X, Y as for am_knn_search_f32 (16-byte aligned, ld % 4 == 0,
 *   ld >= D).  Workspace: the row norms, two floats per column and [am_sample_scores_chunks][N] (uint64, uint64, int32)
 *   partials.  Everything is validated before the first HIP call; the call is asynchronous.
 * ------------------------------------------------------------------------- */
size_t am_sample_scores_workspace_bytes(int64_t N, int64_t M, int D);
int am_sample_scores_chunks(int64_t N, int64_t M, int D);      /* column chunks the plan uses (tests, tools) */
int am_sample_scores_f32(const float* X, int64_t N, int64_t ldx, const float* Y, int64_t M, int64_t ldy, int D,
                         const float* r_y, float* out_realism, int64_t* out_realism_idx, int32_t* out_count,
                         float* out_rarity, int64_t* out_rarity_idx,
                         void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * PER-SAMPLE realism, ball count and rarity that LEAVE A GROUP OUT (csrc/sample_scores.hip)   no counterpart in the reference
 *   am_sample_scores_f32 with one int32 label per row of X and per row of Y (the song a window was cut from).  A pair
 *   (i, j) with x_group[i] == y_group[j] is NO PAIR, for any int32 values (labels are moved and compared for equality,
 *   never computed with): it is not counted, its ratio is 0, it is no candidate of the rarity.
 *     out_realism[i]     = sqrt_rn(max { q_ij : y_group[j] != x_group[i] }), out_realism_idx[i] the j that attains it, ties to
 *                          the SMALLEST j; 0.0f and -1 where the maximum is 0 (a non-finite sample row, no admissible row of
 *                          Y with a positive radius at a finite distance, every row of Y in the row's own group)
 *     out_count[i]       = #{ j : y_group[j] != x_group[i], member }
 *     out_rarity[i]      = min { r_j : y_group[j] != x_group[i], member }, out_rarity_idx[i] the j that attains it, ties to
 *                          the smallest j; 0.0f and -1 for a row outside every admissible ball
 *   Everything else is am_sample_scores_f32, to the bit: d2, the cleaned radii, the strict membership test, the correctly
 *   rounded ratio and its square root, the order of ties, the chunk plan (am_sample_scores_chunks), the partials and the
 *   merge kernel.  With label values that no row of the other set carries the five outputs ARE those of
 *   am_sample_scores_f32; with one value on every row of both sets every row gets (0, -1, 0, 0, -1).  X may be Y with
 *   x_group == y_group: every row is then scored against the rows of the OTHER groups, itself excluded through its own.
 *   No floating-point atomics: two calls return the same bits, whatever the chunking.
 *   x_group, y_group: device pointers, N and M values; null -> AM_ERR_BAD_ARG.  M < 2^32 - 1; X, Y as for
 *   am_knn_search_f32 (16-byte aligned, ld % 4 == 0, ld >= D).  Workspace (caller-owned; the library allocates nothing):
 *   that of am_sample_scores_f32.  Everything is validated before the first HIP call; the call is asynchronous.
 * ------------------------------------------------------------------------- */
size_t am_sample_scores_groups_workspace_bytes(int64_t N, int64_t M, int D);
int am_sample_scores_groups_f32(const float* X, int64_t N, int64_t ldx, const int32_t* x_group,
                                const float* Y, int64_t M, int64_t ldy, const int32_t* y_group, int D,
                                const float* r_y, float* out_realism, int64_t* out_realism_idx, int32_t* out_count,
                                float* out_rarity, int64_t* out_rarity_idx,
                                void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * PROBABILISTIC scoring rule of a point against a set (csrc/psr.hip)                  no counterpart in the reference
 *   The per-row quantity of probabilistic precision and recall (Park & Kim, ICCV 2023).  X: the points (N rows), Y: the
 *   set (M rows), radius: ONE radius for the whole set Y, a HOST double.  One Gram pass on the exact f32 tile engine, no
 *   N x M matrix.  Per pair:
 *     d2       = max(fmaf(-2, <x_i, y_j>, |x_i|^2 + |y_j|^2), 0), NaN -> +inf: the bits of am_knn_search_f32(squared)
 *                (same row norms, same inner order)
 *     in range   d2 < T, T the smallest float32 >= radius * radius (the product in f64)  <=>  (double)d2 < radius * radius;
 *                NaN and +inf are never in range
 *     factor     fminf(fmul_rn(sqrt_rn(d2), (float)(1.0 / radius)), 1.0f) for a pair in range, in f32
 *   Outputs per row i of X, all overwritten:
 *     out_count[i] = #{ j : in range }
 *     out_psr[i]   = 1.0 - prod_{j in range} factor, in f64: exactly 0.0 with no column in range, exactly 1.0 when some
 *                    in-range d2 is 0.  Products of at most 16 factors (one lane's share of a 32 x 32 accumulator sub-tile)
 *                    are formed in f32 - one that underflows to 0 moves psr by less than 1e-37 - everything beyond is an
 *                    f64 running product joined in a fixed order (lane slot order, then chunk order)
 *     out_sums     DEVICE double[2], may be NULL: { sum_i out_psr[i], sum_i out_count[i] }, f64 sums in a fixed tree; the
 *                  second is an exact integer
 *   No floating-point atomics: two calls at the same shapes return the same bits.  Unlike the key-based entry points
 *   (search, assign, sample scores) the LAST BITS of out_psr DEPEND ON THE CHUNK PLAN (am_psr_chunks, a function of N and
 *   M): an f64 product is grouped by chunk.  out_count does not.  X may be Y (nothing is skipped: every finite row then
 *   has psr 1.0).  radius must be finite and > 0 with radius^2 <= FLT_MAX (else AM_ERR_BAD_ARG); the shape rules are those
 *   of am_sample_scores_f32 (M < 2^32 - 1; 16-byte aligned, ld % 4 == 0, ld >= D).  Workspace: the row norms,
 *   [am_psr_chunks][N] (double, int32) partials and the block sums.  Everything is validated before the first HIP call;
 *   the call is asynchronous.
 * ------------------------------------------------------------------------- */
size_t am_psr_workspace_bytes(int64_t N, int64_t M, int D);
int am_psr_chunks(int64_t N, int64_t M, int D);                /* column chunks of the plan (tests, tools) */
int am_psr_f32(const float* X, int64_t N, int64_t ldx, const float* Y, int64_t M, int64_t ldy, int D,
               double radius, double* out_psr, int32_t* out_count, double* out_sums,
               void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * RETRIEVAL RANKS of paired sets (csrc/retrieval.hip)                                no counterpart in the reference
 *   At which rank does query row i find its own gallery rows among all M?  Q: the queries (N rows), G: the gallery (M
 *   rows); the POSITIVES of row i are the columns pos_columns[pos_start[i] .. pos_start[i] + pos_count[i]) - int64 device
 *   arrays, distinct columns inside a segment, rows with one label may share a segment.  One Gram pass on the exact f32
 *   tile engine, no N x M matrix.  Per pair:
 *     u_ij = fmul_rn(a_ij, w_j),  a_ij = <q_i, g_j> with the bits of the tile engine (the fmaf chain of am_knn_search_f32),
 *            w_j = 1 (cosine == 0) or fdiv_rn(1, sqrt_rn(|g_j|^2)) (cosine != 0; the f32 norms of the search).  The query's
 *            own norm changes no order inside its row and is not applied.  A pair whose u is NaN HAS NO SCORE (a zero-norm
 *            gallery row under cosine, a row with a non-finite element): it is never a positive and never counted
 *   Outputs per row i of Q, all overwritten:
 *     out_positive[i]  the smallest positive column that reaches t_i = max { u_ij : j in P_i, scored }; -1 for an UNRANKED
 *                      row: one with no scored positive, with an entry of its segment outside [0, M) or with a segment
 *                      that leaves pos_columns (nothing out of range is dereferenced)
 *     out_better[i]    #{ negatives j : u_ij >  t_i }, out_tied[i] = #{ negatives j : u_ij == t_i } as IEEE float compares;
 *                      the NEGATIVES are the columns not in P_i and, with group ids, those with g_group[j] != q_group[i];
 *                      -1, -1 for an unranked row.  rank = 1 + out_better is the optimistic convention
 *     out_score[i]     t_i (dot), fmul_rn(t_i, w_i^Q) with the query's own weight (cosine: the cosine itself); NaN unranked
 *     out_n_pos[i]     the entries of the row's segment inside [0, M); out_n_pos_own_group[i] those of them with
 *                      g_group[j] == q_group[i] (0 without group ids)
 *   q_group, g_group: int32 device vectors, BOTH null (every column that is no positive is a negative) or both set; exactly
 *   one null -> AM_ERR_BAD_ARG.  A positive inside the row's own group is still a positive.  No atomics: two calls return
 *   the same bits, whatever the chunk plan (am_retrieval_chunks) and the order of a segment's entries.  M < 2^31 (the
 *   counts are int32); Q, G as for am_knn_search_f32 (16-byte aligned, ld % 4 == 0, ld >= D); Q may be G.  Workspace: the
 *   norms and weights of both sides, t_i, and [am_retrieval_chunks][N] int32 x 2 partials; the query returns 0 for a shape
 *   the call refuses.  Everything is validated before the first HIP call; the call is asynchronous.
 * ------------------------------------------------------------------------- */
size_t am_retrieval_workspace_bytes(int64_t N, int64_t M, int D);
int am_retrieval_chunks(int64_t N, int64_t M, int D);          /* column chunks of the plan (tests, tools) */
int am_retrieval_ranks_f32(const float* Q, int64_t N, int64_t ldq, const float* G, int64_t M, int64_t ldg, int D, int cosine,
                           const int64_t* pos_start, const int64_t* pos_count, const int64_t* pos_columns,
                           int64_t n_pos_columns, const int32_t* q_group, const int32_t* g_group,
                           int32_t* out_better, int32_t* out_tied, float* out_score, int64_t* out_positive,
                           int32_t* out_n_pos, int32_t* out_n_pos_own_group,
                           void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * SLICED WASSERSTEIN distance, its three device steps (csrc/swd.hip)                 no counterpart in the reference
 *   Every pointer below is a DEVICE pointer.  Everything is validated before the first HIP call; the calls are
 *   asynchronous.  No floating-point atomics: two calls return the same bits.
 *
 *   PROJECT.  Z[l * ldz + i] = <Theta_l, x_i> for the N rows of X and the L rows of Theta, in f32 on the exact f32 tile
 *   engine: the fmaf chain over the inner index in the engine's order (that of am_knn_search_f32's dot products), which
 *   does not depend on the tile position - a projection has the same bits alone and among any other directions.  X, Theta
 *   as for am_knn_search_f32 (16-byte aligned, ld % 4 == 0, ld >= D); ldz >= N, no alignment.  Elements of Z outside
 *   [L][N] are not written.  No workspace.
 *
 *   SORT.  Every one of L rows of N floats (row stride ld_in) ascending into `out` (row stride ld_out), keys only.  An LSD
 *   radix sort over u = b ^ (b >> 31 ? 0xffffffff : 0x80000000) of the bits b, 8 bits per pass, stable between passes; one
 *   workgroup owns a row.  -0.0 sorts before +0.0; every NaN (either sign, any payload) comes last, behind +inf, and is
 *   written as the quiet NaN 0x7fc00000; every other value keeps its bits.  out may be in (same pointer and stride);
 *   elements between N and the row stride are neither read nor written.  1 <= N <= 2^31 - 1.  Workspace: one [L][N
 *   rounded up to 4] float matrix.
 *
 *   W.  out[l] = W_p^p between the uniform empirical measures on row l of Zx (n atoms) and row l of Zy (m atoms), both
 *   SORTED ascending (am_sort_rows_f32), p = 1 or 2, in f64: the quantile coupling on the merged grid {i / n} u {j / m},
 *     out[l] = (1 / (n m)) sum over overlapping (i, j) of (min((i + 1) m, (j + 1) n) - max(i m, j n)) |x_(i) - y_(j)|^p
 *   with integer weights (exact: n m < 2^53, else AM_ERR_BAD_SHAPE), one thread per atom of the larger side, f64 block sums
 *   joined in a fixed tree.  The operands are ordered by (size, then argument order): (Zx, Zy) and (Zy, Zx) return the same
 *   bits, a matrix against itself exactly 0.0.  nonfinite[l] (int32) = the number of NaNs and infinities in the two rows;
 *   where it is not 0, out[l] is NaN.  Workspace: one (double, int) pair per 256 atoms of the larger side and row.
 * ------------------------------------------------------------------------- */
int am_sliced_project_f32(const float* X, int64_t N, int64_t ldx, const float* Theta, int64_t L, int64_t ldt, int D,
                          float* Z, int64_t ldz, am_stream_t stream);
size_t am_sort_rows_workspace_bytes(int64_t L, int64_t N);
int am_sort_rows_f32(const float* in, int64_t L, int64_t N, int64_t ld_in, float* out, int64_t ld_out,
                     void* ws, size_t ws_bytes, am_stream_t stream);
size_t am_sliced_w_workspace_bytes(int64_t L, int64_t n, int64_t m);
int am_sliced_w_f32(const float* Zx, int64_t n, int64_t ldzx, const float* Zy, int64_t m, int64_t ldzy, int64_t L, int p,
                    double* out, int32_t* nonfinite, void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * RANDOM FOURIER FEATURES of the Gaussian kernel and their moment matrix (csrc/rff.hip)   no counterpart in the reference
 *   FKEA (Ospanov, Zhang, Jalali, Cao, Bogdanov, Farnia, NeurIPS 2024): the spectrum of K / n, K_ij = exp(-|x_i - x_j|^2 /
 *   (2 bw^2)), at any number of rows from a [2R][2R] matrix.  Every pointer below is a DEVICE pointer.  Everything is
 *   validated before the first HIP call; the calls are asynchronous.  No floating-point atomics: two calls return the same
 *   bits.
 *
 *   W [R][D] float32: the frequencies, a UNIT-bandwidth standard normal draw (the package draws
 *     numpy.random.default_rng(seed).standard_normal((R, D)) rounded to float32 once), independent of the bandwidth.
 *   z_il = <w_l, x_i> in f32 on the exact f32 tile engine (the fmaf chain of am_sliced_project_f32: the bits do not depend on
 *     the tile position).  a_il = (double) z_il * inv_bw with inv_bw = 1 / bw in f64: the host double `inv_bw` (finite, > 0),
 *     or, with bw2_dev != NULL (a float32 DEVICE scalar holding a median squared distance, the output of
 *     am_pairwise_select_f32), 1 / sqrt((double) *bw2_dev) formed on the device - no host round trip.
 *   phi_i = R^(-1/2) [cos a_i1 .. cos a_iR, sin a_i1 .. sin a_iR], cos and sin in f64 (|error| < 2^-53; an argument of
 *     magnitude >= 2^30 - whose float32 projection has no phase left - gives NaN).  <phi_i, phi_j> is an unbiased estimate
 *     of K_ij and |phi_i|^2 = 1.
 *   S = (1 / n) sum_i phi_i phi_i^T, [2R][2R] f64, trace 1: its non-zero eigenvalues are those of Phi Phi^T / n, which
 *     approximates K / n with a Monte-Carlo error of order 1 / sqrt(R).
 *
 *   FEATURES.  F[l * ldo + i] = cos(a)/sqrt(R) and F[(R + l) * ldo + i] = sin(a)/sqrt(R) for the rows row0 + i, 0 <= i <
 *   nrows, of X: feature-major, ldo >= nrows.  A feature has the same bits alone and among any other frequencies, and for
 *   every (row0, nrows) that covers its row.  Elements with i >= nrows are not written.  A row with a NaN or an infinity
 *   writes zeros and is counted: `ws` opens with ONE int64, the number of such rows in [row0, row0 + nrows).  X, W as for
 *   am_sliced_project_f32 (16-byte aligned, ld % 4 == 0, ld >= D); 1 <= R <= am_rff_max_features() = 1024.
 *
 *   MOMENT.  out_s [2R][2R] = S over all N rows.  The rows are cut into am_rff_moment_chunks(N, R) chunks of 4096; per chunk
 *   the features go to the workspace and their Gram runs on v_mfma_f64_16x16x4_f64 over the upper 64 x 64 tiles, the chunk's
 *   rows split among workgroups whose partial tiles are added in split order, chunk after chunk in stream order; the last
 *   fold divides by N and writes the mirror, so S is exactly symmetric.  `ws` opens with the same int64 count, over all N
 *   rows (their features are zeros and the divisor stays N: N S is the sum over the finite rows).  The workspace holds one
 *   chunk - it does not grow with N past 4096 rows.
 * ------------------------------------------------------------------------- */
int am_rff_max_features(void);
size_t am_rff_features_workspace_bytes(int64_t nrows);
int am_rff_features_f32(const float* X, int64_t N, int64_t ldx, int D, const float* W, int R, int64_t ldw,
                        int64_t row0, int64_t nrows, double inv_bw, const float* bw2_dev,
                        double* F, int64_t ldo, void* ws, size_t ws_bytes, am_stream_t stream);
int am_rff_moment_chunks(int64_t n, int R);
size_t am_rff_moment_workspace_bytes(int64_t n, int D, int R);
int am_rff_moment_f32(const float* X, int64_t N, int64_t ldx, int D, const float* W, int R, int64_t ldw,
                      double inv_bw, const float* bw2_dev, double* out_s, void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * CLASSIFIER-OUTPUT scores: row-wise on logits (csrc/class_scores.hip)               no counterpart in the reference
 *   Every pointer below is a DEVICE pointer except `offsets`.  Everything is validated before the first HIP call; the
 *   calls are asynchronous.  All arithmetic is f64: float32 rows are converted on load (exact), so the _f32 and _f64
 *   entry points return the SAME BITS on the same values.  No floating-point atomics; every sum runs in an order that
 *   depends on the shapes and the group sizes only: two calls return the same bits.
 *
 *   Row quantities of a row l of C logits: M = max l_c, e_c = exp(l_c - M), S = sum e_c, U = sum e_c (l_c - M),
 *   p_c = e_c / S, h = sum p_c log p_c = U / S - log S.  A logit of -inf is a masked class (p_c = 0, no term in U).  A
 *   row with a NaN, a +inf, or nothing but -inf is NON-FINITE: its h is NaN and it is counted.
 *
 *   CLASS GROUPS.  Group b = the rows L[idx[offsets[b] + j]] (the group list of am_stats_gather_*; idx == NULL: the rows
 *   in stored order; offsets: HOST, B + 1 entries from 0, every group >= 1 rows of any number).  With n_b rows,
 *     pbar_c = (1 / n_b) sum_i p_ic,   m_b = sum_c pbar_c log pbar_c (0 log 0 = 0),   log IS_b = (1 / n_b) sum_i h_i - m_b
 *   out_rec[b] = { (1 / n_b) sum h, m_b, log IS_b, non-finite rows of the group } (4 doubles; the first three NaN where
 *   the fourth is not 0); out_h (may be NULL) [offsets[B]]: h per list position.  The list positions of a group are cut
 *   into segments of 64 (a segment never crosses a group), one workgroup per segment, a wave per row, the rows of a wave
 *   in ascending order, the four waves' column sums added in wave order, a group's segments in ascending order, m_b in a
 *   fixed tree: the bits of a group depend on its rows and their list order alone - not on idx being NULL or not, not on
 *   the other groups.  The workspace opens with the flag word of the group-list protocol (1 + the list position of an
 *   index outside [0, N), or 0; such an index is never dereferenced and its row counts as non-finite).
 *   Limits: 1 <= C <= 2048 (the column sums of a workgroup stay in LDS), N, B >= 1, else AM_ERR_BAD_SHAPE; L as for
 *   am_stats_gather_* (float32: 16-byte aligned, ld % 4 == 0, N * ld < 2^30; ld >= C), else AM_ERR_BAD_ARG / _BAD_SHAPE.
 *
 *   ROW PAIRS.  One value v_i per row i of two [N, C] matrices (cand, ref) with their own leading dimensions:
 *     AM_PAIR_COSINE        <a, b> / sqrt(|a|^2 |b|^2); a zero norm gives NaN
 *     AM_PAIR_KL_SOFTMAX    sum_c p^r_c (log p^r_c - log(p^c_c + eps)), p = softmax of the row; at eps == 0 evaluated as
 *                           sum_c p^r_c ((r_c - lse_r) - (c_c - lse_c)); terms with p^r_c = 0 are 0; a non-finite row on
 *                           either side gives NaN
 *     AM_PAIR_KL_SIGMOID    sum_c s(r_c) (log s(r_c) - log(s(c_c) + eps)), s the logistic function (one-term form: not a
 *                           divergence, may be negative)
 *     AM_PAIR_KL_BERNOULLI  sum_c [ s log(s / (t + eps)) + (1 - s) log((1 - s) / (1 - t + eps)) ], s = s(r_c), t = s(c_c)
 *   (at eps == 0 the sigmoid forms use log s(x) = min(x, 0) - log1p(exp(-|x|)), log(1 - s(x)) = log s(-x)).
 *   rows_out (may be NULL) [N] = v; sums[4] = { sum v, sum v^2, finite rows, non-finite rows }, a value that is not
 *   finite being counted and left out of the two sums.  One wave per pair, a workgroup the rows [64 g, 64 g + 64): its
 *   four sums by an xor butterfly over the 64 values, the workgroups' partials thread-strided (w = t, t + 256, ...), an xor
 *   butterfly per wave, then (wave 0 + wave 1) + (wave 2 + wave 3).
 *   Limits: N >= 1, 1 <= C <= 8192, else AM_ERR_BAD_SHAPE; ld >= C, float32 rows 16-byte aligned with ld % 4 == 0, a
 *   known mode, eps finite and >= 0, else AM_ERR_BAD_ARG.
 * ------------------------------------------------------------------------- */
enum am_pair_mode { AM_PAIR_COSINE = 0, AM_PAIR_KL_SOFTMAX = 1, AM_PAIR_KL_SIGMOID = 2, AM_PAIR_KL_BERNOULLI = 3 };
size_t am_class_groups_workspace_bytes(int64_t n_total, int B, int C);
int am_class_groups_f32(const float* L, int64_t N, int64_t ld, int C, const int64_t* idx, const int64_t* offsets, int B,
                        double* out_rec, double* out_h, void* ws, size_t ws_bytes, am_stream_t stream);
int am_class_groups_f64(const double* L, int64_t N, int64_t ld, int C, const int64_t* idx, const int64_t* offsets, int B,
                        double* out_rec, double* out_h, void* ws, size_t ws_bytes, am_stream_t stream);
size_t am_row_pairs_workspace_bytes(int64_t N);
int am_row_pairs_f32(const float* cand, int64_t ldc, const float* ref, int64_t ldr, int64_t N, int C, int mode, double eps,
                     double* rows_out, double* sums, void* ws, size_t ws_bytes, am_stream_t stream);
int am_row_pairs_f64(const double* cand, int64_t ldc, const double* ref, int64_t ldr, int64_t N, int C, int mode, double eps,
                     double* rows_out, double* sums, void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * A9, partitioned form for one-process-per-GPU callers that all hold the FULL set X.
 * The self-distance matrix is bitwise symmetric, so only half of the tile pairs are multiplied
 * (csrc/pairwise.hip, knn_sym_kernel); rank `part` of `nparts` owns a contiguous range of the 128-row blocks.
 *   am_knn_sym_eligible     1 if this path applies to the shape (else use am_knn_radii_f32 on row shards)
 *   am_knn_bounds_f32       upper bounds (SQUARED distances) of the final values of rows [row0, row0+nrows)
 *                           from a column sample; ranks split the rows and all-gather the result
 *   am_knn_sym_part_f32     this rank's share: out_lists[N][am_knn_list_width(k)] = its smallest entries per row
 *                           (+inf padded; a NaN in slot 0 flags a row whose candidate buffer overflowed);
 *                           bounds_sq[N] is read (the exact form also tightens it in place)
 *   am_knn_lists_finish_f32 lists[nparts][N][width] (all-gathered) -> out_r[N]; flagged rows are recomputed exactly
 *                           (workspace: am_knn_lists_finish_workspace_bytes)
 * Shapes that take the f16 filter + exact verification form in am_knn_radii_f32 take it here too (csrc/pairwise_fast.h):
 * the bounds come from an f16 sample pass, each rank sweeps its row blocks on the f16 copy and evaluates its surviving
 * pairs exactly; out_lists then holds the rank's smallest EXACT values per row.
 * The result is bit-identical to am_knn_radii_f32(X, X).
 * ------------------------------------------------------------------------- */
int am_knn_sym_eligible(int64_t N, int D, int k);
int am_knn_list_width(int k);
size_t am_knn_part_workspace_bytes(int64_t N, int D, int k);
int am_knn_bounds_f32(const float* X, int64_t N, int64_t ld, int D, int k, int64_t row0, int64_t nrows,
                      float* out_bound_sq, void* ws, size_t ws_bytes, am_stream_t stream);
int am_knn_sym_part_f32(const float* X, int64_t N, int64_t ld, int D, int k, int part, int nparts,
                        float* bounds_sq, float* out_lists, void* ws, size_t ws_bytes, am_stream_t stream);
size_t am_knn_lists_finish_workspace_bytes(int64_t N, int D, int k);
int am_knn_lists_finish_f32(const float* lists, int nparts, const float* X, int64_t N, int64_t ld, int D, int k,
                            float* out_r, void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * Prepared sets.  Every PRDC entry point first derives from each set its squared row norms, their maximum, the largest
 * |element| and - for the f16 filter forms - a scaled f16 copy (0.14 ms per 100k x 512 set and call).  An evaluate() calls
 * three to four entry points per set (more per rank in the partitioned multi-GPU form): am_prepare_set_f32 computes the
 * three pieces ONCE into caller-owned device buffers
 *     norms  float[N]                     squared row norms (the summation order of the k-NN kernels)
 *     stats4 uint32[4]                    { largest squared norm, 0, largest |element|, 0 } as f32 bit patterns
 *     half   uint16[N * am_prepared_half_ld(D)]   f16 copy scaled by an exact power of two, rows zero-padded
 * and the *_prepared_* variants below take them instead of recomputing (same results, bit for bit).  A ROW SHARD of a
 * prepared set is the same struct with `norms` and `half` advanced to the shard's first row (the statistics of the
 * whole set remain valid bounds for the shard).  The struct is a HOST struct of DEVICE pointers.
 * ------------------------------------------------------------------------- */
typedef struct am_prepared_set {
    const float* norms;
    const uint32_t* stats;
    const uint16_t* half;
} am_prepared_set;
int64_t am_prepared_half_ld(int D);
int am_prepare_set_f32(const float* X, int64_t N, int64_t ld, int D, float* norms, uint32_t* stats4, uint16_t* half,
                       am_stream_t stream);
int am_knn_radii_prepared_f32(const float* X, int64_t N, int64_t ldx, int D, const am_prepared_set* prepared, int k,
                              float* out_r, void* ws, size_t ws_bytes, am_stream_t stream);          /* Y == X */
int am_knn_bounds_prepared_f32(const float* X, int64_t N, int64_t ld, int D, const am_prepared_set* prepared, int k,
                               int64_t row0, int64_t nrows, float* out_bound_sq, void* ws, size_t ws_bytes, am_stream_t stream);
int am_knn_sym_part_prepared_f32(const float* X, int64_t N, int64_t ld, int D, const am_prepared_set* prepared, int k,
                                 int part, int nparts, float* bounds_sq, float* out_lists, void* ws, size_t ws_bytes,
                                 am_stream_t stream);
int am_prdc_counts_prepared_f32(const float* R, int64_t Nr, int64_t ldr, const am_prepared_set* prepared_r,
                                const float* C, int64_t Nc, int64_t ldc, const am_prepared_set* prepared_c, int D,
                                const float* r_ref, const float* r_cand,
                                int32_t* out_col_count, uint8_t* out_row_any, uint8_t* out_row_cover, float* out_row_min,
                                void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * A10  hypersphere membership counts            reference: prdc.py:34-48
 *   With d(i,j) the distance between reference row i and candidate row j:
 *   out_col_count[j] = #{ i : d(i,j) < r_ref[i] }             (precision, density)
 *   out_row_any[i]   = any_j d(i,j) < r_cand[j]               (recall)
 *   out_row_cover[i] = any_j d(i,j) < r_ref[i]                (coverage: min_j d(i,j) < r_ref[i], prdc.py:45-47)
 *   out_row_min[i]   = min_j d(i,j)                           OPTIONAL (may be NULL): not needed by any metric
 *   Outputs are OVERWRITTEN.  am_prdc_reduce turns the first three into the four integer totals
 *   { #cols with count>0, #rows with any, sum of counts, #rows covered } (device int64[4]); the caller
 *   divides in f64.
 *   Large problems (Nr * Nc >= 2^24 pairs for D >= 256, 2^26 for 128 <= D < 256, 1e8 for 32 <= D < 128, 2^28 below; D <= 4096) run as a
 *   scaled-f16 MFMA FILTER pass that queues every pair whose membership its error bound
 *   cannot decide, followed by an f32 evaluation of exactly those pairs with the arithmetic of the exact
 *   kernel (csrc/pairwise_fast.h): the outputs are bit-identical to the exact kernel's, which remains the
 *   path for small problems and the automatic fallback.  Asking for out_row_min adds the candidates of the
 *   row minimum to the queue (slower).
 * ------------------------------------------------------------------------- */
size_t am_prdc_workspace_bytes(int64_t Nr, int64_t Nc, int D);
int am_prdc_counts_f32(const float* R, int64_t Nr, int64_t ldr,
                       const float* C, int64_t Nc, int64_t ldc, int D,
                       const float* r_ref, const float* r_cand,
                       int32_t* out_col_count, uint8_t* out_row_any, uint8_t* out_row_cover, float* out_row_min,
                       void* ws, size_t ws_bytes, am_stream_t stream);
int am_prdc_reduce(const int32_t* col_count, int64_t Nc,
                   const uint8_t* row_any, const uint8_t* row_cover, int64_t Nr,
                   int64_t* out4, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * float64 rows: A6-A10 in the dtype of the embeddings.
 *   The reference computes every stage in the dtype of the rows it is given - torch.cdist / kthvalue (prdc.py:12-13,34),
 *   the comparisons against the radii (prdc.py:36-47), np.matmul and the kernel sums (kd.py:112-116, 56-81) - and float64
 *   rows are what its PCA projection hands on (projection.py:20-21: scikit-learn's float64 product; audio_metrics.py:163-182,
 *   the path of every reference test and of examples/2_musdb.py) and what its test embedder yields.  These entry points are
 *   the f64 forms of am_knn_radii_f32 / am_prdc_counts_f32 / am_kd_poly_f32 / am_kd_rbf_f32: same arguments with double
 *   rows, double radii and a double row minimum, every product and sum in f64 on the f64 matrix cores
 *   (v_mfma_f64_16x16x4_f64, csrc/pairwise_f64.hip):  d2 = max(fma(-2, <x, y>, |x|^2 + |y|^2), 0), radius = sqrt_rn of the
 *   (k+1)-th smallest d2, membership  sqrt_rn(d2) < r  decided exactly through d2 < T(r).  Rows need no alignment
 *   (ld >= D, in elements).  Any 1 <= k < M (k > 31: distance blocks + a radix select, a correctness path).
 *   Large problems - am_knn_radii_f64 of a set against itself (Y == X, k <= 10) and am_prdc_counts_f64 without a row minimum,
 *   from the row counts at which the float32 entry points switch to their f16 filter form - take that filter too: the sweep
 *   runs on a float32-rounded copy inside the workspace with an error band widened by the rounding, and every pair the band
 *   cannot decide is evaluated in f64 as a sum of squared differences against the f64 thresholds (csrc/pairwise_fast.h:
 *   knn_fast_select64_kernel, cross_verify_regions64_kernel).  Same results as the general kernels to rounding (counts equal;
 *   the sum of squared differences is the more accurate form on near-duplicate rows), about a tenth of their time at 100 000
 *   rows; data the filter cannot serve runs the general kernels, launched behind a device flag.  The workspace queries cover
 *   the route; with a smaller workspace the general kernels run.
 * ------------------------------------------------------------------------- */
size_t am_knn_f64_workspace_bytes(int64_t N, int64_t M, int D, int k);
int am_knn_radii_f64(const double* X, int64_t N, int64_t ldx,
                     const double* Y, int64_t M, int64_t ldy, int D, int k,
                     double* out_r, void* ws, size_t ws_bytes, am_stream_t stream);
size_t am_prdc_f64_workspace_bytes(int64_t Nr, int64_t Nc, int D);
int am_prdc_counts_f64(const double* R, int64_t Nr, int64_t ldr,
                       const double* C, int64_t Nc, int64_t ldc, int D,
                       const double* r_ref, const double* r_cand,
                       int32_t* out_col_count, uint8_t* out_row_any, uint8_t* out_row_cover, double* out_row_min,
                       void* ws, size_t ws_bytes, am_stream_t stream);
size_t am_kd_f64_workspace_bytes(int S, int m);
int am_kd_poly_f64(const double* X, int64_t N1, int64_t ldx,
                   const double* Y, int64_t N2, int64_t ldy, int D,
                   const int64_t* idx1, const int64_t* idx2, int S, int m,
                   double gamma, double coef0, int degree,
                   double* out_mmd, void* ws, size_t ws_bytes, am_stream_t stream);
int am_kd_rbf_f64(const double* X, int64_t N1, int64_t ldx,
                  const double* Y, int64_t N2, int64_t ldy, int D,
                  const int64_t* idx1, const int64_t* idx2, int S, int m, double sigma,
                  double* out_mmd, void* ws, size_t ws_bytes, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * N1  PCA projection support                   reference: projection.py:6-46 (scikit-learn IncrementalPCA),
 *                                                           audio_metrics.py:163-209
 *   am_eigh_sym_f64  eigen-decomposition of a symmetric POSITIVE SEMI-DEFINITE D x D matrix (the Gram matrix of the
 *                    stacked, centred batch whose SVD scikit-learn takes): evals[D] in DESCENDING order, evecs[D][D]
 *                    with row i = eigenvector i (unit norm; sign not normalised - the caller applies scikit-learn's
 *                    svd_flip).  One-sided block Jacobi in f64; SYNCHRONISES `stream` once per BLOCK of enqueued
 *                    sweeps (12, then 6 at a time: normally once per solve - the kernels of a sweep return at once when
 *                    the sweep before it applied no rotation; fitting happens once per reference set, not per evaluate).  AM_ERR_NO_CONVERGENCE after max_sweeps (<= 0: 40).
 *                    Same input, same bits.  Scale: A is brought to unit scale by the power of two of its trace before the
 *                    first sweep and the eigenvalues are scaled back at the end (both exact), so the result is the
 *                    same at every scale - evals(2^e A) = 2^e evals(A), evecs equal - for any A whose trace is a finite
 *                    normal number: largest eigenvalue from 2^-1022 up to trace A < 2^1024.  Entries that fall below
 *                    2^-1074 trace A are flushed to zero by the scaling (they are below the rounding of the result).
 *                    Non-finite input: a NaN or an infinity anywhere in A, or a trace that overflows, returns
 *                    AM_ERR_NO_CONVERGENCE - the status am_frechet_f64 gives a non-finite product - after one
 *                    synchronisation; no sweep runs and evals / evecs are NOT written.
 *   am_project_f64   out[N][p] (f64) = (X[n][:] - mean[:]) . components[j][:]  - IncrementalPCA.transform - on the f64
 *                    matrix cores; X is the N x D f32 embedding matrix (am_project_rows_f64: f64), mean f64[D], components f64[p][D].
 * ------------------------------------------------------------------------- */
size_t am_eigh_workspace_bytes(int D);
int am_eigh_sym_f64(const double* A, int D, double* evals, double* evecs, int max_sweeps,
                    void* ws, size_t ws_bytes, am_stream_t stream);
int am_project_f64(const float* X, int64_t N, int64_t ld, int D, const double* mean, const double* components, int p,
                   double* out, am_stream_t stream);
/* the same for float64 rows (a float64 embedder in front of the projection: scikit-learn then multiplies in f64 too) */
int am_project_rows_f64(const double* X, int64_t N, int64_t ld, int D, const double* mean, const double* components, int p,
                        double* out, am_stream_t stream);

/* ---------------------------------------------------------------------------
 * A13  one call = one evaluate()                reference: audio_metrics.py:254-274
 *   The FAD + KD + PRDC dispatch of AudioMetrics.evaluate for two embedding sets on ONE device as a single stream-ordered
 *   chain of the entry points above (statistics, Frechet solve on `side_stream` under the PRDC kernels, prepared sets,
 *   radii of both sets, membership counts and totals, kernel distance on the caller's index tables), with every workspace
 *   carved from one caller buffer and every result in ONE device buffer `out`:
 *     out[0..4]   fd, tr sqrt, iterations, residual, Frechet stop code (0: the product needs more than the 32 iterations
 *                 enqueued here - finish with am_frechet_f64 on the statistics; 4: non-finite; -1: FAD not requested)
 *     out[5..8]   #candidate columns with count > 0, #reference rows with a witness, sum of counts, #reference rows covered
 *                 (precision = out[5] / n_cand, recall = out[6] / n_ref, density = out[7] / (k n_cand), coverage = out[8] / n_ref)
 *     out[16 + s] unbiased MMD^2 of subset s (kernel_distance_mean / _std are numpy's mean / std of these, kd.py:189-192)
 *   `what` selects the metrics.  am_evaluate_side (optional, per set) hands in results the caller already holds - the
 *   reference keeps the reference set's statistics and radii between evaluates (data.py:60-66) - and/or names where the
 *   statistics / radii computed here are to be written so that the caller can keep them; NULL members are ignored.
 *   idx_cand / idx_ref: int64 [kd_subsets, kd_m] DEVICE tables (am_kd_draw_indices draws them on the host).
 * ------------------------------------------------------------------------- */
#define AM_EVAL_FAD 1u
#define AM_EVAL_KD 2u
#define AM_EVAL_PRDC 4u
#define AM_EVAL_HEAD 16
typedef struct am_evaluate_side {
    const double* mean;      /* in:  statistics already computed (both or neither) */
    const double* cov;
    const float* radii;      /* in:  radii for nearest_k already computed */
    double* mean_out;        /* out: where statistics computed by this call go (else workspace) */
    double* cov_out;
    float* radii_out;        /* out: where radii computed by this call go (else workspace) */
} am_evaluate_side;
size_t am_evaluate_workspace_bytes(int64_t n_ref, int64_t n_cand, int D, int nearest_k, int kd_subsets, int kd_m, unsigned what);
int am_evaluate_f32(const float* ref, int64_t n_ref, int64_t ld_ref, const float* cand, int64_t n_cand, int64_t ld_cand, int D,
                    unsigned what, int nearest_k, const int64_t* idx_cand, const int64_t* idx_ref, int kd_subsets, int kd_m,
                    double kd_gamma, double kd_coef0, int kd_degree, const am_evaluate_side* given_ref,
                    const am_evaluate_side* given_cand, double* out, void* ws, size_t ws_bytes, am_stream_t stream,
                    am_stream_t side_stream);

/* ---------------------------------------------------------------------------
 * One call = one RANK's share of a row-sharded evaluate: the exchange schedule of
 * audio-metrics_amd/distributed.py: evaluate_sharded behind the C ABI, for one-process-per-GPU hosts that are not Python.
 * The reference has no multi-GPU metrics path (its only multi-GPU code spreads the embedder, util/gpu_parallel.py:79-118).
 *
 *   am_collectives   the two collectives of the schedule as hooks: the library links no collective library.  Both enqueue
 *                    on the stream they are handed (ncclAllReduce / ncclAllGather semantics: stream-ordered, every rank
 *                    calls them in the same order) and return 0 on success.  csrc/rccl/am_rccl.cpp builds them over an
 *                    ncclComm_t (libaudio_metrics_rccl.so: am_rccl_collectives), the tests over torch.distributed.
 *     all_reduce_sum(ctx, buf, count, dtype, stream)        in place; dtype AM_COLL_F64 or AM_COLL_I32
 *     all_gather_v(ctx, send, recv, bytes_per_rank, stream) recv = the ranks' contributions in rank order, rank r's being
 *                    bytes_per_rank[r] bytes (a HOST array of `world` entries, valid during the call only; zero allowed);
 *                    send == recv + (bytes of the lower ranks): the call is always IN PLACE
 *   Every rank passes its row shards (row-major f32, ld % 4 == 0, 16-byte aligned; a shard may be empty - NULL - as long as
 *   each set has rows somewhere), the shard sizes of ALL ranks (host arrays [world], the same on every rank), the metrics
 *   and, for the kernel distance, the two int64 [kd_subsets, kd_m] DEVICE index tables (the same on every rank:
 *   am_kd_draw_indices).  Compute runs on `stream`, the collectives in issue order on `comm_stream` (fenced with events;
 *   pass `stream` itself, or NULL, for the serial form), the Frechet solve on `side_stream`.
 *   Results: the record of am_evaluate_f32 in `out` (device, 16 + kd_subsets doubles), identical on every rank.
 *   Wide, large sets with rows on every rank take the partitioned symmetric k-NN sweep (am_knn_sym_eligible), everything
 *   else the general kernel on the row shard and an all-gather of the radii.
 * ------------------------------------------------------------------------- */
#define AM_COLL_F64 0
#define AM_COLL_I32 1
typedef struct am_collectives {
    void* ctx;
    int rank, world;
    int (*all_reduce_sum)(void* ctx, void* buf, int64_t count, int dtype, am_stream_t stream);
    int (*all_gather_v)(void* ctx, const void* send, void* recv, const int64_t* bytes_per_rank, am_stream_t stream);
} am_collectives;
size_t am_evaluate_sharded_workspace_bytes(const int64_t* ref_counts, const int64_t* cand_counts, int rank, int world, int D,
                                           int nearest_k, int kd_subsets, int kd_m, unsigned what);
int am_evaluate_sharded_f32(const float* ref_local, int64_t ld_ref, const float* cand_local, int64_t ld_cand, int D,
                            const int64_t* ref_counts, const int64_t* cand_counts, const am_collectives* coll, unsigned what,
                            int nearest_k, const int64_t* idx_cand, const int64_t* idx_ref, int kd_subsets, int kd_m,
                            double kd_gamma, double kd_coef0, int kd_degree, double* out, void* ws, size_t ws_bytes,
                            am_stream_t stream, am_stream_t side_stream, am_stream_t comm_stream);

/* ---- optional kernel clock (benchmark support; bench.py's roofline) --------------------------------
 * When enabled, the library brackets every launch of the two tile kernels with a hipEvent pair recorded on
 * the caller's stream, so a benchmark can report the duration of exactly that kernel (the figure
 * `rocprofv3 --kernel-trace --stats` prints for it) rather than of the whole entry point.
 *   AM_KERNEL_KNN          the k-NN tile kernel: knn_wide_kernel / knn_fast_kernel (f16 filter sweep) where the filter path runs,
 *                          else knn_sym_kernel, else knn_partial_kernel's main pass (sampled pre-passes not counted)
 *   AM_KERNEL_PRDC_CROSS   the membership tile kernel: cross_pstat*_kernel / cross_wide_kernel (f16 filter) or prdc_cross_kernel
 *   AM_KERNEL_KNN_VERIFY   knn_fast_verify_kernel (exact f32 values of the queued pairs)
 *   AM_KERNEL_PRDC_VERIFY  cross_verify_regions_kernel (cross_verify_regions64_kernel for float64 rows)
 * am_kernel_clock_read waits for the recorded launches, returns their count and summed duration in
 * milliseconds, and resets that kernel's record.  Disabled by default; no cost when disabled.
 * am_knn_path / am_prdc_path tell which form the library picks for a shape (0 = exact general kernel,
 * 1 = exact symmetric kernel (k-NN only), 2 = f16 filter + exact verification on the 128 x 128 engine (k-NN only),
 * 3 = the same on the 256 x 256 f16 engine, 4 = row-at-a-time kernel for k > AM_MAX_K); am_prdc_path returns 0 or 3.
 * The choice is a pure function of
 * the shapes; inside forms 2 / 3 the DATA can still hand a call to the exact kernels on the device (rows the f16 values
 * cannot separate, queue overflow, operands that cannot be scaled into f16) - am_filter_stats_enable counts those. */
enum am_clocked_kernel { AM_KERNEL_KNN = 0, AM_KERNEL_PRDC_CROSS = 1, AM_KERNEL_KNN_VERIFY = 2, AM_KERNEL_PRDC_VERIFY = 3 };
int am_kernel_clock_enable(int on);
int am_kernel_clock_read(int kernel, int64_t* launches, double* total_ms);
int am_knn_path(int64_t N, int64_t M, int D, int k, int self);
int am_prdc_path(int64_t Nr, int64_t Nc, int D);
/* am_kd_path: which form am_kd_poly_f32 (rbf = 0) / am_kd_rbf_f32 (rbf = 1) take for a shape (set sizes, row strides in
 * elements, feature width, subset size, polynomial degree): 0 = f32 tile kernel, 1 = the same with an inner-dimension tail
 * (D % 32 != 0), 2 = generic pointer form (N * ld * 4 bytes of either set >= 4 GiB), 3 = split-f16 form (polynomial,
 * degree 3, m >= 512, 128 <= D <= 8192); -1 for shapes the entry points reject.  float64 rows take am_kd_*_f64 instead. */
int am_kd_path(int64_t N1, int64_t ldx, int64_t N2, int64_t ldy, int D, int m, int degree, int rbf);
/* form 3 has three tile engines, chosen by the row length alone: 1 = operand-stationary (csrc/pstat_engine.h: the workgroup's
 * 256-row block held in registers, kernels knn_pstat_kernel / cross_pstat_kernel; rows of up to 512 elements),
 * 2 = the same as two independent 256-thread workgroups per CU whose waves own two row tiles (Pstat64Body: kernels
 * knn_pstat64_kernel / cross_pstat64_kernel; rows of up to 128 elements),
 * 0 = both operands streamed through LDS (csrc/wide_engine.h: knn_wide_kernel / cross_wide_kernel) */
int am_filter_engine(int D);

/* ---- optional filter statistics (benchmark support) -------------------------------------------------
 * What the f16 filter passes leave for the exact kernels is data dependent.  A caller hands the library a
 * zero-initialised DEVICE buffer of AM_FILTER_STATS_SLOTS int64 (on the current device; NULL switches the feature
 * off); every filter-form call of am_knn_radii_f32 / am_knn_sym_part_f32 / am_prdc_counts_f32 then ends with a one-
 * workgroup kernel that ADDS to it, stream-ordered, no synchronisation:
 *   [0] k-NN calls           [1] entries queued by the sweep (both directions)   [2] of those via the spill queue
 *   [3] pairs evaluated exactly (after pruning)           [4] rows recomputed by the exact fix-up kernel
 *   [5] membership calls     [6] pairs queued            [7] of those via the overflow queue
 *   [8] membership calls handed to the exact kernel (queues overflowed / operands not scalable)
 *   [9] the error bound of the f16 filter, MEASURED: max over every pair the k-NN verification evaluated of
 *       |f16 matrix-core value - exact f32 value| / (fast_c(D) (|x|^2 + G)), as the bit pattern of a float in the low half
 *       (the filter is sound while this stays <= 1; csrc/pairwise_fast.h derives the bound)     [10] pairs it was measured on
 * The caller reads and clears the buffer itself. */
#define AM_FILTER_STATS_SLOTS 16
int am_filter_stats_enable(int64_t* device_slots);

#ifdef __cplusplus
}
#endif
#endif /* AUDIO_METRICS_HIP_H */
