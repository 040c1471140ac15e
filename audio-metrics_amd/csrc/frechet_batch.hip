// B independent Frechet distances in one stream-ordered chain (am_frechet_batch_f64): the Newton-Schulz solve of
// frechet.hip with the set index in the grid.  Every launch covers all B products - blockIdx.z carries the set (and, in the
// update, which of Y' = Y T / Z' = T Z) - so an iteration is still two launches and the grid is B times larger: 256 / 512
// workgroups of a latency-bound 512 x 512 product become B * 256 / B * 512.  Each set has its own NsState pair, tile sums
// and stop code; the workgroups of a set that has stopped return at once, exactly as the kernels behind the stopping point
// of a single solve do.  The per-set arithmetic is that of frechet.hip (ns_engine.h: same tile product, same summation
// orders, same rule), so for every set the five output doubles are those am_frechet_enqueue_f64 gives on that pair.
// The host enqueues blocks of am_frechet_first_block() iterations and reads the B records once per block; it goes on while
// some set's stop code is 0.
#include "am_common.h"
#include "ns_engine.h"
#include <algorithm>
#include <vector>

namespace am {

// per-set strides (elements) of the batched buffers; y_cov / y_mu are 0 when all sets share one reference
struct NsBatch {
    int64_t dd;          // D * D
    int tiles;           // g * g
    int g;
};

// A_b = Cx_b * Cy_b and per-tile sums of A_b^2
__global__ void __launch_bounds__(256) nsb_product_kernel(const double* __restrict__ cov_x, const double* __restrict__ cov_y,
                                                          int64_t y_stride, double* __restrict__ A, int n, NsBatch nb,
                                                          double* __restrict__ tile_sums) {
    __shared__ __attribute__((aligned(16))) double part[4 * GT * PST];
    __shared__ double red[4];
    const int set = blockIdx.z;
    const GemmJob job{cov_x + set * nb.dd, cov_y + set * y_stride, A + set * nb.dd};
    const int row0 = blockIdx.y * GT, col0 = blockIdx.x * GT;
    double v[4];
    tile_product(job, n, row0, col0, part, v);
    double sq = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = threadIdx.x + 256 * q;
        const int gr = row0 + (e >> 5), gc = col0 + (e & 31);
        if (gr < n && gc < n) {
            job.C[(int64_t)gr * n + gc] = v[q];
            sq += v[q] * v[q];
        }
    }
    sq = block_sum(sq, red);
    if (threadIdx.x == 0) tile_sums[(int64_t)set * nb.tiles + blockIdx.y * gridDim.x + blockIdx.x] = sq;
}

// per set: norm = sqrt(sum tile_sums); Y = A / norm; Z = I; state init (grid.y = set)
__global__ void __launch_bounds__(256) nsb_init_kernel(const double* __restrict__ A, const double* __restrict__ tile_sums, int n,
                                                       NsBatch nb, double* __restrict__ Y, double* __restrict__ Z,
                                                       NsState* __restrict__ state) {
    __shared__ double red[4];
    const int set = blockIdx.y;
    A += set * nb.dd;
    Y += set * nb.dd;
    Z += set * nb.dd;
    tile_sums += (int64_t)set * nb.tiles;
    double v = 0;
    for (int i = threadIdx.x; i < nb.tiles; i += blockDim.x) v += tile_sums[i];
    const double nrm = sqrt(block_sum(v, red));
    const bool bad = !(nrm == nrm) || isinf(nrm);
    const double inv = (nrm > 0.0 && !bad) ? 1.0 / nrm : 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nb.dd; i += (int64_t)gridDim.x * blockDim.x) {
        Y[i] = A[i] * inv;
        Z[i] = (i / n == i % n) ? 1.0 : 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        NsState* s = state + 2 * set;
        s->prev_trace = (nrm > 0.0 && !bad) ? -INFINITY : 0.0;
        s->resid = 0.0;
        s->norm = bad ? 0.0 : nrm;
        s->iters = 0;
        s->done = bad ? 4 : (nrm > 0.0 ? 0 : 3);
    }
}

// per set: T = 1.5 I - 0.5 Z Y, sums of (I - Z Y)^2 per tile and of diag(Y) per diagonal tile.  `cur`: which half of the
// ping-pong buffers holds the iterate
__global__ void __launch_bounds__(256) nsb_t_kernel(const double* __restrict__ Zc, const double* __restrict__ Yc, double* __restrict__ T,
                                                    int n, NsBatch nb, const NsState* __restrict__ state, int cur,
                                                    double* __restrict__ resid_sums, double* __restrict__ trace_sums) {
    const int set = blockIdx.z;
    if (state[2 * set + cur].done) return;
    __shared__ __attribute__((aligned(16))) double part[4 * GT * PST];
    __shared__ double red[4];
    const GemmJob job{Zc + set * nb.dd, Yc + set * nb.dd, T + set * nb.dd};
    const int row0 = blockIdx.y * GT, col0 = blockIdx.x * GT;
    double v[4];
    tile_product(job, n, row0, col0, part, v);
    double sq = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = threadIdx.x + 256 * q;
        const int gr = row0 + (e >> 5), gc = col0 + (e & 31);
        if (gr < n && gc < n) {
            const double eye = (gr == gc) ? 1.0 : 0.0;
            const double d = eye - v[q];
            job.C[(int64_t)gr * n + gc] = 1.5 * eye - 0.5 * v[q];
            sq += d * d;
        }
    }
    sq = block_sum(sq, red);
    if (threadIdx.x == 0) resid_sums[(int64_t)set * nb.tiles + blockIdx.y * gridDim.x + blockIdx.x] = sq;
    if (blockIdx.x == blockIdx.y) {
        const int i = row0 + (int)threadIdx.x;
        const double t = (threadIdx.x < GT && i < n) ? job.B[(int64_t)i * n + i] : 0.0;
        const double ts = block_sum(t, red);
        if (threadIdx.x == 0) trace_sums[(int64_t)set * nb.g + blockIdx.x] = ts;
    }
}

// per set: state[cur ^ 1] = rule(state[cur]); unless stopped: Y' = Y T (z even), Z' = T Z (z odd).  products == 0: the rule
// only, one workgroup per set (grid.z = B)
__global__ void __launch_bounds__(256) nsb_update_kernel(const double* __restrict__ Yc, const double* __restrict__ Zc,
                                                         const double* __restrict__ T, double* __restrict__ Yn, double* __restrict__ Zn,
                                                         int n, NsBatch nb, NsState* __restrict__ state, int cur,
                                                         const double* __restrict__ resid_sums, const double* __restrict__ trace_sums,
                                                         double tol, int products) {
    __shared__ __attribute__((aligned(16))) double part[4 * GT * PST];
    __shared__ double red[4];
    const int set = products ? blockIdx.z >> 1 : blockIdx.z;
    const int which = products ? blockIdx.z & 1 : 0;
    const NsState s = state[2 * set + cur];
    NsState* state_out = state + 2 * set + (cur ^ 1);
    const bool writer = blockIdx.x == 0 && blockIdx.y == 0 && which == 0 && threadIdx.x == 0;
    if (s.done) {
        if (writer) *state_out = s;
        return;
    }
    const NsState o = ns_next_state(s, resid_sums + (int64_t)set * nb.tiles, nb.tiles, trace_sums + (int64_t)set * nb.g, nb.g, n,
                                    tol, red);
    if (writer) *state_out = o;
    if (o.done || !products) return;
    const int64_t off = set * nb.dd;
    const GemmJob job = which == 0 ? GemmJob{Yc + off, T + off, Yn + off} : GemmJob{T + off, Zc + off, Zn + off};
    const int row0 = blockIdx.y * GT, col0 = blockIdx.x * GT;
    double v[4];
    tile_product(job, n, row0, col0, part, v);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = threadIdx.x + 256 * q;
        const int gr = row0 + (e >> 5), gc = col0 + (e & 31);
        if (gr < n && gc < n) job.C[(int64_t)gr * n + gc] = v[q];
    }
}

// out[set] = { fd, tr_sqrt, iterations, residual, stop code }
__global__ void __launch_bounds__(256) nsb_finish_kernel(const double* __restrict__ mu_x, const double* __restrict__ cov_x,
                                                         const double* __restrict__ mu_y, const double* __restrict__ cov_y,
                                                         int64_t y_stride_mu, int64_t y_stride_cov, int n, NsBatch nb,
                                                         const NsState* __restrict__ state, int fin, double* __restrict__ out) {
    __shared__ double red[4];
    const int set = blockIdx.x;
    mu_x += (int64_t)set * n;
    cov_x += set * nb.dd;
    mu_y += set * y_stride_mu;
    cov_y += set * y_stride_cov;
    double a = 0, b = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const double d = mu_x[i] - mu_y[i];
        a += d * d;
        b += cov_x[(int64_t)i * n + i] + cov_y[(int64_t)i * n + i];
    }
    a = block_sum(a, red);
    b = block_sum(b, red);
    if (threadIdx.x == 0) {
        const NsState* s = state + 2 * set + fin;
        const double tr = (s->done == 3) ? 0.0 : s->prev_trace * sqrt(s->norm);
        double* o = out + 5 * set;
        o[0] = a + b - 2.0 * tr;
        o[1] = tr;
        o[2] = (double)s->iters;
        o[3] = s->resid;
        o[4] = (double)s->done;
    }
}

struct NsBatchBuffers {
    double *A, *Y[2], *Z[2], *T, *resid_sums, *trace_sums;
    NsState* state;               // [B][2]: ping-pong per set
    NsBatch nb;
};

static bool carve_nsb(Carver& c, int B, int D, NsBatchBuffers& b) {
    const size_t dd = (size_t)D * D;
    b.nb.g = (int)ceil_div(D, GT);
    b.nb.tiles = b.nb.g * b.nb.g;
    b.nb.dd = (int64_t)dd;
    b.A = c.take<double>(B * dd);
    b.Y[0] = c.take<double>(B * dd);
    b.Y[1] = c.take<double>(B * dd);
    b.Z[0] = c.take<double>(B * dd);
    b.Z[1] = c.take<double>(B * dd);
    b.T = c.take<double>(B * dd);
    b.resid_sums = c.take<double>((size_t)B * b.nb.tiles);
    b.trace_sums = c.take<double>((size_t)B * b.nb.g);
    b.state = c.take<NsState>((size_t)B * 2);
    return c.ok();
}

static int enqueue_nsb(const double* mu_x, const double* cov_x, const double* mu_y, const double* cov_y, int64_t y_sets, int B, int D,
                       int first_iter, int n_iter, bool last_block, double tol, const NsBatchBuffers& b, double* out_dev,
                       hipStream_t st) {
    const unsigned g = (unsigned)b.nb.g;
    const dim3 grid1(g, g, (unsigned)B), grid2(g, g, 2u * (unsigned)B), blk(256);
    const int64_t y_cov = y_sets ? b.nb.dd : 0, y_mu = y_sets ? D : 0;
    if (first_iter == 0) {
        hipLaunchKernelGGL(nsb_product_kernel, grid1, blk, 0, st, cov_x, cov_y, y_cov, b.A, D, b.nb, b.resid_sums);
        AM_LAUNCH_CHECK();
        hipLaunchKernelGGL(nsb_init_kernel, dim3((unsigned)std::min<int64_t>(256, ceil_div((int64_t)D * D, 1024)), (unsigned)B), blk, 0,
                           st, (const double*)b.A, (const double*)b.resid_sums, D, b.nb, b.Y[0], b.Z[0], b.state);
        AM_LAUNCH_CHECK();
    }
    for (int it = first_iter; it < first_iter + n_iter; ++it) {
        const int cur = it & 1;
        hipLaunchKernelGGL(nsb_t_kernel, grid1, blk, 0, st, (const double*)b.Z[cur], (const double*)b.Y[cur], b.T, D, b.nb,
                           (const NsState*)b.state, cur, b.resid_sums, b.trace_sums);
        hipLaunchKernelGGL(nsb_update_kernel, grid2, blk, 0, st, (const double*)b.Y[cur], (const double*)b.Z[cur], (const double*)b.T,
                           b.Y[cur ^ 1], b.Z[cur ^ 1], D, b.nb, b.state, cur, (const double*)b.resid_sums,
                           (const double*)b.trace_sums, tol, 1);
        AM_LAUNCH_CHECK();
    }
    int fin = (first_iter + n_iter) & 1;
    if (last_block) {
        hipLaunchKernelGGL(nsb_t_kernel, grid1, blk, 0, st, (const double*)b.Z[fin], (const double*)b.Y[fin], b.T, D, b.nb,
                           (const NsState*)b.state, fin, b.resid_sums, b.trace_sums);
        hipLaunchKernelGGL(nsb_update_kernel, dim3(1, 1, (unsigned)B), blk, 0, st, (const double*)nullptr, (const double*)nullptr,
                           (const double*)nullptr, (double*)nullptr, (double*)nullptr, D, b.nb, b.state, fin,
                           (const double*)b.resid_sums, (const double*)b.trace_sums, tol, 0);
        AM_LAUNCH_CHECK();
        fin ^= 1;
    }
    hipLaunchKernelGGL(nsb_finish_kernel, dim3((unsigned)B), blk, 0, st, mu_x, cov_x, mu_y, cov_y, y_mu, y_cov, D, b.nb,
                       (const NsState*)b.state, fin, out_dev);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

}  // namespace am

using namespace am;

extern "C" size_t am_frechet_batch_workspace_bytes(int B, int D) {
    if (B < 1 || D < 1) return 0;
    Carver c(nullptr, 0);
    NsBatchBuffers b;
    carve_nsb(c, B, D, b);
    return c.off;
}

extern "C" int am_frechet_batch_f64(const double* mu_x, const double* cov_x, const double* mu_y, const double* cov_y,
                                    int64_t y_stride_sets, int B, int D, int max_iter, double tol, double* out_dev, void* ws,
                                    size_t ws_bytes, am_stream_t stream) {
    AM_REQUIRE(mu_x && cov_x && mu_y && cov_y && out_dev, AM_ERR_BAD_ARG, "null pointer");
    AM_REQUIRE(D >= 1 && B >= 1 && B <= 16384, AM_ERR_BAD_SHAPE, "B=%d D=%d (1 <= B <= 16384)", B, D);
    AM_REQUIRE(y_stride_sets == 0 || y_stride_sets == 1, AM_ERR_BAD_ARG, "y_stride_sets=%lld (0: one shared y, 1: one y per set)",
               (long long)y_stride_sets);
    if (max_iter <= 0) max_iter = 64;
    if (!(tol > 0)) tol = 1e-13;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Carver c(ws, ws_bytes);
    NsBatchBuffers b;
    AM_REQUIRE(carve_nsb(c, B, D, b), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes, have %zu", c.off, ws_bytes);
    std::vector<double> rec((size_t)B * 5, 0.0);
    for (int first = 0; first < max_iter;) {
        const int n_iter = std::min(am_frechet_first_block(), max_iter - first);
        const int rc = enqueue_nsb(mu_x, cov_x, mu_y, cov_y, y_stride_sets, B, D, first, n_iter, first + n_iter >= max_iter, tol, b,
                                   out_dev, st);
        if (rc != AM_OK) return rc;
        AM_HIP_TRY(hipMemcpyAsync(rec.data(), out_dev, rec.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        AM_HIP_TRY(hipStreamSynchronize(st));          // once per block for the whole batch
        first += n_iter;
        bool running = false;
        for (int s = 0; s < B; ++s) running = running || (int)rec[5 * s + 4] == 0;
        if (!running) break;
    }
    for (int s = 0; s < B; ++s)
        AM_REQUIRE((int)rec[5 * s + 4] != 4, AM_ERR_NO_CONVERGENCE,
                   "set %d of %d: non-finite covariance product or trace in Newton-Schulz", s, B);
    return AM_OK;
}
