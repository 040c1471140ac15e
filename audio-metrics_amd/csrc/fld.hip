// Feature likelihood divergence on the f32 tile engine: a mixture of M isotropic Gaussians, one per generated row g_j with its
// own variance sigma_j^2 = exp(theta_j), evaluated on N rows and fitted to them - without an N x M matrix in either direction.
//
//     h_j = 0.5 exp(-theta_j),  c_j = (D / 2) theta_j              f64, rounded to f32 once per pass (fld_columns_kernel)
//     d2  = max(fmaf(-2, <x, g>, |x|^2 + |g|^2), 0)                NaN -> +inf (clamp0): the bits of the search and the soft-min
//     z_ij = fmaf(-d2_ij, h_j, -c_j)                               f32
//
// am_fld_loglik_f32 - rows are the evaluated points, columns the centres:
//     l_i = logsumexp_j z_ij - log M - (D / 2) log 2 pi
// the online log-sum-exp of softmin.hip (a running f32 maximum, the f64 sum of exp(z - max), exp in f64; the four pairs of a
// row meet in LDS, the chunks' pairs in the merge kernel, in a fixed order) with a bandwidth per column where the soft-min has
// one temperature: three aux floats per column in LDS (|g_j|^2, h_j, -c_j).  The merge kernel writes l_i and the block sums
// of { l_i, 1 } over the rows with a finite l_i; fld_stats_kernel adds the blocks in block order: stats = { sum of finite l,
// rows with a finite l, rows without }.
//
// am_fld_grad_f32 - the swapped sweep: rows are the centres, columns the evaluated rows.  With the responsibilities
// r_ij = exp(z_ij - lse_i), lse_i = l_i + log M + (D / 2) log 2 pi (two f32 halves per column, so that r sums to 1 over j to
// f64 accuracy; z has the bits it has in the other sweep: the dot product, the sum of the two norms and the fmaf do not
// depend on which operand is the row)
//     A_j = sum_i r_ij,   B_j = sum_i r_ij d2_ij                   f64 per lane, joined in LDS and over the chunks in a fixed order
// A column without a finite l_i (a row with a non-finite element), a padded column and a centre with a non-finite element
// sit at distance +inf: z = -inf, r = 0, and the product r d2 is formed with 0 in place of +inf - exactly 0 in both sums.
// The merge kernel turns the sums into dL/dtheta_j = -(h_j B_j - (D / 2) A_j) / n_finite and applies one Adam step with the
// clamp, so that a step of the fit reads nothing back.
//
// No floating-point atomics anywhere: every call returns the same bits at the same shapes.
//
// Register budget: the soft-min's (64 accumulators, 64 staging registers, 32 fragment registers); lane state is 6 registers
// in the loglik sweep (mx, s for two rows) and 8 in the gradient sweep (A, B for two rows; |g|^2, h, -c of the rows wait in
// LDS), whose epilogue has no maximum pass and loads its aux values four columns at a time.  __launch_bounds__(256, 2), two
// workgroups per CU.
#include "row_sweep.h"
#include <float.h>
#include <math.h>

namespace am {
namespace fld {

constexpr size_t LDS_BYTES = (ENGINE_LDS_FLOATS + 2 * 3 * TB) * sizeof(float);   // staging slabs + [2][3][128] aux values
constexpr size_t GRAD_LDS_BYTES = LDS_BYTES + 3 * TB * sizeof(float);            // ... + [3][128] values of the rows
constexpr int MERGE_THREADS = 256;
constexpr double THETA_MAX = 30.0;
constexpr double ADAM_B1 = 0.9, ADAM_B2 = 0.999, ADAM_EPS = 1e-8;

__device__ __forceinline__ float z_of(float a, float norms, float h, float negc, float& d2) {
    d2 = clamp0(fmaf(-2.f, a, norms));
    return fmaf(-d2, h, negc);                       // d2 = +inf -> -inf (h is a positive normal number, -c is finite)
}

struct LoglikEpilogue : ColumnAux<PAD_INF, PAD_ONE, PAD_ZERO> {      // |g_j|^2 of the tile, h_j, -c_j
    float xn[2];
    float mx[2];
    double s[2];

    __device__ __forceinline__ LoglikEpilogue(const LaneInfo& l) : ColumnAux<PAD_INF, PAD_ONE, PAD_ZERO>(l) {}

    __device__ __forceinline__ void finish(int t, int64_t, f32x16 (&acc)[2][2]) {
        const float* a = tile(t);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            f32x4 gn[4], hq[4], cq[4];
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                gn[g4] = *reinterpret_cast<const f32x4*>(a + mt * 32 + g4 * 8);
                hq[g4] = *reinterpret_cast<const f32x4*>(a + TB + mt * 32 + g4 * 8);
                cq[g4] = *reinterpret_cast<const f32x4*>(a + 2 * TB + mt * 32 + g4 * 8);
            }
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                float tmax = -INFINITY, d2;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg)
                    tmax = fmaxf(tmax, z_of(acc[mt][nt][reg], xn[nt] + gn[reg >> 2][reg & 3], hq[reg >> 2][reg & 3], cq[reg >> 2][reg & 3], d2));
                const double ref = lse_raise(mx[nt], s[nt], tmax);
                double sum = s[nt];
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const float z = z_of(acc[mt][nt][reg], xn[nt] + gn[reg >> 2][reg & 3], hq[reg >> 2][reg & 3], cq[reg >> 2][reg & 3], d2);
                    sum += exp((double)z - ref);
                    if ((reg & 3) == 3) __builtin_amdgcn_sched_barrier(0);               // four exp chains at a time: more in flight spill
                }
                s[nt] = sum;
            }
        }
    }
};

// columns: |x_i|^2 (+inf for a row without a finite l_i: fld_lse_columns_kernel), then the two halves of lse_i = lhi + llo
struct GradEpilogue : ColumnAux<PAD_INF, PAD_ZERO, PAD_ZERO> {
    const float* rowaux;                 // LDS [3][128] : |g_j|^2, h_j, -c_j of the workgroup's rows (not kept in registers)
    double A[2], B[2];

    __device__ __forceinline__ GradEpilogue(const LaneInfo& l) : ColumnAux<PAD_INF, PAD_ZERO, PAD_ZERO>(l) {}

    __device__ __forceinline__ void finish(int t, int64_t, f32x16 (&acc)[2][2]) {
        const float* a = tile(t);
        float gn[2], h[2], negc[2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int row = sweep_row(0, L, nt);
            gn[nt] = rowaux[row];
            h[nt] = rowaux[TB + row];
            negc[nt] = rowaux[2 * TB + row];
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const f32x4 xq = *reinterpret_cast<const f32x4*>(a + mt * 32 + g4 * 8);
                const f32x4 hi = *reinterpret_cast<const f32x4*>(a + TB + mt * 32 + g4 * 8);
                const f32x4 lo = *reinterpret_cast<const f32x4*>(a + 2 * TB + mt * 32 + g4 * 8);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    double sa = A[nt], sb = B[nt];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float d2;
                        const float z = z_of(acc[mt][nt][g4 * 4 + e], gn[nt] + xq[e], h[nt], negc[nt], d2);
                        const double r = exp(((double)z - (double)hi[e]) - (double)lo[e]);       // z = -inf: exactly 0
                        sa += r;
                        sb = fma(r, (double)(d2 < INFINITY ? d2 : 0.f), sb);                     // never 0 * inf
                        // both sums are final here: left free, the compiler forms the 64 arguments of a tile first and the
                        // exp chains last, and 180 bytes per lane go to scratch
                        asm volatile("" : "+v"(sa), "+v"(sb));
                    }
                    A[nt] = sa;
                    B[nt] = sb;
                    __builtin_amdgcn_sched_barrier(0);                 // four exp chains at a time
                }
            }
        }
    }
};

// h[j] = (float)(0.5 exp(-theta_j)), negc[j] = (float)(-(D / 2) theta_j).  A theta that gives no normal f32 h (or is not
// finite) takes its centre out of the mixture: norm +inf, as a centre with a non-finite element has it.  Runs behind the
// norms of the centres.
__global__ void __launch_bounds__(MERGE_THREADS)
fld_columns_kernel(const double* __restrict__ theta, int64_t M, double half_d, float* __restrict__ h, float* __restrict__ negc,
                   float* __restrict__ gnorm) {
    const int64_t j = (int64_t)blockIdx.x * MERGE_THREADS + threadIdx.x;
    if (j >= M) return;
    const double t = theta[j];
    const float hf = (float)(0.5 * exp(-t));
    const float cf = (float)(-(half_d * t));
    const bool ok = hf >= FLT_MIN && hf <= FLT_MAX && fabsf(cf) <= FLT_MAX;
    h[j] = ok ? hf : 1.f;
    negc[j] = ok ? cf : 0.f;
    if (!ok) gnorm[j] = INFINITY;
}

// the two f32 halves of lse_i = loglik_i + konst; a row without a finite log-likelihood leaves the sweep (norm +inf).
// Runs behind the norms of the rows.
__global__ void __launch_bounds__(MERGE_THREADS)
fld_lse_columns_kernel(const double* __restrict__ loglik, int64_t N, double konst, float* __restrict__ xnorm,
                       float* __restrict__ lhi, float* __restrict__ llo) {
    const int64_t i = (int64_t)blockIdx.x * MERGE_THREADS + threadIdx.x;
    if (i >= N) return;
    const double v = loglik[i] + konst;
    const float hi = (float)v;
    const bool ok = isfinite(v) && fabsf(hi) <= FLT_MAX;
    lhi[i] = ok ? hi : 0.f;
    llo[i] = ok ? (float)(v - (double)hi) : 0.f;
    if (!ok) xnorm[i] = INFINITY;
}

// part_mx / part_s[chunk * N + row] = the (max, sum) pair of `row` inside column chunk `chunk`
template <bool KTAIL>
__global__ void __launch_bounds__(ENGINE_THREADS, 2)
fld_loglik_kernel(const float* __restrict__ X, int64_t N, int64_t ldx, const float* __restrict__ xnorm, const float* __restrict__ G,
                  int64_t M, int64_t ldg, const float* __restrict__ gnorm, const float* __restrict__ hcol,
                  const float* __restrict__ ccol, int D, int nchunks, float* __restrict__ part_mx, double* __restrict__ part_s) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LaneInfo L;
    const WorkItem w = work_item((M + TB - 1) / TB, nchunks);
    const int chunk = blockIdx.x % nchunks;            // the chunk work_item gave this workgroup: its slice of the partials

    LoglikEpilogue epi(L);
    epi.src[0] = gnorm;
    epi.src[1] = hcol;
    epi.src[2] = ccol;
    epi.nc = M;
    epi.lds = lds + ENGINE_LDS_FLOATS;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        epi.xn[nt] = row_norm(xnorm, w.prow0, N, L, nt);
        epi.mx[nt] = -INFINITY;
        epi.s[nt] = 0.0;
    }
    dense_pipeline_early<EV_DEFAULT, KTAIL>(G, M, ldg, LinearTiles{w.qtile0}, X, N, ldx, w.prow0, w.ntiles, D, lds, L, epi);

    // a row is covered by 4 pairs (2 half-waves x 2 column-half waves): [128][4] sums, then [128][4] maxima, through the
    // staging slabs, free now
    double* ms = reinterpret_cast<double*>(lds);
    float* mm = lds + 2 * TB * 4;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int slot = join_slot(L, nt);
        ms[slot] = epi.s[nt];
        mm[slot] = epi.mx[nt];
    }
    __syncthreads();
    if (L.tid < 128) {
        const int64_t i = joined_row(w.prow0, L.tid);
        if (i < N) {
            float m = mm[L.tid * 4];
            double s = ms[L.tid * 4];
#pragma unroll
            for (int k = 1; k < 4; ++k) lse_join(m, s, mm[L.tid * 4 + k], ms[L.tid * 4 + k]);
            part_mx[(int64_t)chunk * N + i] = m;
            part_s[(int64_t)chunk * N + i] = s;
        }
    }
}

// part_a / part_b[chunk * M + centre] = the (A, B) sums of `centre` over the rows of column chunk `chunk`
template <bool KTAIL>
__global__ void __launch_bounds__(ENGINE_THREADS, 2)
fld_grad_kernel(const float* __restrict__ G, int64_t M, int64_t ldg, const float* __restrict__ gnorm, const float* __restrict__ hrow,
                const float* __restrict__ crow, const float* __restrict__ X, int64_t N, int64_t ldx, const float* __restrict__ xnorm,
                const float* __restrict__ lhi, const float* __restrict__ llo, int D, int nchunks, double* __restrict__ part_a,
                double* __restrict__ part_b) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LaneInfo L;
    const WorkItem w = work_item((N + TB - 1) / TB, nchunks);
    const int chunk = blockIdx.x % nchunks;

    GradEpilogue epi(L);
    epi.src[0] = xnorm;
    epi.src[1] = lhi;
    epi.src[2] = llo;
    epi.nc = N;
    epi.lds = lds + ENGINE_LDS_FLOATS;
    float* rowaux = lds + ENGINE_LDS_FLOATS + 2 * 3 * TB;
    epi.rowaux = rowaux;
    if (L.tid < TB) {                                  // visible to finish() behind the pipeline's first barrier
        const int64_t j = w.prow0 + L.tid;
        rowaux[L.tid] = j < M ? gnorm[j] : 0.f;
        rowaux[TB + L.tid] = j < M ? hrow[j] : 1.f;
        rowaux[2 * TB + L.tid] = j < M ? crow[j] : 0.f;
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        epi.A[nt] = 0.0;
        epi.B[nt] = 0.0;
    }
    dense_pipeline_early<EV_DEFAULT, KTAIL>(X, N, ldx, LinearTiles{w.qtile0}, G, M, ldg, w.prow0, w.ntiles, D, lds, L, epi);

    // the 4 pairs of a row: [128][4] A sums, then [128][4] B sums, through the staging slabs, free now; added in slot order
    double* sa = reinterpret_cast<double*>(lds);
    double* sb = sa + TB * 4;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int slot = join_slot(L, nt);
        sa[slot] = epi.A[nt];
        sb[slot] = epi.B[nt];
    }
    __syncthreads();
    if (L.tid < 128) {
        const int64_t j = joined_row(w.prow0, L.tid);
        if (j < M) {
            double a = sa[L.tid * 4], b = sb[L.tid * 4];
#pragma unroll
            for (int k = 1; k < 4; ++k) {
                a += sa[L.tid * 4 + k];
                b += sb[L.tid * 4 + k];
            }
            part_a[(int64_t)chunk * M + j] = a;
            part_b[(int64_t)chunk * M + j] = b;
        }
    }
}

// the chunks' pairs of a row in chunk order -> l_i, and this block's { sum of the finite l_i, their number }
__global__ void __launch_bounds__(MERGE_THREADS)
fld_loglik_merge_kernel(const float* __restrict__ part_mx, const double* __restrict__ part_s, int64_t N, int nchunks, double konst,
                        double* __restrict__ out, double* __restrict__ block_sums) {
    __shared__ double red[MERGE_THREADS];
    const int64_t i = (int64_t)blockIdx.x * MERGE_THREADS + threadIdx.x;
    double l = 0.0, one = 0.0;
    if (i < N) {
        float m = part_mx[i];
        double s = part_s[i];
        for (int c = 1; c < nchunks; ++c) lse_join(m, s, part_mx[(int64_t)c * N + i], part_s[(int64_t)c * N + i]);
        const double v = m > -INFINITY && s > 0.0 ? ((double)m + log(s)) - konst : -INFINITY;
        out[i] = isfinite(v) ? v : -INFINITY;
        if (isfinite(v)) {
            l = v;
            one = 1.0;
        }
    }
    const double sum = block_reduce_256<SumOp>(l, red);
    __syncthreads();
    const double cnt = block_reduce_256<SumOp>(one, red);
    __syncthreads();                                   // guards nothing: kept so the kernel stays the program it was
    if (threadIdx.x == 0) {
        block_sums[2 * (int64_t)blockIdx.x] = sum;
        block_sums[2 * (int64_t)blockIdx.x + 1] = cnt;
    }
}

// one workgroup: the blocks' sums in block order (thread t takes blocks t, t + 256, ...), then the fixed tree
__global__ void __launch_bounds__(MERGE_THREADS)
fld_stats_kernel(const double* __restrict__ block_sums, int64_t nblocks, int64_t N, double* __restrict__ stats) {
    __shared__ double red[MERGE_THREADS];
    double l = 0.0, cnt = 0.0;
    for (int64_t b = threadIdx.x; b < nblocks; b += MERGE_THREADS) {
        l += block_sums[2 * b];
        cnt += block_sums[2 * b + 1];
    }
    const double sum = block_reduce_256<SumOp>(l, red);
    __syncthreads();
    const double n = block_reduce_256<SumOp>(cnt, red);
    __syncthreads();                                   // (as above)
    if (threadIdx.x == 0) {
        stats[0] = sum;
        stats[1] = n;
        stats[2] = (double)N - n;
    }
}

// the chunks' sums of a centre in chunk order -> A_j, B_j -> the gradient -> one Adam step with the clamp.  Every operation
// is a single rounded one in the order of the host formula (fld_adam_step): no contraction into fused multiply-adds.
__global__ void __launch_bounds__(MERGE_THREADS)
fld_grad_merge_kernel(const double* __restrict__ part_a, const double* __restrict__ part_b, int64_t M, int nchunks, double half_d,
                      const double* __restrict__ n_finite, const double* theta, double* adam_m, double* adam_v, double bc1,
                      double bc2, double lr, double theta_min, double* theta_out, double* __restrict__ out_a,
                      double* __restrict__ out_b) {
#pragma clang fp contract(off)
    const int64_t j = (int64_t)blockIdx.x * MERGE_THREADS + threadIdx.x;
    if (j >= M) return;
    double a = part_a[j], b = part_b[j];
    for (int c = 1; c < nchunks; ++c) {
        a += part_a[(int64_t)c * M + j];
        b += part_b[(int64_t)c * M + j];
    }
    if (out_a != nullptr) out_a[j] = a;
    if (out_b != nullptr) out_b[j] = b;
    const double n = n_finite[0];
    const double t = theta[j];
    const double h = 0.5 * exp(-t);
    const double grad = n > 0.0 ? -((h * b - half_d * a) / n) : 0.0;
    const double m = ADAM_B1 * adam_m[j] + (1.0 - ADAM_B1) * grad;
    const double v = ADAM_B2 * adam_v[j] + (1.0 - ADAM_B2) * (grad * grad);
    const double mhat = m / bc1, vhat = v / bc2;
    double tn = t - lr * (mhat / (sqrt(vhat) + ADAM_EPS));
    tn = fmin(fmax(tn, theta_min), THETA_MAX);
    adam_m[j] = m;
    adam_v[j] = v;
    theta_out[j] = tn;
}

static bool shape_ok(int64_t rows, int64_t cols, int D) { return sweep_shape_ok(rows, cols, D, COLUMNS_TILED); }

struct LoglikBuffers {
    float *xn, *gn, *h, *negc, *part_mx;
    double *part_s, *block_sums;
};
static void carve(Carver& c, int64_t N, int64_t M, int nchunks, LoglikBuffers& b) {
    b.xn = c.take<float>((size_t)N);
    b.gn = c.take<float>((size_t)M);
    b.h = c.take<float>((size_t)M);
    b.negc = c.take<float>((size_t)M);
    b.part_mx = c.take<float>((size_t)nchunks * (size_t)N);
    b.part_s = c.take<double>((size_t)nchunks * (size_t)N);
    b.block_sums = c.take<double>(2 * (size_t)ceil_div(N, MERGE_THREADS));
}

struct GradBuffers {
    float *gn, *h, *negc, *xn, *lhi, *llo;
    double *part_a, *part_b;
};
static void carve(Carver& c, int64_t M, int64_t N, int nchunks, GradBuffers& b) {
    b.gn = c.take<float>((size_t)M);
    b.h = c.take<float>((size_t)M);
    b.negc = c.take<float>((size_t)M);
    b.xn = c.take<float>((size_t)N);
    b.lhi = c.take<float>((size_t)N);
    b.llo = c.take<float>((size_t)N);
    b.part_a = c.take<double>((size_t)nchunks * (size_t)M);
    b.part_b = c.take<double>((size_t)nchunks * (size_t)M);
}

static double mixture_constant(int64_t M, int D) { return log((double)M) + 0.5 * (double)D * log(2.0 * M_PI); }

}  // namespace fld
}  // namespace am

using namespace am;

extern "C" size_t am_fld_loglik_workspace_bytes(int64_t N, int64_t M, int D) {
    if (!fld::shape_ok(N, M, D)) return 0;
    Carver c(nullptr, 0);
    fld::LoglikBuffers b;
    fld::carve(c, N, M, choose_chunks(N, M), b);
    return c.off;
}

extern "C" size_t am_fld_grad_workspace_bytes(int64_t M, int64_t N, int D) {
    if (!fld::shape_ok(M, N, D)) return 0;
    Carver c(nullptr, 0);
    fld::GradBuffers b;
    fld::carve(c, M, N, choose_chunks(M, N), b);
    return c.off;
}

extern "C" int am_fld_loglik_f32(const float* X, int64_t N, int64_t ldx, const float* G, int64_t M, int64_t ldg, int D,
                                 const double* theta, double* out_loglik, double* stats, void* ws, size_t ws_bytes,
                                 am_stream_t stream) {
    int rc;
    if ((rc = check_matrix(X, N, ldx, D, "X")) != AM_OK) return rc;
    if ((rc = check_matrix(G, M, ldg, D, "G")) != AM_OK) return rc;
    AM_REQUIRE(theta != nullptr, AM_ERR_BAD_ARG, "theta is null");
    AM_REQUIRE(out_loglik != nullptr, AM_ERR_BAD_ARG, "out_loglik is null");
    AM_REQUIRE(stats != nullptr, AM_ERR_BAD_ARG, "stats is null");
    AM_REQUIRE(fld::shape_ok(N, M, D), AM_ERR_BAD_SHAPE, "N=%lld M=%lld: too large for one launch", (long long)N, (long long)M);
    const int nchunks = choose_chunks(N, M);
    Carver c(ws, ws_bytes);
    fld::LoglikBuffers b;
    fld::carve(c, N, M, nchunks, b);
    AM_REQUIRE(c.ok(), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (am_fld_loglik_workspace_bytes), have %zu", c.off, ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = launch_norms(X, N, ldx, D, b.xn, st)) != AM_OK) return rc;
    if ((rc = launch_norms(G, M, ldg, D, b.gn, st)) != AM_OK) return rc;
    hipLaunchKernelGGL(fld::fld_columns_kernel, dim3((unsigned)ceil_div(M, fld::MERGE_THREADS)), dim3(fld::MERGE_THREADS), 0, st, theta,
                       M, 0.5 * (double)D, b.h, b.negc, b.gn);
    AM_LAUNCH_CHECK();
    rc = launch_sweep(&fld::fld_loglik_kernel<false>, &fld::fld_loglik_kernel<true>, fld::LDS_BYTES, N, nchunks, D, st, X, N, ldx, b.xn, G,
                      M, ldg, b.gn, b.h, b.negc, D, nchunks, b.part_mx, b.part_s);
    if (rc != AM_OK) return rc;
    const int64_t nblocks = ceil_div(N, fld::MERGE_THREADS);
    hipLaunchKernelGGL(fld::fld_loglik_merge_kernel, dim3((unsigned)nblocks), dim3(fld::MERGE_THREADS), 0, st, (const float*)b.part_mx,
                       (const double*)b.part_s, N, nchunks, fld::mixture_constant(M, D), out_loglik, b.block_sums);
    AM_LAUNCH_CHECK();
    hipLaunchKernelGGL(fld::fld_stats_kernel, dim3(1), dim3(fld::MERGE_THREADS), 0, st, (const double*)b.block_sums, nblocks, N, stats);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

extern "C" int am_fld_grad_f32(const float* G, int64_t M, int64_t ldg, const float* X, int64_t N, int64_t ldx, int D,
                               const double* theta, const double* loglik, const double* n_finite, double* adam_m, double* adam_v,
                               int64_t step, double lr, double theta_min, double* theta_out, double* out_a, double* out_b,
                               void* ws, size_t ws_bytes, am_stream_t stream) {
    int rc;
    if ((rc = check_matrix(G, M, ldg, D, "G")) != AM_OK) return rc;
    if ((rc = check_matrix(X, N, ldx, D, "X")) != AM_OK) return rc;
    AM_REQUIRE(theta != nullptr && loglik != nullptr && n_finite != nullptr, AM_ERR_BAD_ARG, "theta, loglik or n_finite is null");
    AM_REQUIRE(adam_m != nullptr && adam_v != nullptr && theta_out != nullptr, AM_ERR_BAD_ARG, "adam_m, adam_v or theta_out is null");
    AM_REQUIRE(step >= 1, AM_ERR_BAD_ARG, "step=%lld must be at least 1 (the first Adam step)", (long long)step);
    AM_REQUIRE(isfinite(lr) && lr >= 0.0, AM_ERR_BAD_ARG, "lr=%g must be finite and not negative", lr);
    // h = 0.5 exp(-theta) multiplies every squared distance in f32: the clamp has to keep it a normal f32 number
    AM_REQUIRE(isfinite(theta_min) && theta_min <= fld::THETA_MAX && 0.5 * exp(-theta_min) <= (double)FLT_MAX, AM_ERR_BAD_ARG,
               "theta_min=%g must be finite and at most %g, with 0.5 exp(-theta_min) a normal float32 number", theta_min,
               fld::THETA_MAX);
    AM_REQUIRE(fld::shape_ok(M, N, D), AM_ERR_BAD_SHAPE, "M=%lld N=%lld: too large for one launch", (long long)M, (long long)N);
    const int nchunks = choose_chunks(M, N);
    Carver c(ws, ws_bytes);
    fld::GradBuffers b;
    fld::carve(c, M, N, nchunks, b);
    AM_REQUIRE(c.ok(), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (am_fld_grad_workspace_bytes), have %zu", c.off, ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = launch_norms(G, M, ldg, D, b.gn, st)) != AM_OK) return rc;
    if ((rc = launch_norms(X, N, ldx, D, b.xn, st)) != AM_OK) return rc;
    hipLaunchKernelGGL(fld::fld_columns_kernel, dim3((unsigned)ceil_div(M, fld::MERGE_THREADS)), dim3(fld::MERGE_THREADS), 0, st, theta,
                       M, 0.5 * (double)D, b.h, b.negc, b.gn);
    AM_LAUNCH_CHECK();
    hipLaunchKernelGGL(fld::fld_lse_columns_kernel, dim3((unsigned)ceil_div(N, fld::MERGE_THREADS)), dim3(fld::MERGE_THREADS), 0, st,
                       loglik, N, fld::mixture_constant(M, D), b.xn, b.lhi, b.llo);
    AM_LAUNCH_CHECK();
    rc = launch_sweep(&fld::fld_grad_kernel<false>, &fld::fld_grad_kernel<true>, fld::GRAD_LDS_BYTES, M, nchunks, D, st, G, M, ldg, b.gn,
                      b.h, b.negc, X, N, ldx, b.xn, b.lhi, b.llo, D, nchunks, b.part_a, b.part_b);
    if (rc != AM_OK) return rc;
    // the bias corrections 1 - beta^step on the host: the pow of the host formula
    const double bc1 = 1.0 - pow(fld::ADAM_B1, (double)step), bc2 = 1.0 - pow(fld::ADAM_B2, (double)step);
    hipLaunchKernelGGL(fld::fld_grad_merge_kernel, dim3((unsigned)ceil_div(M, fld::MERGE_THREADS)), dim3(fld::MERGE_THREADS), 0, st,
                       (const double*)b.part_a, (const double*)b.part_b, M, nchunks, 0.5 * (double)D, n_finite, theta, adam_m, adam_v,
                       bc1, bc2, lr, theta_min, theta_out, out_a, out_b);
    AM_LAUNCH_CHECK();
    return AM_OK;
}
