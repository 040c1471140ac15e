// Soft-min on the f32 tile engine: one log-domain Sinkhorn half-step, without an N x M cost matrix.
//
// am_softmin_f32: for every row x_i of X against the M rows of Y, potentials g on the columns and a temperature eps > 0
//     T_i = -eps log( (1 / M) sum_j exp( (g_j - C(x_i, y_j)) / eps ) ),        C = d2 / 2
// with the arithmetic of a pair that the search and the k-means assign use,
//     d2 = max(fmaf(-2, <x, y>, |x|^2 + |y|^2), 0)       NaN -> +inf (clamp0); a padded column has |y|^2 = +inf
// on the same sweep (dense_pipeline_early with the production schedule, the (row block) x (column chunk) plan of work_item /
// choose_chunks, the KTAIL instantiation for D % 32 != 0, the f32 norms of launch_norms).  kmeans.hip is the hard-min form:
// there a lane keeps one 64-bit key per row, here a running (max, sum) pair - the online log-sum-exp:
//     z  = fmaf(-d2, (float)(0.5 / eps), (float)(g_j / eps))          f32, from the f32 d2 bits
//     mx = max z so far (f32),   s = sum exp(z - mx) (f64; exp in f64 as the kernel sums of kad.hip)
// and s is rescaled by exp(mx_old - mx_new) when the maximum rises: at most one more exp per accumulator tile of 16 values.
// The weight 1 / M is not folded into z - eps log M is added once, in f64, at the end: inside the f32 z it would cost
// eps log M 2^-24 at the large temperatures of the first steps of an eps-scaling schedule.  A column at distance +inf (a
// padded one, a NaN distance) has z = -inf and contributes exactly 0.
//
// The four pairs of a row (2 half-waves x 2 column-half waves) meet in LDS, the chunks' pairs in softmin_merge_kernel, both
// in a fixed order with (mx, s) + (mx', s') = (m, s exp(mx - m) + s' exp(mx' - m)), m = max(mx, mx').  The merge kernel also
// does the bookkeeping of a Sinkhorn step, so that a step reads nothing back:
//     out_i = damping prev_i + (1 - damping) T_i                       (damping == 0: out_i = T_i, prev is not read for it)
//     stats[0] = max_i |out_i - prev_i|  (prev == NULL: |out_i|),   stats[1] = max_i |out_i|
// the maxima as integer maxima over the bit patterns of the non-negative doubles.  No floating-point atomics anywhere:
// every call returns the same bits.
//
// Register budget: the assign's (64 accumulators, 64 staging registers, 32 fragment registers) with 6 registers of state
// per lane - mx and s for two rows - in place of its 4 key registers; __launch_bounds__(256, 2), two workgroups per CU.
#include "row_sweep.h"
#include <float.h>
#include <math.h>

namespace am {
namespace softmin {

constexpr size_t LDS_BYTES = (ENGINE_LDS_FLOATS + 2 * 2 * TB) * sizeof(float);   // staging slabs + [2][2][128]: |y_j|^2, g_j / eps
constexpr int MERGE_THREADS = 256;

struct SoftminEpilogue {
    const float* ynorm;
    const float* ge;                     // g_j / eps, rounded to f32 (softmin_columns_kernel)
    int64_t nc;
    float* aux;                          // LDS [2][2][128] : |y_j|^2 of the tile (+inf past nc), then g_j / eps (0 past nc)
    float hie;                           // 0.5 / eps
    float xn[2];
    float mx[2];
    double s[2];
    float aux_n, aux_g;
    const LaneInfo& L;

    __device__ __forceinline__ SoftminEpilogue(const LaneInfo& l) : L(l) {}
    __device__ __forceinline__ void aux_issue(int, int64_t qtile) {
        if (L.tid < TB) {
            const int64_t j = qtile * TB + L.tid;
            aux_n = j < nc ? ynorm[j] : INFINITY;
            aux_g = j < nc ? ge[j] : 0.f;
        }
    }
    __device__ __forceinline__ void aux_commit(int t) {
        if (L.tid < TB) {
            aux[(t & 1) * 2 * TB + L.tid] = aux_n;
            aux[(t & 1) * 2 * TB + TB + L.tid] = aux_g;
        }
    }
    __device__ __forceinline__ float z_of(float a, float norms, float g) const {
        return fmaf(-clamp0(fmaf(-2.f, a, norms)), hie, g);          // d2 = +inf -> -inf (hie is a positive normal number)
    }

    __device__ __forceinline__ void finish(int t, int64_t, f32x16 (&acc)[2][2]) {
        const float* a = aux + (t & 1) * 2 * TB + L.wm * 64 + L.h * 4;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            f32x4 yn[4], gq[4];
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                yn[g4] = *reinterpret_cast<const f32x4*>(a + mt * 32 + g4 * 8);
                gq[g4] = *reinterpret_cast<const f32x4*>(a + TB + mt * 32 + g4 * 8);
            }
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                float tmax = -INFINITY;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg)
                    tmax = fmaxf(tmax, z_of(acc[mt][nt][reg], xn[nt] + yn[reg >> 2][reg & 3], gq[reg >> 2][reg & 3]));
                const double ref = lse_raise(mx[nt], s[nt], tmax);
                double sum = s[nt];
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const float z = z_of(acc[mt][nt][reg], xn[nt] + yn[reg >> 2][reg & 3], gq[reg >> 2][reg & 3]);
                    sum += exp((double)z - ref);
                    if ((reg & 3) == 3) __builtin_amdgcn_sched_barrier(0);               // four exp chains at a time: more in flight spill
                }
                s[nt] = sum;
            }
        }
    }
};

// ge[j] = (float)(g_j / eps); g == NULL: zero potentials
__global__ void __launch_bounds__(MERGE_THREADS)
softmin_columns_kernel(const double* __restrict__ g, int64_t M, double eps, float* __restrict__ ge) {
    const int64_t j = (int64_t)blockIdx.x * MERGE_THREADS + threadIdx.x;
    if (j < M) ge[j] = g != nullptr ? (float)(g[j] / eps) : 0.f;
}

// part_mx / part_s[chunk * N + row] = the (max, sum) pair of `row` inside column chunk `chunk`
template <bool KTAIL>
__global__ void __launch_bounds__(ENGINE_THREADS, 2)
softmin_kernel(const float* __restrict__ X, int64_t N, int64_t ldx, const float* __restrict__ xnorm, const float* __restrict__ Y,
               int64_t M, int64_t ldy, const float* __restrict__ ynorm, const float* __restrict__ ge, int D, int nchunks, float hie,
               float* __restrict__ part_mx, double* __restrict__ part_s) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LaneInfo L;
    const WorkItem w = work_item((M + TB - 1) / TB, nchunks);
    const int chunk = blockIdx.x % nchunks;            // the chunk work_item gave this workgroup: its slice of the partials

    SoftminEpilogue epi(L);
    epi.ynorm = ynorm;
    epi.ge = ge;
    epi.nc = M;
    epi.aux = lds + ENGINE_LDS_FLOATS;
    epi.hie = hie;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        epi.xn[nt] = row_norm(xnorm, w.prow0, N, L, nt);
        epi.mx[nt] = -INFINITY;
        epi.s[nt] = 0.0;
    }
    dense_pipeline_early<EV_DEFAULT, KTAIL>(Y, M, ldy, LinearTiles{w.qtile0}, X, N, ldx, w.prow0, w.ntiles, D, lds, L, epi);

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

// largest value of the workgroup (non-negative doubles or NaN, as bit patterns): a fixed tree
__device__ __forceinline__ unsigned long long block_max_256(unsigned long long v, unsigned long long* s) {
    s[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int w = MERGE_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] = s[threadIdx.x + w] > s[threadIdx.x] ? s[threadIdx.x + w] : s[threadIdx.x];
        __syncthreads();
    }
    return s[0];
}

// the chunks' pairs of a row in chunk order -> T_i -> out_i, and the two maxima of the step (stats zeroed before the launch)
__global__ void __launch_bounds__(MERGE_THREADS)
softmin_merge_kernel(const float* __restrict__ part_mx, const double* __restrict__ part_s, int64_t N, int nchunks, double eps,
                     double eps_log_m, const double* prev, double damping, double* out,
                     unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long red[MERGE_THREADS];
    const int64_t i = (int64_t)blockIdx.x * MERGE_THREADS + threadIdx.x;
    unsigned long long change = 0ull, magnitude = 0ull;
    if (i < N) {
        float m = part_mx[i];
        double s = part_s[i];
        for (int c = 1; c < nchunks; ++c) lse_join(m, s, part_mx[(int64_t)c * N + i], part_s[(int64_t)c * N + i]);
        const double t = eps_log_m - eps * ((double)m + log(s));
        const double p = prev != nullptr ? prev[i] : 0.0;
        const double o = damping != 0.0 ? damping * p + (1.0 - damping) * t : t;
        out[i] = o;
        change = (unsigned long long)__double_as_longlong(fabs(o - p));
        magnitude = (unsigned long long)__double_as_longlong(fabs(o));
    }
    if (stats == nullptr) return;                      // (uniform over the grid)
    const unsigned long long c = block_max_256(change, red);
    __syncthreads();
    const unsigned long long g = block_max_256(magnitude, red);
    if (threadIdx.x == 0) {
        atomicMax(stats, c);
        atomicMax(stats + 1, g);
    }
}

static bool shape_ok(int64_t N, int64_t M, int D) { return sweep_shape_ok(N, M, D, COLUMNS_TILED); }

struct Buffers {
    float *xn, *yn, *ge, *part_mx;
    double* part_s;
};
static void carve(Carver& c, int64_t N, int64_t M, int nchunks, Buffers& b) {
    b.xn = c.take<float>((size_t)N);
    b.yn = c.take<float>((size_t)M);
    b.ge = c.take<float>((size_t)M);
    b.part_mx = c.take<float>((size_t)nchunks * (size_t)N);
    b.part_s = c.take<double>((size_t)nchunks * (size_t)N);
}

}  // namespace softmin
}  // namespace am

using namespace am;

extern "C" size_t am_softmin_workspace_bytes(int64_t N, int64_t M, int D) {
    if (!softmin::shape_ok(N, M, D)) return 0;
    Carver c(nullptr, 0);
    softmin::Buffers b;
    softmin::carve(c, N, M, choose_chunks(N, M), b);
    return c.off;
}

extern "C" int am_softmin_f32(const float* X, int64_t N, int64_t ldx, const float* Y, int64_t M, int64_t ldy, int D, const double* g,
                              double eps, const double* prev, double damping, double* out, double* stats, void* ws, size_t ws_bytes,
                              am_stream_t stream) {
    int rc;
    if ((rc = check_matrix(X, N, ldx, D, "X")) != AM_OK) return rc;
    if ((rc = check_matrix(Y, M, ldy, D, "Y")) != AM_OK) return rc;
    AM_REQUIRE(out != nullptr, AM_ERR_BAD_ARG, "out is null");
    // 0.5 / eps multiplies every squared distance in f32: it has to be a normal f32 number
    AM_REQUIRE(isfinite(eps) && eps > 0.0 && 0.5 / eps <= (double)FLT_MAX && 0.5 / eps >= (double)FLT_MIN, AM_ERR_BAD_ARG,
               "eps=%g must be finite and > 0, with 0.5 / eps a normal float32 number", eps);
    AM_REQUIRE(damping >= 0.0 && damping < 1.0, AM_ERR_BAD_ARG, "damping=%g must lie in [0, 1)", damping);
    AM_REQUIRE(damping == 0.0 || prev != nullptr, AM_ERR_BAD_ARG, "damping=%g needs prev, which is null", damping);
    AM_REQUIRE(softmin::shape_ok(N, M, D), AM_ERR_BAD_SHAPE, "N=%lld M=%lld: too large for one launch", (long long)N, (long long)M);
    const int nchunks = choose_chunks(N, M);
    Carver c(ws, ws_bytes);
    softmin::Buffers b;
    softmin::carve(c, N, M, nchunks, b);
    AM_REQUIRE(c.ok(), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (am_softmin_workspace_bytes), have %zu", c.off, ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float* yn;
    if ((rc = launch_norms_pair(X, N, ldx, Y, M, ldy, D, b.xn, b.yn, st, &yn)) != AM_OK) return rc;
    hipLaunchKernelGGL(softmin::softmin_columns_kernel, dim3((unsigned)ceil_div(M, softmin::MERGE_THREADS)),
                       dim3(softmin::MERGE_THREADS), 0, st, g, M, eps, b.ge);
    AM_LAUNCH_CHECK();
    rc = launch_sweep(&softmin::softmin_kernel<false>, &softmin::softmin_kernel<true>, softmin::LDS_BYTES, N, nchunks, D, st, X, N, ldx,
                      b.xn, Y, M, ldy, yn, b.ge, D, nchunks, (float)(0.5 / eps), b.part_mx, b.part_s);
    if (rc != AM_OK) return rc;
    if (stats != nullptr) AM_HIP_TRY(hipMemsetAsync(stats, 0, 2 * sizeof(double), st));
    hipLaunchKernelGGL(softmin::softmin_merge_kernel, dim3((unsigned)ceil_div(N, softmin::MERGE_THREADS)), dim3(softmin::MERGE_THREADS),
                       0, st, (const float*)b.part_mx, (const double*)b.part_s, N, nchunks, eps, eps * log((double)M), prev, damping, out,
                       reinterpret_cast<unsigned long long*>(stats));
    AM_LAUNCH_CHECK();
    return AM_OK;
}
