// Probabilistic scoring rule of a point against a set (Park & Kim, ICCV 2023: probabilistic precision and recall): for
// every row x_i of X against the M rows of Y and ONE radius R of the set Y, without an N x M matrix,
//     psr_i   = 1 - prod_{j : |x_i - y_j| < R} |x_i - y_j| / R             0: no row of Y within R;  1: x_i sits on a row of Y
//     count_i = #{ j : |x_i - y_j| < R }
//
// A sixth epilogue on the exact f32 128 x 128 tile engine, beside the radii (pairwise.hip), the search (knn_search.hip),
// the k-means assign (kmeans.hip), the per-sample scores (sample_scores.hip) and the soft-min (softmin.hip):
// dense_pipeline_early with the production schedule, the (row block) x (column chunk) plan of work_item / choose_chunks,
// the KTAIL instantiation for D % 32 != 0, the f32 norms of launch_norms and the arithmetic of a pair
//     u = fmaf(-2, <x, y>, |x|^2 + |y|^2),  d2 = clamp0(u)       NaN -> +inf; a padded column has |y|^2 = +inf
// - the bits of am_knn_search_f32(squared).
//
// In range: d2 < T, T the smallest float32 >= R * R (the product in f64, formed on the host), so that for a float d2
//     d2 < T  <=>  (double)d2 < R * R                             exactly; NaN and +inf are never in range.
// The tile kernel tests the UNCLAMPED u against T' = (T > 0 ? T : -inf), as sample_scores.hip does: max(u, 0) < T <=> u < T
// for T > 0, nothing is below -inf, and a NaN loses the compare as +inf does.
//
// Factor of a pair in range: f = fminf(fmul_rn(sqrt_rn(d2), (float)(1 / R)), 1) - f32 arithmetic, so that the isotropic
// high-dimensional case, where almost every pair is in range, pays no f64 division per pair.  The sixteen factors a lane
// holds of one 32 x 32 accumulator sub-tile are multiplied in f32 (a product that underflows to 0 moves psr by less than
// 1e-37); everything beyond - sub-tiles, tiles, the four lanes of a row, the chunks - is an f64 running product joined in
// a fixed order (lane slot order, then chunk order).  The compare and the count run on every pair; the square roots only
// in a sub-tile in which some lane's count moved (__any over the wave): on clustered data in-range pairs are as rare as
// PRDC memberships and the epilogue is a compare.
//
// The four (product, count) pairs of a row (2 half-waves x 2 column-half waves) meet in LDS, the chunks' partials
// ([nchunks][N] double, int32) in psr_merge_kernel, which also forms the block sums of psr and count in a fixed tree;
// psr_sums_kernel adds those.  No floating-point atomics: two calls at the same shapes return the same bits.  Unlike the
// key-based epilogues the product's last bits DEPEND ON THE CHUNK PLAN (the grouping of an f64 product); the counts do not.
//
// Register budget: 64 accumulators, 64 staging registers, 32 fragment registers, 4 product registers and 2 counts;
// __launch_bounds__(256, 2), two workgroups per CU, no scratch (tests/test_psr_resources_cpu.py).
#include "row_sweep.h"
#include <float.h>
#include <math.h>

namespace am {
namespace psr {

constexpr size_t LDS_BYTES = (ENGINE_LDS_FLOATS + 2 * TB) * sizeof(float);       // staging slabs + [2][128] column norms
constexpr int MERGE_THREADS = 256;

struct PsrEpilogue : ColumnAux<PAD_INF> {               // |y_j|^2 of the tile (+inf past the end)
    float thr;                           // T' : T, or -inf when T == 0
    float inv;                           // (float)(1 / R)
    float xn[2];
    double prod[2];
    int cnt[2];

    __device__ __forceinline__ PsrEpilogue(const LaneInfo& l) : ColumnAux<PAD_INF>(l) {}

    __device__ __forceinline__ void finish(int t, int64_t, f32x16 (&acc)[2][2]) {
        const float* a = tile(t);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            f32x4 yn[4];
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) yn[g4] = *reinterpret_cast<const f32x4*>(a + mt * 32 + g4 * 8);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const int c0 = cnt[nt];
                int c = c0;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg)
                    c += fmaf(-2.f, acc[mt][nt][reg], xn[nt] + yn[reg >> 2][reg & 3]) < thr ? 1 : 0;
                cnt[nt] = c;
                // rare on clustered data: some lane of the wave has a pair in range in this 32 x 32 sub-tile
                if (__any(c != c0)) {
                    float p = 1.f;
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const float u = fmaf(-2.f, acc[mt][nt][reg], xn[nt] + yn[reg >> 2][reg & 3]);
                        const float f = fminf(__fmul_rn(sqrt_rn(clamp0(u)), inv), 1.f);
                        p *= u < thr ? f : 1.f;
                        if ((reg & 3) == 3) __builtin_amdgcn_sched_barrier(0);           // four square roots at a time
                    }
                    prod[nt] *= (double)p;
                }
            }
        }
    }
};

// pprod / pcnt [chunk * N + row] = the row's product of factors and count inside column chunk `chunk`
template <bool KTAIL>
__global__ void __launch_bounds__(ENGINE_THREADS, 2)
psr_kernel(const float* __restrict__ X, int64_t N, int64_t ldx, const float* __restrict__ xnorm, const float* __restrict__ Y,
           int64_t M, int64_t ldy, const float* __restrict__ ynorm, int D, int nchunks, float thr, float inv,
           double* __restrict__ pprod, int* __restrict__ pcnt) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LaneInfo L;
    const WorkItem w = work_item((M + TB - 1) / TB, nchunks);
    const int chunk = blockIdx.x % nchunks;            // the chunk work_item gave this workgroup: its slice of the partials

    PsrEpilogue epi(L);
    epi.src[0] = ynorm;
    epi.nc = M;
    epi.lds = lds + ENGINE_LDS_FLOATS;
    epi.thr = thr;
    epi.inv = inv;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        epi.xn[nt] = row_norm(xnorm, w.prow0, N, L, nt);
        epi.prod[nt] = 1.0;
        epi.cnt[nt] = 0;
    }
    dense_pipeline_early<EV_DEFAULT, KTAIL>(Y, M, ldy, LinearTiles{w.qtile0}, X, N, ldx, w.prow0, w.ntiles, D, lds, L, epi);

    // a row is covered by 4 lanes (2 half-waves x 2 column-half waves): [128][4] products, then [128][4] counts, through
    // the staging slabs, free now; joined in slot order
    double* mgp = reinterpret_cast<double*>(lds);
    int* mgc = reinterpret_cast<int*>(mgp + TB * 4);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int slot = join_slot(L, nt);
        mgp[slot] = epi.prod[nt];
        mgc[slot] = epi.cnt[nt];
    }
    __syncthreads();
    if (L.tid < TB) {
        const int64_t i = joined_row(w.prow0, L.tid);
        if (i < N) {
            double p = mgp[L.tid * 4];
            int c = mgc[L.tid * 4];
#pragma unroll
            for (int s = 1; s < 4; ++s) {
                p *= mgp[L.tid * 4 + s];
                c += mgc[L.tid * 4 + s];
            }
            pprod[(int64_t)chunk * N + i] = p;
            pcnt[(int64_t)chunk * N + i] = c;
        }
    }
}

// the chunks' partials of a row in chunk order -> psr and count; block_sums[2 * block + {0, 1}] = the block's sums of both
// (block_sums == NULL: no sums were asked for)
__global__ void __launch_bounds__(MERGE_THREADS)
psr_merge_kernel(const double* __restrict__ pprod, const int* __restrict__ pcnt, int64_t N, int nchunks,
                 double* __restrict__ out_psr, int32_t* __restrict__ out_count, double* __restrict__ block_sums) {
    __shared__ double red[MERGE_THREADS];
    const int64_t i = (int64_t)blockIdx.x * MERGE_THREADS + threadIdx.x;
    double v = 0.0, cv = 0.0;
    if (i < N) {
        double p = pprod[i];
        int c = pcnt[i];
        for (int ch = 1; ch < nchunks; ++ch) {
            p *= pprod[(int64_t)ch * N + i];
            c += pcnt[(int64_t)ch * N + i];
        }
        v = 1.0 - p;
        cv = (double)c;
        out_psr[i] = v;
        out_count[i] = c;
    }
    if (block_sums == nullptr) return;                 // (uniform over the grid)
    const double sv = block_reduce_256<SumOp>(v, red);
    __syncthreads();
    const double sc = block_reduce_256<SumOp>(cv, red);          // integers below 2^53: exact
    if (threadIdx.x == 0) {
        block_sums[2 * (int64_t)blockIdx.x] = sv;
        block_sums[2 * (int64_t)blockIdx.x + 1] = sc;
    }
}

__global__ void __launch_bounds__(MERGE_THREADS)
psr_sums_kernel(const double* __restrict__ block_sums, int64_t nblocks, double* __restrict__ out_sums) {
    __shared__ double red[MERGE_THREADS];
    double v = 0.0, cv = 0.0;
    for (int64_t j = threadIdx.x; j < nblocks; j += MERGE_THREADS) {
        v += block_sums[2 * j];
        cv += block_sums[2 * j + 1];
    }
    const double sv = block_reduce_256<SumOp>(v, red);
    __syncthreads();
    const double sc = block_reduce_256<SumOp>(cv, red);
    if (threadIdx.x == 0) {
        out_sums[0] = sv;
        out_sums[1] = sc;
    }
}

static bool shape_ok(int64_t N, int64_t M, int D) { return sweep_shape_ok(N, M, D, COLUMNS_KEYED); }   // as am_sample_scores_f32

struct Buffers {
    float *xn, *yn;
    double *pprod, *block_sums;
    int* pcnt;
};
static void carve(Carver& c, int64_t N, int64_t M, int nchunks, Buffers& b) {
    b.xn = c.take<float>((size_t)N);
    b.yn = c.take<float>((size_t)M);
    b.pprod = c.take<double>((size_t)nchunks * (size_t)N);
    b.block_sums = c.take<double>(2 * (size_t)ceil_div(N, MERGE_THREADS));
    b.pcnt = c.take<int>((size_t)nchunks * (size_t)N);
}

}  // namespace psr
}  // namespace am

using namespace am;

extern "C" size_t am_psr_workspace_bytes(int64_t N, int64_t M, int D) {
    if (!psr::shape_ok(N, M, D)) return 0;
    Carver c(nullptr, 0);
    psr::Buffers b;
    psr::carve(c, N, M, choose_chunks(N, M), b);
    return c.off;
}

extern "C" int am_psr_chunks(int64_t N, int64_t M, int D) { return psr::shape_ok(N, M, D) ? choose_chunks(N, M) : 0; }

extern "C" int am_psr_f32(const float* X, int64_t N, int64_t ldx, const float* Y, int64_t M, int64_t ldy, int D, double radius,
                          double* out_psr, int32_t* out_count, double* out_sums, void* ws, size_t ws_bytes, am_stream_t stream) {
    int rc;
    if ((rc = check_matrix(X, N, ldx, D, "X")) != AM_OK) return rc;
    if ((rc = check_matrix(Y, M, ldy, D, "Y")) != AM_OK) return rc;
    AM_REQUIRE(out_psr != nullptr && out_count != nullptr, AM_ERR_BAD_ARG, "%s is null", out_psr == nullptr ? "out_psr" : "out_count");
    AM_REQUIRE(isfinite(radius) && radius > 0.0 && radius * radius <= (double)FLT_MAX, AM_ERR_BAD_ARG,
               "radius=%g must be finite and > 0, with radius^2 a finite float32 number", radius);
    AM_REQUIRE(psr::shape_ok(N, M, D), AM_ERR_BAD_SHAPE, "N=%lld M=%lld: too large for one launch (M < 2^32 - 1)", (long long)N,
               (long long)M);
    const int nchunks = choose_chunks(N, M);
    Carver c(ws, ws_bytes);
    psr::Buffers b;
    psr::carve(c, N, M, nchunks, b);
    AM_REQUIRE(c.ok(), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (am_psr_workspace_bytes), have %zu", c.off, ws_bytes);
    // T = the smallest float32 >= radius^2: for a float d2, d2 < T <=> (double)d2 < radius^2
    const double r2 = radius * radius;
    float T = (float)r2;
    if ((double)T < r2) T = nextafterf(T, INFINITY);
    const float thr = T > 0.f ? T : -INFINITY;
    // (a radius below 1 / FLT_MAX: only d2 == 0 is in range, and 0 * FLT_MAX is the factor 0 that 0 * inf would not be)
    const float inv = 1.0 / radius > (double)FLT_MAX ? FLT_MAX : (float)(1.0 / radius);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float* yn;
    if ((rc = launch_norms_pair(X, N, ldx, Y, M, ldy, D, b.xn, b.yn, st, &yn)) != AM_OK) return rc;
    rc = launch_sweep(&psr::psr_kernel<false>, &psr::psr_kernel<true>, psr::LDS_BYTES, N, nchunks, D, st, X, N, ldx, b.xn, Y, M, ldy, yn,
                      D, nchunks, thr, inv, b.pprod, b.pcnt);
    if (rc != AM_OK) return rc;
    const int64_t nblocks = ceil_div(N, psr::MERGE_THREADS);
    hipLaunchKernelGGL(psr::psr_merge_kernel, dim3((unsigned)nblocks), dim3(psr::MERGE_THREADS), 0, st, (const double*)b.pprod,
                       (const int*)b.pcnt, N, nchunks, out_psr, out_count, out_sums != nullptr ? b.block_sums : (double*)nullptr);
    AM_LAUNCH_CHECK();
    if (out_sums != nullptr) {
        hipLaunchKernelGGL(psr::psr_sums_kernel, dim3(1), dim3(psr::MERGE_THREADS), 0, st, (const double*)b.block_sums, nblocks,
                           out_sums);
        AM_LAUNCH_CHECK();
    }
    return AM_OK;
}
