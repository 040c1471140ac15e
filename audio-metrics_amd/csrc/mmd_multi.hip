// Whole-set kernel sums of the unbiased MMD^2 under several kernels at once: one Gram pass, one epilogue value per scale.
//
// am_mmd_rbf_f32 (kad.hip) redoes the tile work of the three blocks for every bandwidth; only its epilogue depends on the
// bandwidth.  am_mmd_multi_f32 keeps the accumulator tile and evaluates up to AM_MMD_MULTI_MAX kernels on it:
//   Gaussian   exp(-d2 g_s),        g_s = 0.5 / (bw2 (c_s c_s))
//   Laplacian  exp(-sqrt(d2) h_s),  h_s = 1 / (c_s sqrt(bw2))
//   energy     -sqrt(d2)            (one "scale", no bandwidth: the MMD of k = -d is the energy distance)
// with d2 = max((|a|^2 + |b|^2) - 2 dot(a, b), 0) in f64, f64 squared norms and the f32 matrix-core dot product - the
// arithmetic, tile engine, grid plan (mmd_plan), workspace carve and summation order of kad_mmd_kernel.  Every scale keeps its
// own running sum, added in the order MmdEpilogue adds its one: the Gaussian sums of scale c equal those of am_mmd_rbf_f32 at
// gamma = g bit for bit, and no scale's sums depend on which other scales share the call.
//
// Padded rows: the Gaussian and Laplacian kernels give them a norm of +inf, exp(-inf) = 0 exactly.  The energy kernel would
// add -inf, so it gives them a norm of 0 and drops the pair by index.
//
// Registers (two workgroups of four waves per CU, 256 per lane, 64 of them accumulators), without / with the inner-dimension
// tail: one to four Gaussian scales take 234 / 236, 244 / 245, 248 / 249, 252 / 254; one to four Laplacian scales 240, 249,
// 255, 256 either way; the energy kernel 206 / 208; none with scratch memory (tests/test_mmd_multi_cpu.py).  Four Laplacian
// scales fill the file - hence AM_MMD_MULTI_MAX = 4; a longer grid is several calls.
#include "am_common.h"
#include "kad_common.h"
#include "pairwise_common.h"

namespace am {

constexpr size_t MMD_MULTI_LDS_BYTES = ENGINE_LDS_FLOATS * sizeof(float);

struct MultiScales {
    double c[AM_MMD_MULTI_MAX];
};

template <int KIND, int S>
struct MultiEpilogue {
    const double* qn;            // f64 squared norms of the Q rows
    int64_t nq, np, ptile;
    double par[S];               // g_s (Gaussian) / h_s (Laplacian)
    bool sym;                    // Q and P are the same set: tile (tq, tp), tq < tp, stands for its mirror image too
    double sum[S];
    double pnorm[2];             // padded rows: +inf (exp(-inf) = 0), or 0 and pok = false (energy)
    bool pok[2];
    const LaneInfo& L;
    __device__ __forceinline__ MultiEpilogue(const LaneInfo& l) : L(l) {}
    __device__ __forceinline__ void aux_issue(int, int64_t) {}
    __device__ __forceinline__ void aux_commit(int) {}
    // (rows are indexed in 32 bits: N * ld * 4 < 4 GiB and ld >= 4 put N below 2^28)
    __device__ __forceinline__ void finish(int, int64_t qtile, f32x16 (&acc)[2][2]) {
        const bool diag = sym && qtile == ptile;
        const int q0 = (int)qtile * TB + L.wm * 64 + 4 * L.h, p0 = (int)ptile * TB + L.wn * 64 + L.r;
        double s[S];
#pragma unroll
        for (int j = 0; j < S; ++j) s[j] = 0.0;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int q = q0 + mt * 32 + (i & 3) + 8 * (i >> 2);
                const bool qok = q < (int)nq;
                const double qnorm = qok ? qn[q] : (KIND == AM_MMD_ENERGY ? 0.0 : (double)INFINITY);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    double d2 = (qnorm + pnorm[nt]) - 2.0 * (double)acc[mt][nt][i];
                    d2 = d2 < 0.0 ? 0.0 : d2;
                    const bool drop = diag && p0 + nt * 32 == q;
                    if constexpr (KIND == AM_MMD_GAUSSIAN) {
#pragma unroll
                        for (int j = 0; j < S; ++j) {
                            const double k = exp(-d2 * par[j]);
                            s[j] += drop ? 0.0 : k;
                        }
                    } else if constexpr (KIND == AM_MMD_LAPLACIAN) {
                        const double d = sqrt(d2);
#pragma unroll
                        for (int j = 0; j < S; ++j) {
                            const double k = exp(-d * par[j]);
                            s[j] += drop ? 0.0 : k;
                        }
                    } else {
                        const double k = -sqrt(d2);
                        s[0] += (drop || !qok || !pok[nt]) ? 0.0 : k;
                    }
                    if (S > 2) __builtin_amdgcn_sched_barrier(0);       // at most four exp chains at a time: more in flight spill
                }
                if (S == 2 || (i & 1) == 1) __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
        for (int j = 0; j < S; ++j) sum[j] += (sym && !diag) ? 2.0 * s[j] : s[j];
    }
};

// grid: x = P tile, y = chunk of Q tiles (the plan of kad_mmd_kernel); partial[j * slots + y * gridDim.x + x] = this
// workgroup's weighted sum of scale j (0 for an empty chunk)
template <int KIND, int S, bool KTAIL>
__global__ void __launch_bounds__(ENGINE_THREADS, 2)
mmd_multi_kernel(const float* __restrict__ Q, int64_t nq, int64_t ldq, const double* __restrict__ qn, const float* __restrict__ P,
                 int64_t np, int64_t ldp, const double* __restrict__ pn, int D, int sym, int chunk_tiles,
                 const float* __restrict__ bw2_dev, double bw2, MultiScales sc, double* __restrict__ partial, int64_t slots) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LaneInfo L;
    const int64_t TQ = (nq + TB - 1) / TB, TP = (np + TB - 1) / TB;
    const int64_t tp = sym ? TP - 1 - (int64_t)blockIdx.x : (int64_t)blockIdx.x;
    const int64_t q0 = (int64_t)blockIdx.y * chunk_tiles;
    const int64_t qlast = sym ? tp : TQ - 1;
    const int64_t slot = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (q0 > qlast) {
        if (L.tid < S) partial[L.tid * slots + slot] = 0.0;
        return;
    }
    const int64_t left = qlast + 1 - q0;
    const int ntiles = left < chunk_tiles ? (int)left : chunk_tiles;
    MultiEpilogue<KIND, S> epi(L);
    epi.qn = qn;
    epi.nq = nq;
    epi.np = np;
    epi.ptile = tp;
    epi.sym = sym != 0;
    if (bw2_dev != nullptr) bw2 = (double)*bw2_dev;                        // the median feeds the sums without a host round trip
#pragma unroll
    for (int j = 0; j < S; ++j) {
        const double c = sc.c[j];
        epi.par[j] = KIND == AM_MMD_GAUSSIAN ? 0.5 / (bw2 * (c * c)) : KIND == AM_MMD_LAPLACIAN ? 1.0 / (c * sqrt(bw2)) : 0.0;
        epi.sum[j] = 0.0;
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int64_t p = tp * TB + L.wn * 64 + nt * 32 + L.r;
        epi.pok[nt] = p < np;
        epi.pnorm[nt] = p < np ? pn[p] : (KIND == AM_MMD_ENERGY ? 0.0 : (double)INFINITY);
    }
    dense_pipeline_early<EV_DEFAULT, KTAIL>(Q, nq, ldq, LinearTiles{q0}, P, np, ldp, tp * TB, ntiles, D, lds, L, epi);
    double* red = reinterpret_cast<double*>(lds);          // staging slabs are idle after the pipeline's last barrier
#pragma unroll
    for (int j = 0; j < S; ++j) {
        double v = epi.sum[j];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        if (L.lane == 0) red[j * 4 + (L.tid >> 6)] = v;
    }
    __syncthreads();
    if (L.tid < S) {
        const double* r = red + L.tid * 4;
        partial[L.tid * slots + slot] = ((r[0] + r[1]) + r[2]) + r[3];
    }
}

// out[j] = sum of partial[j * count .. (j + 1) * count) for workgroup j, in a fixed order: strided per-thread sums, then a
// tree.  The one reduce kernel of the family (launch_mmd_reduce): am_mmd_rbf_f32 and am_mmd_rbf_f64 use it with one output.
__global__ void __launch_bounds__(256) mmd_multi_reduce_kernel(const double* __restrict__ partial, int64_t count,
                                                               double* __restrict__ out) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const double* mine = partial + (int64_t)blockIdx.x * count;
    double s = 0.0;
    for (int64_t i = tid; i < count; i += 256) s += mine[i];
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = red[0];
}

int launch_mmd_reduce(const double* partial, int64_t count, int nout, double* out, hipStream_t st) {
    hipLaunchKernelGGL(mmd_multi_reduce_kernel, dim3((unsigned)nout), dim3(256), 0, st, partial, count, out);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

struct MultiCall {
    const float *X, *Y;
    int64_t N1, N2, ldx, ldy;
    int D;
    const float* bw2_dev;
    double bw2;
    MultiScales sc;
    int nscales;
    unsigned blocks;
    double* out_sums;
    MmdPlan plan;
    MmdWs w;
    hipStream_t st;
};

template <int KIND, int S, bool KTAIL>
static int launch_blocks(const MultiCall& c) {
    auto kernel = &mmd_multi_kernel<KIND, S, KTAIL>;
    AM_HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), (int)MMD_MULTI_LDS_BYTES));
    for (int b = 0; b < 3; ++b) {
        if (!(c.blocks & (1u << b))) continue;
        const bool q_is_y = b == 1, p_is_x = b == 0;
        hipLaunchKernelGGL(kernel, c.plan.grid[b], dim3(ENGINE_THREADS), MMD_MULTI_LDS_BYTES, c.st,
                           q_is_y ? c.Y : c.X, q_is_y ? c.N2 : c.N1, q_is_y ? c.ldy : c.ldx, (const double*)(q_is_y ? c.w.n.n2 : c.w.n.n1),
                           p_is_x ? c.X : c.Y, p_is_x ? c.N1 : c.N2, p_is_x ? c.ldx : c.ldy, (const double*)(p_is_x ? c.w.n.n1 : c.w.n.n2),
                           c.D, b < 2 ? 1 : 0, c.plan.chunk[b], c.bw2_dev, c.bw2, c.sc, c.w.partial[b], (int64_t)c.plan.slots[b]);
        AM_LAUNCH_CHECK();
        const int rc = launch_mmd_reduce(c.w.partial[b], (int64_t)c.plan.slots[b], S, c.out_sums + (size_t)b * S, c.st);
        if (rc != AM_OK) return rc;
    }
    return AM_OK;
}

template <int KIND, int S>
static int launch_tail(const MultiCall& c) {
    return (c.D % BK) != 0 ? launch_blocks<KIND, S, true>(c) : launch_blocks<KIND, S, false>(c);
}

template <int KIND>
static int launch_scales(const MultiCall& c) {
    switch (c.nscales) {
        case 1: return launch_tail<KIND, 1>(c);
        case 2: return launch_tail<KIND, 2>(c);
        case 3: return launch_tail<KIND, 3>(c);
        default: return launch_tail<KIND, 4>(c);
    }
}

static bool finite_positive(double v) { return v > 0.0 && v < (double)INFINITY; }

// the part of a call every kernel shares: plan and workspace (`query` names the caller's own size query), then the norms
static int open_call(MultiCall& c, const float* X, int64_t N1, int64_t ldx, const float* Y, int64_t N2, int64_t ldy, int D, int nscales,
                     unsigned blocks, double* out_sums, void* ws, size_t ws_bytes, const char* query, am_stream_t stream) {
    c.plan = mmd_plan(N1, N2, TB);
    c.w = mmd_carve(ws, ws_bytes, N1, N2, nscales, blocks, c.plan);
    AM_REQUIRE(c.w.ok, AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (%s), have %zu", c.w.bytes, query, ws_bytes);
    c.X = X, c.Y = Y, c.N1 = N1, c.N2 = N2, c.ldx = ldx, c.ldy = ldy, c.D = D;
    c.nscales = nscales, c.blocks = blocks, c.out_sums = out_sums;
    c.st = static_cast<hipStream_t>(stream);
    return launch_set_norms(X, N1, ldx, Y, N2, ldy, D, c.w.n, c.st);
}

}  // namespace am

using namespace am;

extern "C" size_t am_mmd_multi_workspace_bytes(int64_t N1, int64_t N2, int D, int nscales, unsigned blocks) {
    if (N1 < 1 || N2 < 1 || D < 1 || nscales < 1 || nscales > AM_MMD_MULTI_MAX || (blocks & 7u) == 0) return 0;
    return mmd_carve(nullptr, 0, N1, N2, nscales, blocks & 7u, mmd_plan(N1, N2, TB)).bytes;
}

extern "C" int am_mmd_multi_f32(const float* X, int64_t N1, int64_t ldx, const float* Y, int64_t N2, int64_t ldy, int D, int kernel,
                                const float* bw2_dev, double bw2, const double* scales, int nscales, unsigned blocks,
                                double* out_sums, void* ws, size_t ws_bytes, am_stream_t stream) {
    AM_REQUIRE(out_sums && scales, AM_ERR_BAD_ARG, "null pointer");
    AM_REQUIRE(kernel == AM_MMD_GAUSSIAN || kernel == AM_MMD_LAPLACIAN || kernel == AM_MMD_ENERGY, AM_ERR_BAD_ARG,
               "kernel = %d is not one of AM_MMD_GAUSSIAN, AM_MMD_LAPLACIAN, AM_MMD_ENERGY", kernel);
    int rc = check_two_sets_f32(X, N1, ldx, Y, N2, ldy, D, blocks);
    if (rc != AM_OK) return rc;
    AM_REQUIRE(nscales >= 1 && nscales <= AM_MMD_MULTI_MAX, AM_ERR_BAD_SHAPE,
               "nscales = %d: one call takes 1 .. AM_MMD_MULTI_MAX = %d scales (split a longer grid into several calls)", nscales,
               AM_MMD_MULTI_MAX);
    AM_REQUIRE(kernel != AM_MMD_ENERGY || nscales == 1, AM_ERR_BAD_SHAPE, "nscales = %d: the energy kernel has no scale, nscales must be 1",
               nscales);
    MultiCall c{};
    for (int j = 0; j < nscales; ++j) {
        AM_REQUIRE(finite_positive(scales[j]), AM_ERR_BAD_ARG, "scales[%d] = %g must be finite and positive", j, scales[j]);
        c.sc.c[j] = scales[j];
    }
    AM_REQUIRE(kernel == AM_MMD_ENERGY || bw2_dev != nullptr || finite_positive(bw2), AM_ERR_BAD_ARG,
               "bw2 = %g must be finite and positive (or bw2_dev given)", bw2);
    c.bw2_dev = kernel == AM_MMD_ENERGY ? nullptr : bw2_dev;
    c.bw2 = kernel == AM_MMD_ENERGY ? 1.0 : bw2;
    rc = open_call(c, X, N1, ldx, Y, N2, ldy, D, nscales, blocks, out_sums, ws, ws_bytes, "am_mmd_multi_workspace_bytes", stream);
    if (rc != AM_OK) return rc;
    switch (kernel) {
        case AM_MMD_GAUSSIAN: return launch_scales<AM_MMD_GAUSSIAN>(c);
        case AM_MMD_LAPLACIAN: return launch_scales<AM_MMD_LAPLACIAN>(c);
        default: return launch_tail<AM_MMD_ENERGY, 1>(c);
    }
}
