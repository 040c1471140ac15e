// K-means on the f32 tile engine: the two halves of a Lloyd iteration, each one entry point.
//
// ASSIGN (am_kmeans_assign_f32): for every row of X the nearest of the K centroids, without an N x K matrix.  This is the
// exact search of knn_search.hip at k = 1 with the list taken out: the same 128 x 128 tile kernel (dense_pipeline_early
// with the production schedule, the (row block) x (column chunk) plan of work_item / choose_chunks, the KTAIL instantiation
// for D % 32 != 0) and the same arithmetic of a pair,
//     d2 = max(fmaf(-2, <x, c>, |x|^2 + |c|^2), 0)       NaN -> +inf (clamp0); a padded column has |c|^2 = +inf
// with the f32 norms of launch_norms, so labels and distances have the bits of am_knn_search_f32(k = 1, squared).  What a
// lane keeps per row is ONE 64-bit key
//     key = (uint64)(bits(d2) & 0x7fffffff) << 32 | column
// - no list, no insert chain.  Behind the value gate of the search (the tile minimum against the key's distance, strict:
// a lane meets its columns in increasing order, so an equal distance always has the larger column) the sixteen values of
// an accumulator tile are reduced to their first minimum on the VALUE and one key is formed and min-ed.  Ties therefore go
// to the smallest column whatever the chunking.  The four keys of a row (2 half-waves x 2 column-half waves) meet in LDS,
// the chunks' keys in kmeans_assign_merge_kernel, which also writes (-1, +inf) for a row without a finite distance and
// the block sums of d2 in f64; kmeans_inertia_kernel adds those in a fixed tree.  No floating-point atomics anywhere:
// every call returns the same bits.
//
// Register budget: 64 accumulators, 64 staging registers (two slabs in flight), 32 fragment registers and 4 key registers
// - 28 fewer than the search's shortest list; __launch_bounds__(256, 2), two workgroups per CU (2 x 73 KiB of LDS).
//
// UPDATE (am_kmeans_update_f32): centroid c = mean of its rows, accumulated in f64 in the order of `order`, divided in f64,
// rounded once.  Bandwidth-bound; every row is read once, a wave reads 1 KiB of a row at a time (float4 per lane, 256
// columns per workgroup).  `order` is cut into SEGMENTS of SEG_ROWS positions, one per workgroup, which walks its rows in
// order and closes a sum whenever the cluster changes.  A cluster that lies inside one segment is finished there.  A
// cluster that crosses segment borders leaves one partial sum per segment it touches - a segment has at most one cluster
// that began before it (slot 0) and one that goes on behind it (slot 1) - and kmeans_update_finish_kernel adds them in
// segment order.  Skewed cluster sizes cost nothing: the work is cut by rows, not by clusters.
#include "row_sweep.h"

namespace am {
namespace kmeans {

constexpr unsigned long long EMPTY_KEY = 0x7f800000ffffffffull;          // (+inf, no column): larger than every real key
constexpr unsigned INF_BITS = 0x7f800000u;
constexpr size_t LDS_BYTES = (ENGINE_LDS_FLOATS + 2 * TB) * sizeof(float);   // staging slabs + [2][128] centroid norms
constexpr int MERGE_THREADS = 256;
constexpr int SEG_ROWS = 64;                                             // positions of `order` per update workgroup
constexpr int UPD_THREADS = 64;
constexpr int UPD_COLS = UPD_THREADS * 4;                                // columns per update workgroup

struct AssignEpilogue : ColumnAux<PAD_INF> {            // |c_j|^2 of the tile (+inf past the end)
    float xn[2];
    unsigned long long best[2];

    __device__ __forceinline__ AssignEpilogue(const LaneInfo& l) : ColumnAux<PAD_INF>(l) {}
    __device__ __forceinline__ float last(int nt) const { return __uint_as_float((unsigned)(best[nt] >> 32)); }

    __device__ __forceinline__ void finish(int t, int64_t qtile, f32x16 (&acc)[2][2]) {
        const float* a = tile(t);
        const unsigned cbase = (unsigned)(qtile * TB + L.wm * 64 + L.h * 4);      // the lane's first column of the tile
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            f32x4 yn[4];
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) yn[g4] = *reinterpret_cast<const f32x4*>(a + mt * 32 + g4 * 8);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                // the gate runs on unclamped values: max(., 0) commutes with min, and a NaN loses every compare
                float tmin = INFINITY;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) tmin = fminf(tmin, fmaf(-2.f, acc[mt][nt][reg], xn[nt] + yn[reg >> 2][reg & 3]));
                tmin = fmaxf(tmin, 0.f);
                // common case after warm-up: no lane of the wave improves its key with this 32 x 32 tile
                if (__any(tmin < last(nt))) {
                    float vmin = INFINITY;
                    unsigned rel = 0;
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {                 // ascending registers = ascending columns: the first minimum
                        const float d2 = clamp0(fmaf(-2.f, acc[mt][nt][reg], xn[nt] + yn[reg >> 2][reg & 3]));
                        const bool lt = d2 < vmin;
                        vmin = lt ? d2 : vmin;
                        rel = lt ? (unsigned)(mt * 32 + (reg & 3) + 8 * (reg >> 2)) : rel;
                    }
                    const unsigned long long key = ((unsigned long long)(__float_as_uint(vmin) & 0x7fffffffu) << 32) | (cbase + rel);
                    best[nt] = key < best[nt] ? key : best[nt];
                }
            }
        }
    }
};

// partial[chunk * N + row] = smallest key of `row` inside column chunk `chunk`
template <bool KTAIL>
__global__ void __launch_bounds__(ENGINE_THREADS, 2)
kmeans_assign_kernel(const float* __restrict__ X, int64_t N, int64_t ldx, const float* __restrict__ xnorm,
                     const float* __restrict__ C, int64_t K, int64_t ldc, const float* __restrict__ cnorm, int D, int nchunks,
                     unsigned long long* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LaneInfo L;
    const WorkItem w = work_item((K + TB - 1) / TB, nchunks);
    const int chunk = blockIdx.x % nchunks;            // the chunk work_item gave this workgroup: its slice of `partial`

    AssignEpilogue epi(L);
    epi.src[0] = cnorm;
    epi.nc = K;
    epi.lds = lds + ENGINE_LDS_FLOATS;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        epi.xn[nt] = row_norm(xnorm, w.prow0, N, L, nt);
        epi.best[nt] = EMPTY_KEY;
    }
    dense_pipeline_early<EV_DEFAULT, KTAIL>(C, K, ldc, LinearTiles{w.qtile0}, X, N, ldx, w.prow0, w.ntiles, D, lds, L, epi);

    // a row is covered by 4 keys (2 half-waves x 2 column-half waves): [2][64][4] keys through the staging slabs, free now
    unsigned long long* mg = reinterpret_cast<unsigned long long*>(lds);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) mg[join_slot(L, nt)] = epi.best[nt];
    __syncthreads();
    if (L.tid < 128) {
        const int64_t i = joined_row(w.prow0, L.tid);
        if (i < N) {
            const unsigned long long* src = mg + L.tid * 4;
            unsigned long long m = src[0];
#pragma unroll
            for (int s = 1; s < 4; ++s) m = src[s] < m ? src[s] : m;
            partial[(int64_t)chunk * N + i] = m;
        }
    }
}

// smallest key of a row over all chunks -> (label, d2); no finite distance -> (-1, +inf), left out of the sum
__global__ void __launch_bounds__(MERGE_THREADS)
kmeans_assign_merge_kernel(const unsigned long long* __restrict__ partial, int64_t N, int nchunks, int64_t* __restrict__ labels,
                           float* __restrict__ d2_out, double* __restrict__ block_sums) {
    __shared__ double s[MERGE_THREADS];
    const int64_t i = (int64_t)blockIdx.x * MERGE_THREADS + threadIdx.x;
    double v = 0.0;
    if (i < N) {
        unsigned long long m = partial[i];
        for (int c = 1; c < nchunks; ++c) {
            const unsigned long long o = partial[(int64_t)c * N + i];
            m = o < m ? o : m;
        }
        const unsigned bits = (unsigned)(m >> 32);
        const bool found = bits < INF_BITS;
        const float d2 = found ? __uint_as_float(bits) : INFINITY;
        labels[i] = found ? (int64_t)(unsigned)m : (int64_t)-1;
        d2_out[i] = d2;
        v = found ? (double)d2 : 0.0;
    }
    const double total = block_reduce_256<SumOp>(v, s);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(MERGE_THREADS)
kmeans_inertia_kernel(const double* __restrict__ block_sums, int64_t nblocks, double* __restrict__ inertia) {
    __shared__ double s[MERGE_THREADS];
    double v = 0.0;
    for (int64_t j = threadIdx.x; j < nblocks; j += MERGE_THREADS) v += block_sums[j];
    const double total = block_reduce_256<SumOp>(v, s);
    if (threadIdx.x == 0) inertia[0] = total;
}

// ---- update ------------------------------------------------------------------------------------------------------------
// value of lane j (wave-uniform j) of a 64-bit register pair, as a scalar
__device__ __forceinline__ int64_t lane_value(int64_t v, int j) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v & 0xffffffffull), j);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), j);
    return (int64_t)(((unsigned long long)hi << 32) | lo);
}

// partial[(seg * 2 + slot) * ldp + col]: slot 0 = the cluster that began before segment `seg`, slot 1 = the one that goes on
// behind it.  Every index read from `order`, `labels` and `offsets` is range-checked before it addresses anything.
__global__ void __launch_bounds__(UPD_THREADS)
kmeans_update_kernel(const float* __restrict__ X, int64_t N, int64_t ldx, int D, const int64_t* __restrict__ labels,
                     const int64_t* __restrict__ order, const int64_t* __restrict__ offsets, int64_t K, float* __restrict__ Cnew,
                     int64_t ldcn, double* __restrict__ partial, int64_t ldp) {
    const int lane = threadIdx.x;
    const int64_t seg = blockIdx.x;
    const int col = (int)blockIdx.y * UPD_COLS + lane * 4;
    // lane j holds position seg * SEG_ROWS + j of `order`: its row and that row's cluster (-1: nothing to add)
    int64_t row = -1, cl = -1;
    {
        const int64_t p = seg * SEG_ROWS + lane;
        if (p < N) {
            const int64_t r = order[p];
            if (r >= 0 && r < N) {
                const int64_t c = labels[r];
                if (c >= 0 && c < K) {
                    row = r;
                    cl = c;
                }
            }
        }
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    int64_t cur = -1;
    auto flush = [&](int64_t c) {
        if (c < 0) return;
        const int64_t lo = offsets[c], hi = offsets[c + 1];
        if (hi <= lo || col >= D) return;
        const int64_t b0 = lo / SEG_ROWS, b1 = (hi - 1) / SEG_ROWS;
        if (b0 == b1) {                                    // the whole cluster lies in this segment: finished here
            const double cnt = (double)(hi - lo);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (col + e < D) Cnew[c * ldcn + col + e] = (float)(acc[e] / cnt);
        } else {
            double* dst = partial + (seg * 2 + (seg == b0 ? 1 : 0)) * ldp + col;
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[e] = acc[e];
        }
    };
#pragma unroll 1
    for (int j0 = 0; j0 < SEG_ROWS; j0 += 8) {
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {                      // eight rows in flight per wave
            const int64_t r = lane_value(row, j0 + u);
            v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (r >= 0 && col < D) v[u] = *reinterpret_cast<const f32x4*>(X + r * ldx + col);   // ld % 4 == 0: stays in the row
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t c = lane_value(cl, j0 + u);
            if (c != cur) {                                // wave-uniform
                flush(cur);
                cur = c;
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = 0.0;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += (double)v[u][e];
        }
    }
    flush(cur);
}

// one thread per centroid element: the count, the copy of an empty cluster's old centroid, the partial sums of a cluster
// that crosses segments in segment order
__global__ void __launch_bounds__(256)
kmeans_update_finish_kernel(const int64_t* __restrict__ offsets, int64_t K, int D, const unsigned* Cold, int64_t ldco,
                            unsigned* Cnew, int64_t ldcn, int64_t* __restrict__ counts,
                            const double* __restrict__ partial, int64_t ldp, int64_t nseg) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= K * D) return;
    const int64_t c = g / D;
    const int col = (int)(g - c * D);
    const int64_t lo = offsets[c], hi = offsets[c + 1];
    const int64_t cnt = hi > lo ? hi - lo : 0;
    if (col == 0) counts[c] = cnt;
    if (cnt == 0) {
        Cnew[c * ldcn + col] = Cold[c * ldco + col];       // bit for bit
        return;
    }
    int64_t b0 = lo / SEG_ROWS, b1 = (hi - 1) / SEG_ROWS;
    if (b0 == b1) return;                                  // written by kmeans_update_kernel
    b0 = b0 < 0 ? 0 : (b0 > nseg - 1 ? nseg - 1 : b0);     // (inconsistent offsets must not address outside `partial`)
    if (b1 > nseg - 1) b1 = nseg - 1;
    double s = partial[(b0 * 2 + 1) * ldp + col];
    for (int64_t b = b0 + 1; b <= b1; ++b) s += partial[(b * 2) * ldp + col];
    Cnew[c * ldcn + col] = __float_as_uint((float)(s / (double)cnt));
}

static bool assign_shape_ok(int64_t N, int64_t K, int D) { return sweep_shape_ok(N, K, D, COLUMNS_KEYED); }

struct AssignBuffers {
    float *xn, *cn;
    unsigned long long* partial;
    double* block_sums;
};
static void carve(Carver& c, int64_t N, int64_t K, int nchunks, AssignBuffers& b) {
    b.xn = c.take<float>((size_t)N);
    b.cn = c.take<float>((size_t)K);
    b.partial = c.take<unsigned long long>((size_t)nchunks * (size_t)N);
    b.block_sums = c.take<double>((size_t)ceil_div(N, MERGE_THREADS));
}

static bool update_shape_ok(int64_t N, int64_t K, int D) {
    return N >= 1 && K >= 1 && D >= 1 && ceil_div(N, SEG_ROWS) < (int64_t)0x7fffffff && ceil_div(D, UPD_COLS) <= 65535 &&
           K <= ((int64_t)1 << 39) / D;                                       // one thread per centroid element, 256 per workgroup
}
static int64_t partial_ld(int D) { return ceil_div(D, 4) * 4; }

}  // namespace kmeans
}  // namespace am

using namespace am;

extern "C" size_t am_kmeans_assign_workspace_bytes(int64_t N, int64_t K, int D) {
    if (!kmeans::assign_shape_ok(N, K, D)) return 0;
    Carver c(nullptr, 0);
    kmeans::AssignBuffers b;
    kmeans::carve(c, N, K, choose_chunks(N, K), b);
    return c.off;
}

extern "C" int am_kmeans_assign_f32(const float* X, int64_t N, int64_t ldx, const float* C, int64_t K, int64_t ldc, int D,
                                    int64_t* labels, float* d2, double* inertia, void* ws, size_t ws_bytes, am_stream_t stream) {
    int rc;
    if ((rc = check_matrix(X, N, ldx, D, "X")) != AM_OK) return rc;
    if ((rc = check_matrix(C, K, ldc, D, "C")) != AM_OK) return rc;
    AM_REQUIRE(labels != nullptr && d2 != nullptr && inertia != nullptr, AM_ERR_BAD_ARG, "%s is null",
               labels == nullptr ? "labels" : d2 == nullptr ? "d2" : "inertia");
    AM_REQUIRE(kmeans::assign_shape_ok(N, K, D), AM_ERR_BAD_SHAPE,
               "N=%lld K=%lld: a centroid index takes 32 bits of a key (K < 2^32 - 1)", (long long)N, (long long)K);
    const int nchunks = choose_chunks(N, K);
    Carver c(ws, ws_bytes);
    kmeans::AssignBuffers b;
    kmeans::carve(c, N, K, nchunks, b);
    AM_REQUIRE(c.ok(), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (am_kmeans_assign_workspace_bytes), have %zu", c.off,
               ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = launch_norms(X, N, ldx, D, b.xn, st)) != AM_OK) return rc;
    if ((rc = launch_norms(C, K, ldc, D, b.cn, st)) != AM_OK) return rc;
    rc = launch_sweep(&kmeans::kmeans_assign_kernel<false>, &kmeans::kmeans_assign_kernel<true>, kmeans::LDS_BYTES, N, nchunks, D, st, X, N,
                      ldx, b.xn, C, K, ldc, b.cn, D, nchunks, b.partial);
    if (rc != AM_OK) return rc;
    const int64_t nblocks = ceil_div(N, kmeans::MERGE_THREADS);
    hipLaunchKernelGGL(kmeans::kmeans_assign_merge_kernel, dim3((unsigned)nblocks), dim3(kmeans::MERGE_THREADS), 0, st,
                       (const unsigned long long*)b.partial, N, nchunks, labels, d2, b.block_sums);
    AM_LAUNCH_CHECK();
    hipLaunchKernelGGL(kmeans::kmeans_inertia_kernel, dim3(1), dim3(kmeans::MERGE_THREADS), 0, st, (const double*)b.block_sums, nblocks,
                       inertia);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

extern "C" size_t am_kmeans_update_workspace_bytes(int64_t N, int64_t K, int D) {
    if (!kmeans::update_shape_ok(N, K, D)) return 0;
    Carver c(nullptr, 0);
    c.take<double>((size_t)ceil_div(N, kmeans::SEG_ROWS) * 2 * (size_t)kmeans::partial_ld(D));
    return c.off;
}

extern "C" int am_kmeans_update_f32(const float* X, int64_t N, int64_t ldx, int D, const int64_t* labels, const int64_t* order,
                                    const int64_t* offsets, int64_t K, const float* C_old, int64_t ldc_old, float* C_new,
                                    int64_t ldc_new, int64_t* counts, void* ws, size_t ws_bytes, am_stream_t stream) {
    int rc;
    if ((rc = check_matrix(X, N, ldx, D, "X")) != AM_OK) return rc;
    if ((rc = check_matrix(C_old, K, ldc_old, D, "C_old")) != AM_OK) return rc;
    if ((rc = check_matrix(C_new, K, ldc_new, D, "C_new")) != AM_OK) return rc;
    AM_REQUIRE(labels != nullptr && order != nullptr && offsets != nullptr && counts != nullptr, AM_ERR_BAD_ARG, "%s is null",
               labels == nullptr ? "labels" : order == nullptr ? "order" : offsets == nullptr ? "offsets" : "counts");
    AM_REQUIRE(kmeans::update_shape_ok(N, K, D), AM_ERR_BAD_SHAPE, "N=%lld K=%lld D=%d: too large for one launch", (long long)N,
               (long long)K, D);
    const int64_t nseg = ceil_div(N, kmeans::SEG_ROWS), ldp = kmeans::partial_ld(D);
    Carver c(ws, ws_bytes);
    double* partial = c.take<double>((size_t)nseg * 2 * (size_t)ldp);
    AM_REQUIRE(c.ok(), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (am_kmeans_update_workspace_bytes), have %zu", c.off,
               ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(kmeans::kmeans_update_kernel, dim3((unsigned)nseg, (unsigned)ceil_div(D, kmeans::UPD_COLS)),
                       dim3(kmeans::UPD_THREADS), 0, st, X, N, ldx, D, labels, order, offsets, K, C_new, ldc_new, partial, ldp);
    AM_LAUNCH_CHECK();
    hipLaunchKernelGGL(kmeans::kmeans_update_finish_kernel, dim3((unsigned)ceil_div(K * D, 256)), dim3(256), 0, st, offsets, K, D,
                       reinterpret_cast<const unsigned*>(C_old), ldc_old, reinterpret_cast<unsigned*>(C_new), ldc_new, counts,
                       (const double*)partial, ldp, nseg);
    AM_LAUNCH_CHECK();
    return AM_OK;
}
