// Exact k-nearest-neighbour SEARCH: for every row of X the k smallest distances to the rows of Y and the rows they
// belong to, without an N x M matrix.  The radii of the PRDC path (pairwise.hip: knn_partial_kernel / KnnEpilogue) keep
// lane-local sorted lists of the smallest d2 of a row and drop the column each value came from; this file keeps it.
//
// Arithmetic of one pair, exactly that of KnnEpilogue on the same 128 x 128 f32 tile engine (tile_engine.h,
// v_mfma_f32_32x32x2_f32, dense_pipeline_early with the production schedule):
//     d2 = max(fmaf(-2, <x, y>, |x|^2 + |y|^2), 0)       NaN -> +inf (clamp0); a padded column has |y|^2 = +inf
// with the f32 row norms of row_sqnorm_kernel (launch_norms of pairwise.hip).  Every reported squared
// distance therefore has the bits of the exact general kernel and of oracle/exact_c/pairwise_exact.c.
//
// Lists.  A list entry is ONE 64-bit key
//     key = (uint64)(bits(d2) & 0x7fffffff) << 32 | column
// Non-negative floats order like their bit patterns, so one unsigned compare orders by distance and then by column: ties
// go to the smallest column whatever the chunking, the tile order or the lane that saw the value - a call returns the
// same bits every time.  The column of accumulator register `reg` of tile mt is
//     qtile * 128 + wm * 64 + mt * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h
// = a per-tile base plus a compile-time constant; no index array lives in registers.  The two gates of KnnEpilogue are
// kept on the VALUE (the list's last distance is the high word of its last key): the tile minimum, then __any per
// element; after warm-up almost no tile reaches the 64-bit insert.  The gates are strict (d2 < last): a lane meets the
// columns of its chunk in increasing order, so a value equal to the list's last distance always has the larger column
// and loses the tie anyway; the insert itself compares whole keys.
//
// Self exclusion is by INDEX (column i + self_offset is skipped for row i; duplicates of a row stay its neighbours), and
// only the tiles the shifted diagonal crosses run the variant of the epilogue that tests for it.
//
// Column chunks: the (row block) x (column chunk) plan of the radii (work_item / choose_chunks of pairwise_common.h).
// Partial lists: uint64 [nchunks][N][KCAP] in the caller's workspace; knn_search_merge_kernel takes the k smallest
// keys of a row and writes sqrt_rn(d2) (or d2) and the column as int64, -1 where the distance is +inf (fewer than k
// finite candidates: M < k, M - 1 < k with exclusion, non-finite rows).
//
// Register budget (lists are 2 rows x KCAP keys x 2 registers per lane, beside 64 accumulators and the staging /
// fragment registers of the pipeline; no instantiation uses scratch - tests/test_knn_search_cpu.py):
//     KCAP  8:  32 list registers, __launch_bounds__(256, 2), two workgroups per CU
//     KCAP 16:  64 list registers, __launch_bounds__(256, 2), two workgroups per CU
//     KCAP 32: 128 list registers, __launch_bounds__(256, 1): ONE workgroup per CU (the lists alone are half of the 256
//              registers a wave has at two per SIMD)
#include "knn_keys.h"

namespace am {
namespace search {

constexpr size_t LDS_BYTES = (ENGINE_LDS_FLOATS + 2 * TB) * sizeof(float);   // staging slabs + [2][128] column norms

template <int KCAP>
struct KnnIndexEpilogue {
    const float* qnorm;
    int64_t nq;
    float* aux;                          // LDS [2][128] : |y_j|^2 of the tile (+inf past nq)
    int64_t self_lo;                     // column excluded for the first row of this row block (row r: self_lo + r); none: -2 * TB
    float xn[2];
    unsigned long long best[2][KCAP];
    float aux_reg;
    const LaneInfo& L;

    __device__ __forceinline__ KnnIndexEpilogue(const LaneInfo& l) : L(l) {}
    __device__ __forceinline__ void aux_issue(int, int64_t qtile) {
        if (L.tid < TB) {
            const int64_t j = qtile * TB + L.tid;
            aux_reg = j < nq ? qnorm[j] : INFINITY;
        }
    }
    __device__ __forceinline__ void aux_commit(int t) {
        if (L.tid < TB) aux[(t & 1) * TB + L.tid] = aux_reg;
    }
    __device__ __forceinline__ float last(int nt) const { return __uint_as_float((unsigned)(best[nt][KCAP - 1] >> 32)); }

    // The two gates run on values that are recomputed, not kept (16 more live registers cost the KCAP 16 form its second
    // workgroup per CU), and unclamped: max(., 0) commutes with min, and a NaN loses every compare.  On a tile the shifted
    // diagonal crosses (wave-uniform `diag`) the lane's excluded column counts as +inf.  Past the gates, the registers that
    // may improve some lane's list are visited through a wave-uniform bit mask, so that the 64-bit insert is instantiated
    // once per accumulator tile and not once per register (unrolled 16 times it pushed the KCAP 16 / 32 kernels over the
    // unroll budget and their accumulators into scratch).  The mask is taken before the inserts tighten the list: a
    // superset, and a key that no longer fits falls through the insert.
    __device__ __forceinline__ void finish(int t, int64_t qtile, f32x16 (&acc)[2][2]) {
        const float* a = aux + (t & 1) * TB + L.wm * 64 + L.h * 4;
        const int64_t c0 = qtile * TB + L.wm * 64 + L.h * 4;       // the lane's first column of the tile
        const unsigned cbase = (unsigned)c0;
        const bool diag = qtile * TB < self_lo + TB && qtile * TB + TB > self_lo;
        int srel[2] = {-1, -1};                                     // excluded column relative to c0 (-1: not in this tile)
        if (diag) {
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const int64_t rel = self_lo + sweep_row(0, L, nt) - c0;
                srel[nt] = (rel >= 0 && rel < 64) ? (int)rel : -1;
            }
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            f32x4 yn[4];
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) yn[g4] = *reinterpret_cast<const f32x4*>(a + mt * 32 + g4 * 8);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                auto value = [&](int reg, bool self_test) {
                    const float u = fmaf(-2.f, acc[mt][nt][reg], xn[nt] + yn[reg >> 2][reg & 3]);
                    return (self_test && mt * 32 + (reg & 3) + 8 * (reg >> 2) == srel[nt]) ? INFINITY : u;   // the row itself: by index
                };
                float tmin = INFINITY;
                if (diag) {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) tmin = fminf(tmin, value(reg, true));
                } else {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) tmin = fminf(tmin, value(reg, false));
                }
                tmin = fmaxf(tmin, 0.f);
                // common case after warm-up: no lane of the wave improves its list with this 32 x 32 tile
                if (__any(tmin < last(nt))) {
                    unsigned mask = 0;
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg)
                        if (__any(value(reg, true) < last(nt))) mask |= 1u << reg;
                    while (mask != 0) {                             // wave-uniform, ascending registers = ascending columns
                        const int reg = __builtin_ctz(mask);
                        mask &= mask - 1;
                        const int rel = mt * 32 + (reg & 3) + 8 * (reg >> 2);
                        float p = acc[mt][nt][0];
#pragma unroll
                        for (int q = 1; q < 16; ++q) p = (reg == q) ? acc[mt][nt][q] : p;
                        const float u = fmaf(-2.f, p, xn[nt] + a[rel]);
                        const float d2 = rel == srel[nt] ? INFINITY : clamp0(u);
                        key_insert<KCAP>(best[nt], ((unsigned long long)(__float_as_uint(d2) & 0x7fffffffu) << 32) | (cbase + (unsigned)rel));
                    }
                }
            }
        }
    }
};

// partial[(chunk * N + row) * KCAP + s] = s-th smallest key of `row` inside column chunk `chunk`
template <int KCAP, bool KTAIL>
__global__ void __launch_bounds__(ENGINE_THREADS, KCAP <= 16 ? 2 : 1)
knn_search_kernel(const float* __restrict__ X, int64_t N, int64_t ldx, const float* __restrict__ xnorm,
                  const float* __restrict__ Y, int64_t M, int64_t ldy, const float* __restrict__ ynorm, int D, int nchunks,
                  int64_t self_offset, unsigned long long* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LaneInfo L;
    const WorkItem w = work_item((M + TB - 1) / TB, nchunks);
    const int chunk = blockIdx.x % nchunks;            // the chunk work_item gave this workgroup: its slice of `partial`

    KnnIndexEpilogue<KCAP> epi(L);
    epi.qnorm = ynorm;
    epi.nq = M;
    epi.aux = lds + ENGINE_LDS_FLOATS;
    epi.self_lo = self_offset >= 0 ? w.prow0 + self_offset : -2 * TB;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        epi.xn[nt] = row_norm(xnorm, w.prow0, N, L, nt);
#pragma unroll
        for (int s = 0; s < KCAP; ++s) epi.best[nt][s] = EMPTY_KEY;
    }
    dense_pipeline_early<EV_DEFAULT, KTAIL>(Y, M, ldy, LinearTiles{w.qtile0}, X, N, ldx, w.prow0, w.ntiles, D, lds, L, epi);

    // (its own slot and row arithmetic, one P tile per pass: through join_slot / joined_row of row_sweep.h the register
    // numbers of all six instantiations moved, and the 16-key form has no register to spare)
    // A P row is covered by 4 lists (2 half-waves x 2 Q-half waves): merged through LDS, the rows of one 32-row P tile
    // per wave at a time ([64][4][KCAP] keys: 64 KiB at KCAP = 32, inside the 72 KiB of staging slabs, which are free now)
    unsigned long long* mg = reinterpret_cast<unsigned long long*>(lds);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        if (nt != 0) __syncthreads();                  // the readers of the first pass are done
        unsigned long long* dst = mg + ((L.wn * 32 + L.r) * 4 + (L.wm * 2 + L.h)) * KCAP;
#pragma unroll
        for (int s = 0; s < KCAP; ++s) dst[s] = epi.best[nt][s];
        __syncthreads();
        if (L.tid < 64) {
            const int64_t i = w.prow0 + (L.tid >> 5) * 64 + nt * 32 + (L.tid & 31);
            if (i < N) {
                const unsigned long long* src = mg + L.tid * 4 * KCAP;
                unsigned long long m[KCAP];
#pragma unroll
                for (int s = 0; s < KCAP; ++s) m[s] = src[s];
                for (int s = KCAP; s < 4 * KCAP; ++s) key_insert<KCAP>(m, src[s]);
                unsigned long long* out = partial + ((int64_t)chunk * N + i) * KCAP;
#pragma unroll
                for (int s = 0; s < KCAP; ++s) out[s] = m[s];
            }
        }
    }
}

// the k smallest keys of a row over all chunks -> (distance, column); +inf distance -> column -1
template <int KCAP>
__global__ void __launch_bounds__(256) knn_search_merge_kernel(const unsigned long long* __restrict__ partial, int64_t N, int nchunks,
                                                               int k, int squared, float* __restrict__ out_dist,
                                                               int64_t* __restrict__ out_idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    unsigned long long m[KCAP];
#pragma unroll
    for (int s = 0; s < KCAP; ++s) m[s] = partial[i * KCAP + s];
    for (int c = 1; c < nchunks; ++c) {
        const unsigned long long* src = partial + ((int64_t)c * N + i) * KCAP;
        for (int s = 0; s < KCAP; ++s) key_insert<KCAP>(m, src[s]);
    }
#pragma unroll
    for (int s = 0; s < KCAP; ++s) {
        if (s < k) {
            const unsigned bits = (unsigned)(m[s] >> 32);
            const float d2 = __uint_as_float(bits);
            out_dist[i * k + s] = squared ? d2 : sqrt_rn(d2);
            out_idx[i * k + s] = bits >= INF_BITS ? (int64_t)-1 : (int64_t)(unsigned)m[s];
        }
    }
}

template <int KCAP>
static int run_merge(const unsigned long long* partial, int64_t N, int nchunks, int k, int squared, float* out_dist, int64_t* out_idx,
                     hipStream_t st) {
    hipLaunchKernelGGL(knn_search_merge_kernel<KCAP>, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, st, partial, N, nchunks, k,
                       squared, out_dist, out_idx);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

// (knn_keys.h: the grouped search of knn_groups.hip merges its partial lists with the same kernel)
int launch_merge(int kcap, const unsigned long long* partial, int64_t N, int nchunks, int k, int squared, float* out_dist,
                 int64_t* out_idx, hipStream_t st) {
    switch (kcap) {
        case 8:  return run_merge<8>(partial, N, nchunks, k, squared, out_dist, out_idx, st);
        case 16: return run_merge<16>(partial, N, nchunks, k, squared, out_dist, out_idx, st);
        default: return run_merge<32>(partial, N, nchunks, k, squared, out_dist, out_idx, st);
    }
}

template <int KCAP>
static int run(const float* X, int64_t N, int64_t ldx, const float* xn, const float* Y, int64_t M, int64_t ldy, const float* yn,
               int D, int k, int nchunks, int64_t self_offset, int squared, unsigned long long* partial, float* out_dist,
               int64_t* out_idx, hipStream_t st) {
    const int rc = launch_sweep(&knn_search_kernel<KCAP, false>, &knn_search_kernel<KCAP, true>, LDS_BYTES, N, nchunks, D, st, X, N, ldx,
                                xn, Y, M, ldy, yn, D, nchunks, self_offset, partial);
    if (rc != AM_OK) return rc;
    return run_merge<KCAP>(partial, N, nchunks, k, squared, out_dist, out_idx, st);
}

}  // namespace search
}  // namespace am

using namespace am;

extern "C" size_t am_knn_search_workspace_bytes(int64_t N, int64_t M, int D, int k) {
    if (!search::shape_ok(N, M, D, k)) return 0;
    Carver c(nullptr, 0);
    search::Buffers b;
    search::carve(c, N, M, k, choose_chunks(N, M), b);
    return c.off;
}

extern "C" int am_knn_search_chunks(int64_t N, int64_t M, int D, int k) {
    return search::shape_ok(N, M, D, k) ? choose_chunks(N, M) : 0;
}

extern "C" int am_knn_search_f32(const float* X, int64_t N, int64_t ldx, const float* Y, int64_t M, int64_t ldy, int D, int k,
                                 int64_t self_offset, int squared, float* out_dist, int64_t* out_idx, void* ws, size_t ws_bytes,
                                 am_stream_t stream) {
    int rc;
    if ((rc = check_matrix(X, N, ldx, D, "X")) != AM_OK) return rc;
    if ((rc = check_matrix(Y, M, ldy, D, "Y")) != AM_OK) return rc;
    AM_REQUIRE(out_dist != nullptr && out_idx != nullptr, AM_ERR_BAD_ARG, "%s is null", out_dist == nullptr ? "out_dist" : "out_idx");
    AM_REQUIRE(k >= 1 && k <= search::MAX_K, AM_ERR_BAD_SHAPE, "k = %d: the search keeps 1 .. %d neighbours per row", k, search::MAX_K);
    AM_REQUIRE(search::shape_ok(N, M, D, k), AM_ERR_BAD_SHAPE, "N=%lld M=%lld: a column index takes 32 bits of a list key (M < 2^32 - 1)",
               (long long)N, (long long)M);
    const int nchunks = choose_chunks(N, M);
    Carver c(ws, ws_bytes);
    search::Buffers b;
    search::carve(c, N, M, k, nchunks, b);
    AM_REQUIRE(c.ok(), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (am_knn_search_workspace_bytes), have %zu", c.off, ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // a column past the end excludes nothing; the kernel adds row indices to the offset
    if (self_offset >= M) self_offset = -1;
    const float* yn;
    if ((rc = launch_norms_pair(X, N, ldx, Y, M, ldy, D, b.xn, b.yn, st, &yn)) != AM_OK) return rc;
    switch (search::kcap_for(k)) {
        case 8:  return search::run<8>(X, N, ldx, b.xn, Y, M, ldy, yn, D, k, nchunks, self_offset, squared, b.partial, out_dist, out_idx, st);
        case 16: return search::run<16>(X, N, ldx, b.xn, Y, M, ldy, yn, D, k, nchunks, self_offset, squared, b.partial, out_dist, out_idx, st);
        default: return search::run<32>(X, N, ldx, b.xn, Y, M, ldy, yn, D, k, nchunks, self_offset, squared, b.partial, out_dist, out_idx, st);
    }
}
