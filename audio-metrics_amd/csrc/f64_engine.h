// The f64 tile engine shared by pairwise_f64.hip and kad_f64.hip: 64 x 64 tiles on v_mfma_f64_16x16x4_f64, 256 threads,
// 16-element slabs through LDS at row stride 17 (the layout is described at the head of pairwise_f64.hip).
#pragma once
#include "am_common.h"

namespace am {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int FT = 64;                 // tile rows of either operand
constexpr int FK = 16;                 // inner-dimension slab
constexpr int FLD = 17;                // padded LDS row stride (doubles)
constexpr int FTILE = FT * FLD;        // one operand slab
constexpr int FENGINE_DOUBLES = 4 * FTILE;   // two stages x (Q slab, P slab) = 34 816 bytes
constexpr int FTHREADS = 256;

__device__ __forceinline__ double clamp0d(double v) { return v != v ? __builtin_inf() : fmax(v, 0.0); }

struct FLane {
    int tid, lane, wave, l15, l4;
    __device__ __forceinline__ FLane() {
        tid = threadIdx.x;
        lane = tid & 63;
        wave = tid >> 6;
        l15 = lane & 15;
        l4 = lane >> 4;
    }
    __device__ __forceinline__ int prow() const { return wave * 16 + l15; }                 // P row of the tile this lane owns
    __device__ __forceinline__ int qrow(int m, int r) const { return m * 16 + l4 + 4 * r; }   // Q row behind acc[m][r]
};

// rows base + (row0 + local) of a dense matrix, nullptr (= a zero row) past n
struct DenseRows64 {
    const double* base;
    int64_t ld, n, row0;
    __device__ __forceinline__ const double* operator()(int row) const {
        const int64_t g = row0 + row;
        return g < n ? base + g * ld : nullptr;
    }
};
// rows gathered through an index list: local row -> X[idx[pos0 + row]], zero rows past m
struct GatherRows64 {
    const double* base;
    int64_t ld;
    const int64_t* idx;
    int m, pos0;
    __device__ __forceinline__ const double* operator()(int row) const {
        const int p = pos0 + row;
        return p < m ? base + idx[p] * ld : nullptr;
    }
};

// acc[m][r] += <Q row 16 m + l4 + 4 r, P row 16 wave + l15> over the D inner elements.  All 256 threads take part.
// The caller's LDS writes before this call (side data of the tile) become visible at the first barrier inside.
template <class QRows, class PRows>
__device__ __forceinline__ void f64_tile(const QRows& qrows, const PRows& prows, int D, double* __restrict__ lds, const FLane& L,
                                         f64x4 (&acc)[4]) {
    const int srow = L.tid >> 2, scol = (L.tid & 3) * 4;             // this thread stages 4 elements of one row per operand
    const double* qsrc = qrows(srow);
    const double* psrc = prows(srow);
    const int nslabs = (D + FK - 1) / FK;
    double qv[4], pv[4];
    auto fetch = [&](int s) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = s * FK + scol + j;
            qv[j] = (qsrc != nullptr && k < D) ? qsrc[k] : 0.0;
            pv[j] = (psrc != nullptr && k < D) ? psrc[k] : 0.0;
        }
    };
    fetch(0);
    for (int s = 0; s < nslabs; ++s) {
        double* st = lds + (s & 1) * 2 * FTILE;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            st[srow * FLD + scol + j] = qv[j];
            st[FTILE + srow * FLD + scol + j] = pv[j];
        }
        __syncthreads();
        if (s + 1 < nslabs) fetch(s + 1);
        const double* q = st + L.l15 * FLD + L.l4;
        const double* p = st + FTILE + (L.wave * 16 + L.l15) * FLD + L.l4;
#pragma unroll
        for (int ks = 0; ks < FK / 4; ++ks) {
            const double b = p[ks * 4];
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(q[m * 16 * FLD + ks * 4], b, acc[m], 0, 0, 0);
        }
        // (no second barrier: the next slab goes to the other stage, which every wave finished reading before it arrived at
        // the barrier above)
    }
    __syncthreads();                                                 // the stages are free for the next tile / the caller
}

__device__ __forceinline__ void zero4(f64x4 (&acc)[4]) {
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m] = f64x4{0.0, 0.0, 0.0, 0.0};
}

}  // namespace am
