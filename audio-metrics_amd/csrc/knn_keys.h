// The 64-bit (distance, column) keys of the nearest-neighbour searches: knn_search.hip (exclusion by index) and
// knn_groups.hip (exclusion by label) keep the same sorted lists, write the same partial lists and share ONE merge kernel,
// which lives in knn_search.hip and is reached from the other file through launch_merge.
//     key = (uint64)(bits(d2) & 0x7fffffff) << 32 | column
// Non-negative floats order like their bit patterns, so one unsigned compare orders by distance and then by column.
#pragma once
#include "row_sweep.h"

namespace am {
namespace search {

constexpr int MAX_K = 32;
constexpr unsigned long long EMPTY_KEY = 0x7f800000ffffffffull;          // (+inf, no column): larger than every real key
constexpr unsigned INF_BITS = 0x7f800000u;

__host__ __device__ constexpr int kcap_for(int k) { return k <= 8 ? 8 : k <= 16 ? 16 : 32; }

// Branch-free sorted insertion of a key into an ascending list of CAP keys (list_insert of tile_engine.h on uint64:
// compare-exchange down the list, fully unrolled).  A key >= best[CAP-1] falls through.
template <int CAP>
__device__ __forceinline__ void key_insert(unsigned long long (&best)[CAP], unsigned long long x) {
#pragma unroll
    for (int i = 0; i < CAP; ++i) {
        const bool lt = x < best[i];
        const unsigned long long lo = lt ? x : best[i];
        x = lt ? best[i] : x;
        best[i] = lo;
    }
}

// ---- host side, the same for both searches: the shapes a call takes and what its workspace holds --------------------------
static inline bool shape_ok(int64_t N, int64_t M, int D, int k) { return k >= 1 && k <= MAX_K && sweep_shape_ok(N, M, D, COLUMNS_KEYED); }

struct Buffers {
    float *xn, *yn;
    unsigned long long* partial;
};
static inline void carve(Carver& c, int64_t N, int64_t M, int k, int nchunks, Buffers& b) {
    b.xn = c.take<float>((size_t)N);
    b.yn = c.take<float>((size_t)M);
    b.partial = c.take<unsigned long long>((size_t)nchunks * (size_t)N * kcap_for(k));
}

// knn_search_merge_kernel<kcap> of knn_search.hip on `st`: the k smallest keys of every row over the nchunks partial lists
// uint64 [nchunks][N][kcap] -> sqrt_rn(d2) (squared != 0: d2) and the column as int64, (+inf, -1) past the finite keys.
int launch_merge(int kcap, const unsigned long long* partial, int64_t N, int nchunks, int k, int squared, float* out_dist,
                 int64_t* out_idx, hipStream_t st);

}  // namespace search
}  // namespace am
