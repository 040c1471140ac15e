// What the per-sample scores of sample_scores.hip (every pair counts) and of sample_scores_groups.hip (a pair of equal
// labels is no pair) have in common: the two 64-bit keys a row keeps, the constants of the division gate, what a call's
// workspace holds, and the two small kernels around the tile kernel - scores_columns_kernel (cleaned radii and membership
// thresholds) and sample_scores_merge_kernel (the chunks' partials -> the five outputs) - which live in sample_scores.hip
// and are reached from the other file through launch_columns / launch_merge.
//     max key = (uint64)bits(q)   << 32 | (0xffffffff - column)      q >= 0: floats order like their bits
//     min key = (uint64)bits(r_j) << 32 | column                     over the members only
#pragma once
#include "row_sweep.h"

namespace am {
namespace scores {

constexpr unsigned long long NO_MEMBER = 0xffffffffffffffffull;          // min key of a row outside every ball
constexpr int MERGE_THREADS = 256;
constexpr float GATE_SHRINK = 1.f - 9.5367431640625e-07f;                // 1 - 2^-20
constexpr float GATE_TINY = 7.888609052210118e-31f;                      // 2^-100
constexpr float F32_MAX = 3.4028234663852886e+38f;
constexpr float F32_MIN_NORMAL = 1.1754943508222875e-38f;

// ---- host side, the same for both files: the shapes a call takes and what its workspace holds -----------------------------
static inline bool shape_ok(int64_t N, int64_t M, int D) { return sweep_shape_ok(N, M, D, COLUMNS_KEYED); }

struct Buffers {
    float *xn, *yn, *thr, *rad;
    unsigned long long *pmax, *pmin;
    int* pcnt;
};
static inline void carve(Carver& c, int64_t N, int64_t M, int nchunks, Buffers& b) {
    b.xn = c.take<float>((size_t)N);
    b.yn = c.take<float>((size_t)M);
    b.thr = c.take<float>((size_t)M);
    b.rad = c.take<float>((size_t)M);
    b.pmax = c.take<unsigned long long>((size_t)nchunks * (size_t)N);
    b.pmin = c.take<unsigned long long>((size_t)nchunks * (size_t)N);
    b.pcnt = c.take<int>((size_t)nchunks * (size_t)N);
}

// scores_columns_kernel of sample_scores.hip on `st`: rad[j] = r_y[j] > 0 ? r_y[j] : 0 and thr[j] = T'(rad[j]), j < M
int launch_columns(const float* r_y, int64_t M, float* rad, float* thr, hipStream_t st);

// sample_scores_merge_kernel of sample_scores.hip on `st`: max / min / sum of every row's partials [nchunks][N] -> the five
// outputs of am_sample_scores_f32
int launch_merge(const unsigned long long* pmax, const unsigned long long* pmin, const int* pcnt, int64_t N, int nchunks,
                 float* out_realism, int64_t* out_realism_idx, int32_t* out_count, float* out_rarity, int64_t* out_rarity_idx,
                 hipStream_t st);

}  // namespace scores
}  // namespace am
