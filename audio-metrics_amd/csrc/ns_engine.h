// Device helpers of the Newton-Schulz solve shared by frechet.hip (one product) and frechet_batch.hip (B products advancing
// together): the 32 x 32 f64 tile product on v_mfma_f64_16x16x4_f64, the fixed-order workgroup sum, the per-solve state
// and the stopping rule.  Both files call the same code, so a product goes through the same arithmetic in the same order
// whichever entry point solves it.
#pragma once
#include "am_common.h"
#include <math.h>

namespace am {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int GT = 32;            // output tile (GT x GT), every wave computes all of it over its share of k
constexpr int GKC = 16;           // inner slab: lane (l15, l4) holds k = slab + 4 l4 + s, s = 0..3
constexpr int PST = GT + 1;       // row stride of the partial tiles in LDS

struct NsState {
    double prev_trace;            // last accepted tr(Y)
    double resid;                 // |I - ZY|_F at the last check
    double norm;                  // |A|_F
    int iters;
    int done;                     // 0 running, 1 converged, 2 trace stalled (noise), 3 zero matrix, 4 non-finite input
};

enum { MODE_PLAIN = 0, MODE_NS_T = 1 };

struct GemmJob {
    const double* A;
    const double* B;
    double* C;
};

// sum of `count` doubles by the whole workgroup in a fixed order (thread-strided partials, xor butterfly, 4 waves)
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
    __syncthreads();
    return s;
}

// 32 x 32 tile of A*B at (row0, col0); result of the four waves' k-shares combined in `part` (LDS, [4][GT * PST]).
// After the call thread t owns elements e = t, t + 256, t + 512, t + 768 (row e / 32, column e % 32) in out[4].
__device__ __forceinline__ void tile_product(const GemmJob& job, int n, int row0, int col0, double* part, double (&out)[4]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0, 0, 0, 0};
    const int nslab = (n + GKC - 1) / GKC;
    const bool vec = (n % 4 == 0) && ((reinterpret_cast<uintptr_t>(job.A) & 31u) == 0);
    double ra0[2][4], rb0[2][4], ra1[2][4], rb1[2][4];      // two register buffers, [tile half][s]
    auto fetch = [&](double (&ra)[2][4], double (&rb)[2][4], int slab) {
        const int k0 = slab * GKC + 4 * l4;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int gr = row0 + t * 16 + l15;
            if (vec && gr < n && k0 + 3 < n) {
                const f64x4 v = *reinterpret_cast<const f64x4*>(job.A + (int64_t)gr * n + k0);
#pragma unroll
                for (int s = 0; s < 4; ++s) ra[t][s] = v[s];
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) ra[t][s] = (gr < n && k0 + s < n) ? job.A[(int64_t)gr * n + k0 + s] : 0.0;
            }
            const int gc = col0 + t * 16 + l15;
#pragma unroll
            for (int s = 0; s < 4; ++s) rb[t][s] = (gc < n && k0 + s < n) ? job.B[(int64_t)(k0 + s) * n + gc] : 0.0;
        }
    };
    auto multiply = [&](const double (&ra)[2][4], const double (&rb)[2][4]) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(ra[mt][s], rb[nt][s], acc[mt][nt], 0, 0, 0);
    };
    // wave w takes slabs w, w + 4, ...; the next slab is in flight while this one multiplies
    int slab = wave;
    if (slab < nslab) fetch(ra0, rb0, slab);
    while (slab < nslab) {
        if (slab + 4 < nslab) fetch(ra1, rb1, slab + 4);
        multiply(ra0, rb0);
        slab += 4;
        if (slab >= nslab) break;
        if (slab + 4 < nslab) fetch(ra0, rb0, slab + 4);
        multiply(ra1, rb1);
        slab += 4;
    }
    // f64 C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg
    double* mine = part + wave * GT * PST;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) mine[(mt * 16 + l4 + 4 * r) * PST + nt * 16 + l15] = acc[mt][nt][r];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = tid + 256 * q;
        const int o = (e >> 5) * PST + (e & 31);
        out[q] = (part[o] + part[GT * PST + o]) + (part[2 * GT * PST + o] + part[3 * GT * PST + o]);
    }
    __syncthreads();
}

// The stopping rule (see file header) as a pure function of the previous state and the sums of ns_t_kernel: every
// workgroup evaluates it and gets the same answer; only one of them writes it down.
__device__ __forceinline__ NsState ns_next_state(const NsState& s, const double* __restrict__ resid_sums, int ntiles,
                                                 const double* __restrict__ trace_sums, int g, int n, double tol, double* red) {
    double r = 0, t = 0;
    for (int i = threadIdx.x; i < ntiles; i += blockDim.x) r += resid_sums[i];
    for (int i = threadIdx.x; i < g; i += blockDim.x) t += trace_sums[i];
    r = sqrt(block_sum(r, red));
    t = block_sum(t, red);
    NsState o = s;
    const bool finite = (t == t) && !isinf(t) && (r == r);
    if (!finite || t < s.prev_trace * (1.0 - 1e-14) - 1e-300) {
        o.done = isinf(s.prev_trace) ? 4 : 2;               // keep the previous trace
    } else {
        o.prev_trace = t;
        o.resid = r;
        o.iters = s.iters + 1;
        if (r < tol * sqrt((double)n)) o.done = 1;
    }
    return o;
}

}  // namespace am
