// Classifier-output scores: row-wise quantities of an [N, C] matrix of logits, or of two matrices paired row by row.
// All arithmetic is f64; float32 rows are converted on load (exact), so both row types share every later bit.
//
// Row quantities of a row l:  M = max l_c,  e_c = exp(l_c - M),  S = sum e_c,  U = sum e_c (l_c - M),  p_c = e_c / S,
//     h = sum p_c log p_c = U / S - log S      (a logit of -inf is a masked class: p_c = 0, no term in U).
// A row with a NaN, a +inf, or nothing but -inf is non-finite: h = NaN, the row is counted and adds nothing else.
//
//   am_class_groups_*   the Inception Score of B groups of rows (the group-list protocol of groups_common.h):
//       cs_plan_kernel     gseg[b] = the number of 64-position segments in front of group b (a segment never crosses a group)
//       cs_rows_kernel     one workgroup per segment, wave w the rows w, w + 4, ... of it in ascending order.  A lane owns the
//                          columns 256 j + 4 lane .. + 3 (one 16-byte load per float32 chunk, a scalar tail for C % 4), holds
//                          them in registers (compile-time chunk count), reduces M, then S and U, with an xor butterfly and
//                          adds p_c into its wave's [C] f64 slab in LDS - plain read-add-write, the lane owns the column.
//                          The four slabs are added in wave order; the segment's [C] partial, its sum of h and its count of
//                          non-finite rows go to the workspace.
//       cs_groups_kernel   one workgroup per group: the segments added in ascending order, / n_b, m_b = sum pbar log pbar
//                          (0 log 0 = 0) thread-strided, xor butterfly, the four waves in order.
//   am_row_pairs_*      one value per row pair (cosine, or one of three Kullback-Leibler forms), one wave per pair, a
//       cs_pairs_kernel    workgroup the rows [64 g, 64 g + 64), its {sum v, sum v^2, finite, non-finite} to the workspace;
//       cs_sums_kernel     one workgroup adds the workgroups' partials in a fixed order (the shape of fi_sums_kernel).
// No floating-point atomics and no data-dependent order: every sum is a function of the shapes and the group sizes only.
#include "am_common.h"
#include "groups_common.h"
#include <cmath>

namespace am {

constexpr int CS_SEG = 64;                  // list positions per segment, row pairs per workgroup
constexpr int CS_MAX_C = 2048;              // class groups: 4 slabs x 2048 f64 = 64 KiB, two workgroups per CU
constexpr int CS_PAIR_MAX_C = 8192;
constexpr int CS_LDS_MAX = (4 * CS_MAX_C + 8) * 8;

__device__ __forceinline__ double cs_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ double cs_wave_max(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

// the elements k .. k + 3 of a row as doubles, `fill` past C.  float32: one 16-byte load where the four lie inside the row
// (X is 16-byte aligned, ld % 4 == 0, k % 4 == 0), else the scalar tail
__device__ __forceinline__ void cs_load4(const float* __restrict__ p, int k, int C, double fill, double (&v)[4]) {
    if (k + 3 < C) {
        const float4 f = *reinterpret_cast<const float4*>(p + k);
        v[0] = (double)f.x; v[1] = (double)f.y; v[2] = (double)f.z; v[3] = (double)f.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = k + e < C ? (double)p[k + e] : fill;
    }
}
__device__ __forceinline__ void cs_load4(const double* __restrict__ p, int k, int C, double fill, double (&v)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = k + e < C ? p[k + e] : fill;
}

// ---------------------------------------------------------------- class groups
__global__ void __launch_bounds__(256)
cs_plan_kernel(const int64_t* __restrict__ offs, int B, int64_t* __restrict__ gseg) {
    __shared__ int64_t tot[256];
    const int tid = threadIdx.x;
    const int64_t per = ((int64_t)B + 255) / 256;
    const int64_t b0 = tid * per < B ? tid * per : B, b1 = b0 + per < B ? b0 + per : B;
    int64_t s = 0;
    for (int64_t b = b0; b < b1; ++b) s += (offs[b + 1] - offs[b] + CS_SEG - 1) / CS_SEG;
    tot[tid] = s;
    __syncthreads();
    int64_t base = 0;
    for (int t = 0; t < tid; ++t) base += tot[t];
    for (int64_t b = b0; b < b1; ++b) {
        gseg[b] = base;
        base += (offs[b + 1] - offs[b] + CS_SEG - 1) / CS_SEG;
    }
    if (tid == 255) gseg[B] = base;
}

template <class T, int CH>
__global__ void __launch_bounds__(256, 2)
cs_rows_kernel(const T* __restrict__ X, int64_t N, int64_t ld, int C, const int64_t* __restrict__ idx, const int64_t* __restrict__ offs,
               const int64_t* __restrict__ gseg, int B, double* __restrict__ part, double* __restrict__ out_h,
               unsigned long long* __restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) double cs_lds[];        // [4][C] slabs, then 4 sums of h, 4 counts
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t seg = blockIdx.x;
    int lo = 0, hi = B;                                                     // gseg[lo] <= seg < gseg[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (gseg[mid] <= seg) lo = mid; else hi = mid;
    }
    const int64_t pos0 = offs[lo] + (seg - gseg[lo]) * CS_SEG;
    const int64_t left = offs[lo + 1] - pos0;
    const int cnt = left < CS_SEG ? (int)left : CS_SEG;
    double* slab = cs_lds + wave * C;
    double* wsum = cs_lds + 4 * C;
#pragma unroll
    for (int j = 0; j < CH; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = 256 * j + 4 * lane + e;
            if (k < C) slab[k] = 0.0;
        }
    const double ninf = -__builtin_inf();
    double hsum = 0.0, nbad = 0.0;
    for (int r = wave; r < cnt; r += 4) {
        const int64_t pos = pos0 + r;
        const int64_t row = idx ? idx[pos] : pos;
        const bool inside = (unsigned long long)row < (unsigned long long)N;
        if (!inside && lane == 0) atomicMax(flag, (unsigned long long)pos + 1ull);     // never dereferenced
        const T* x = X + (inside ? row : 0) * ld;
        double v[CH][4];
#pragma unroll
        for (int j = 0; j < CH; ++j) cs_load4(x, 256 * j + 4 * lane, C, ninf, v[j]);
        double m = ninf;
        bool bad = false;
#pragma unroll
        for (int j = 0; j < CH; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                bad |= v[j][e] != v[j][e] || v[j][e] == __builtin_inf();
                m = fmax(m, v[j][e]);
            }
        m = cs_wave_max(m);
        bad = __any(bad) || m == ninf || !inside;
        double S = 0.0, U = 0.0;
#pragma unroll
        for (int j = 0; j < CH; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = v[j][e] - m;
                const double ex = exp(d);
                S += ex;
                U += d == ninf ? 0.0 : ex * d;
                v[j][e] = ex;
            }
        S = cs_wave_sum(S);
        U = cs_wave_sum(U);
        double h = U / S - log(S);
        if (bad) {
            h = __builtin_nan("");
            nbad += 1.0;
        } else {
            hsum += h;
#pragma unroll
            for (int j = 0; j < CH; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = 256 * j + 4 * lane + e;
                    if (k < C) slab[k] += v[j][e] / S;
                }
        }
        if (out_h != nullptr && lane == 0) out_h[pos] = h;
    }
    if (lane == 0) {
        wsum[wave] = hsum;
        wsum[4 + wave] = nbad;
    }
    __syncthreads();
    double* dst = part + seg * (C + 2);
    for (int k = tid; k < C; k += 256) dst[k] = ((cs_lds[k] + cs_lds[C + k]) + cs_lds[2 * C + k]) + cs_lds[3 * C + k];
    if (tid == 0) {
        dst[C] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        dst[C + 1] = ((wsum[4] + wsum[5]) + wsum[6]) + wsum[7];
    }
}

// out_rec[b] = { (1 / n_b) sum h, m_b, log IS_b, non-finite rows }; the first three NaN when the fourth is not 0
__global__ void __launch_bounds__(256)
cs_groups_kernel(const double* __restrict__ part, int C, const int64_t* __restrict__ offs, const int64_t* __restrict__ gseg,
                 double* __restrict__ out_rec) {
    __shared__ double red[4], tail[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int64_t s0 = gseg[b], s1 = gseg[b + 1];
    const double nd = (double)(offs[b + 1] - offs[b]);
    double m = 0.0;
    for (int k = tid; k < C + 2; k += 256) {
        double acc = 0.0;
#pragma unroll 4
        for (int64_t s = s0; s < s1; ++s) acc += part[s * (C + 2) + k];
        if (k < C) {
            const double pbar = acc / nd;
            m += pbar > 0.0 ? pbar * log(pbar) : 0.0;
        } else {
            tail[k - C] = acc;
        }
    }
    m = cs_wave_sum(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    if (tid == 0) {
        const double mb = (red[0] + red[1]) + (red[2] + red[3]);
        const double hmean = tail[0] / nd, nbad = tail[1];
        const double nan = __builtin_nan("");
        double* rec = out_rec + (int64_t)b * 4;
        rec[0] = nbad != 0.0 ? nan : hmean;
        rec[1] = nbad != 0.0 ? nan : mb;
        rec[2] = nbad != 0.0 ? nan : hmean - mb;
        rec[3] = nbad;
    }
}

// ---------------------------------------------------------------- row pairs
// f(a, b) for every column of the pair in this lane's order: chunks ascending, the four of a chunk ascending
template <class T, class F>
__device__ __forceinline__ void cs_pair_loop(const T* __restrict__ a, const T* __restrict__ b, int C, int lane, F&& f) {
    for (int k = 4 * lane; k < C; k += 256) {
        double av[4], bv[4];
        cs_load4(a, k, C, 0.0, av);
        cs_load4(b, k, C, 0.0, bv);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k + e < C) f(av[e], bv[e]);
    }
}

// s(x), 1 - s(x) and their logarithms in the stable forms: log s(x) = min(x, 0) - log1p(exp(-|x|)), log(1 - s(x)) = log s(-x)
struct CsSigmoid {
    double s, ns, ls, lns;
    __device__ __forceinline__ explicit CsSigmoid(double x) {
        const double z = exp(-fabs(x));
        const double l1p = log1p(z), den = 1.0 + z;
        const double big = 1.0 / den, small = z / den;
        s = x >= 0.0 ? big : small;
        ns = x >= 0.0 ? small : big;
        if (x != x) s = ns = x;
        ls = fmin(x, 0.0) - l1p;
        lns = fmin(-x, 0.0) - l1p;
    }
};

// a mode: row(cand, ref, C, lane, eps) -> the pair's value, the same in every lane
struct CsCosine {
    template <class T>
    static __device__ __forceinline__ double row(const T* a, const T* b, int C, int lane, double) {
        double dot = 0.0, na = 0.0, nb = 0.0;
        cs_pair_loop(a, b, C, lane, [&](double x, double y) {
            dot = fma(x, y, dot);
            na = fma(x, x, na);
            nb = fma(y, y, nb);
        });
        dot = cs_wave_sum(dot);
        na = cs_wave_sum(na);
        nb = cs_wave_sum(nb);
        return (na == 0.0 || nb == 0.0) ? __builtin_nan("") : dot / sqrt(na * nb);
    }
};

struct CsKlSoftmax {
    template <class T>
    static __device__ __forceinline__ double row(const T* cand, const T* ref, int C, int lane, double eps) {
        const double ninf = -__builtin_inf();
        double mr = ninf, mc = ninf;
        bool bad = false;
        cs_pair_loop(cand, ref, C, lane, [&](double c, double r) {
            bad |= c != c || r != r || c == __builtin_inf() || r == __builtin_inf();
            mr = fmax(mr, r);
            mc = fmax(mc, c);
        });
        mr = cs_wave_max(mr);
        mc = cs_wave_max(mc);
        if (__any(bad) || mr == ninf || mc == ninf) return __builtin_nan("");
        double sr = 0.0, sc = 0.0;
        cs_pair_loop(cand, ref, C, lane, [&](double c, double r) {
            sr += exp(r - mr);
            sc += exp(c - mc);
        });
        sr = cs_wave_sum(sr);
        sc = cs_wave_sum(sc);
        const double lsr = log(sr), lsc = log(sc);
        double v = 0.0;
        cs_pair_loop(cand, ref, C, lane, [&](double c, double r) {
            const double dr = r - mr, dc = c - mc;
            const double er = exp(dr);
            if (er == 0.0) return;                                          // p^r_c = 0: the term is 0
            const double lq = eps == 0.0 ? dc - lsc : log(exp(dc) / sc + eps);
            v += (er / sr) * ((dr - lsr) - lq);
        });
        return cs_wave_sum(v);
    }
};

struct CsKlSigmoid {
    template <class T>
    static __device__ __forceinline__ double row(const T* cand, const T* ref, int C, int lane, double eps) {
        double v = 0.0;
        cs_pair_loop(cand, ref, C, lane, [&](double c, double r) {
            const CsSigmoid p(r), q(c);
            const double lq = eps == 0.0 ? q.ls : log(q.s + eps);
            v += p.s == 0.0 ? 0.0 : p.s * (p.ls - lq);
        });
        return cs_wave_sum(v);
    }
};

struct CsKlBernoulli {
    template <class T>
    static __device__ __forceinline__ double row(const T* cand, const T* ref, int C, int lane, double eps) {
        double v = 0.0;
        cs_pair_loop(cand, ref, C, lane, [&](double c, double r) {
            const CsSigmoid p(r), q(c);
            const double lq = eps == 0.0 ? q.ls : log(q.s + eps), lnq = eps == 0.0 ? q.lns : log(q.ns + eps);
            const double t1 = p.s == 0.0 ? 0.0 : p.s * (p.ls - lq), t0 = p.ns == 0.0 ? 0.0 : p.ns * (p.lns - lnq);
            v += t1 + t0;
        });
        return cs_wave_sum(v);
    }
};

template <class T, class Mode>
__global__ void __launch_bounds__(256)
cs_pairs_kernel(const T* __restrict__ A, int64_t lda, const T* __restrict__ Bm, int64_t ldb, int64_t N, int C, double eps,
                double* __restrict__ rows_out, double* __restrict__ partials) {
    __shared__ double vals[CS_SEG];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * CS_SEG;
    for (int r = wave; r < CS_SEG; r += 4) {
        const int64_t row = row0 + r;
        if (row >= N) break;
        const double v = Mode::row(A + row * lda, Bm + row * ldb, C, lane, eps);
        if (lane == 0) vals[r] = v;
    }
    __syncthreads();
    if (wave == 0) {
        const int64_t row = row0 + lane;
        const bool valid = row < N;
        const double v = valid ? vals[lane] : 0.0;
        const bool fin = v - v == 0.0;
        if (valid && rows_out != nullptr) rows_out[row] = v;
        double s1 = (valid && fin) ? v : 0.0, s2 = (valid && fin) ? __dmul_rn(v, v) : 0.0;
        double nf = (valid && fin) ? 1.0 : 0.0, nn = (valid && !fin) ? 1.0 : 0.0;
        s1 = cs_wave_sum(s1);
        s2 = cs_wave_sum(s2);
        nf = cs_wave_sum(nf);
        nn = cs_wave_sum(nn);
        if (lane == 0) {
            double* p = partials + (int64_t)blockIdx.x * 4;
            p[0] = s1; p[1] = s2; p[2] = nf; p[3] = nn;
        }
    }
}

// sums[q] = sum over the workgroups' partials: thread-strided, xor butterfly, the four waves in order
__global__ void __launch_bounds__(256)
cs_sums_kernel(const double* __restrict__ partials, int64_t nwg, double* __restrict__ sums) {
    __shared__ double red[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t w = tid; w < nwg; w += 256)
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] += partials[w * 4 + q];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        s[q] = cs_wave_sum(s[q]);
        if (lane == 0) red[wave][q] = s[q];
    }
    __syncthreads();
    if (tid < 4) sums[tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// ---------------------------------------------------------------- host side
struct ClassBuffers {
    GroupHead head;
    int64_t* gseg;
    double* part;
    int64_t nseg_max;
};

// sum ceil(n_b / 64) <= (n_total + 63 B) / 64
static bool carve_class(Carver& c, int64_t n_total, int B, int C, ClassBuffers& w) {
    w.head = carve_group_head(c, B, ((size_t)B + 1) * 8);
    w.gseg = reinterpret_cast<int64_t*>(w.head.tail);
    w.nseg_max = (n_total + (int64_t)63 * B) / CS_SEG;
    w.part = c.take<double>((size_t)w.nseg_max * ((size_t)C + 2));
    return c.ok();
}

template <class T, int CH>
static int launch_class_rows(int64_t nseg, size_t lds, hipStream_t st, const T* X, int64_t N, int64_t ld, int C, const int64_t* idx,
                             const ClassBuffers& w, int B, double* out_h) {
    AM_HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(&cs_rows_kernel<T, CH>), CS_LDS_MAX));
    hipLaunchKernelGGL((cs_rows_kernel<T, CH>), dim3((unsigned)nseg), dim3(256), lds, st, X, N, ld, C, idx, (const int64_t*)w.head.offs,
                       (const int64_t*)w.gseg, B, w.part, out_h, w.head.flag);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

template <class T>
static int class_groups(const T* X, int64_t N, int64_t ld, int C, const int64_t* idx, const int64_t* offsets, int B, double* out_rec,
                        double* out_h, void* ws, size_t ws_bytes, hipStream_t st) {
    AM_REQUIRE(X && offsets && out_rec, AM_ERR_BAD_ARG, "null pointer");
    AM_REQUIRE(N >= 1 && B >= 1 && C >= 1 && C <= CS_MAX_C, AM_ERR_BAD_SHAPE, "L has shape %lld x %d, B=%d (N, B >= 1, 1 <= C <= %d)",
               (long long)N, C, B, CS_MAX_C);
    AM_TRY(check_group_rows(X, N, ld, C));
    int64_t n_total;
    AM_TRY(check_group_offsets(offsets, B, 0, &n_total));
    AM_TRY(check_stored_rows(idx, n_total, N));
    int64_t nseg = 0;
    for (int b = 0; b < B; ++b) nseg += ceil_div(offsets[b + 1] - offsets[b], CS_SEG);
    AM_REQUIRE(nseg < ((int64_t)1 << 31), AM_ERR_BAD_SHAPE, "%lld rows exceed the grid", (long long)n_total);
    Carver c(ws, ws_bytes);
    ClassBuffers w;
    AM_REQUIRE(carve_class(c, n_total, B, C, w), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes, have %zu", c.off, ws_bytes);
    AM_TRY(upload_group_head(w.head, offsets, B, st));
    hipLaunchKernelGGL(cs_plan_kernel, dim3(1), dim3(256), 0, st, (const int64_t*)w.head.offs, B, w.gseg);
    AM_LAUNCH_CHECK();
    const size_t lds = ((size_t)4 * C + 8) * 8;
    const int chunks = (C + 255) / 256;
    if (chunks <= 1) AM_TRY((launch_class_rows<T, 1>(nseg, lds, st, X, N, ld, C, idx, w, B, out_h)));
    else if (chunks <= 2) AM_TRY((launch_class_rows<T, 2>(nseg, lds, st, X, N, ld, C, idx, w, B, out_h)));
    else if (chunks <= 3) AM_TRY((launch_class_rows<T, 3>(nseg, lds, st, X, N, ld, C, idx, w, B, out_h)));
    else if (chunks <= 4) AM_TRY((launch_class_rows<T, 4>(nseg, lds, st, X, N, ld, C, idx, w, B, out_h)));
    else if (chunks <= 6) AM_TRY((launch_class_rows<T, 6>(nseg, lds, st, X, N, ld, C, idx, w, B, out_h)));
    else AM_TRY((launch_class_rows<T, 8>(nseg, lds, st, X, N, ld, C, idx, w, B, out_h)));
    hipLaunchKernelGGL(cs_groups_kernel, dim3((unsigned)B), dim3(256), 0, st, (const double*)w.part, C, (const int64_t*)w.head.offs,
                       (const int64_t*)w.gseg, out_rec);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

template <class T, class Mode>
static int launch_pairs(int64_t nwg, hipStream_t st, const T* A, int64_t lda, const T* Bm, int64_t ldb, int64_t N, int C, double eps,
                        double* rows_out, double* partials) {
    hipLaunchKernelGGL((cs_pairs_kernel<T, Mode>), dim3((unsigned)nwg), dim3(256), 0, st, A, lda, Bm, ldb, N, C, eps, rows_out, partials);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

template <class T>
static int row_pairs(const T* A, int64_t lda, const T* Bm, int64_t ldb, int64_t N, int C, int mode, double eps, double* rows_out,
                     double* sums, void* ws, size_t ws_bytes, hipStream_t st) {
    AM_REQUIRE(A && Bm && sums, AM_ERR_BAD_ARG, "null pointer");
    AM_REQUIRE(mode >= AM_PAIR_COSINE && mode <= AM_PAIR_KL_BERNOULLI, AM_ERR_BAD_ARG,
               "mode=%d (AM_PAIR_COSINE, AM_PAIR_KL_SOFTMAX, AM_PAIR_KL_SIGMOID or AM_PAIR_KL_BERNOULLI)", mode);
    AM_REQUIRE(std::isfinite(eps) && eps >= 0.0, AM_ERR_BAD_ARG, "eps=%g must be finite and >= 0", eps);
    AM_REQUIRE(N >= 1 && C >= 1 && C <= CS_PAIR_MAX_C, AM_ERR_BAD_SHAPE, "the matrices have shape %lld x %d (N >= 1, 1 <= C <= %d)",
               (long long)N, C, CS_PAIR_MAX_C);
    AM_REQUIRE(lda >= C && ldb >= C, AM_ERR_BAD_ARG, "lda=%lld, ldb=%lld must be >= C=%d", (long long)lda, (long long)ldb, C);
    if (sizeof(T) == 4)
        AM_REQUIRE(aligned16(A) && aligned16(Bm) && lda % 4 == 0 && ldb % 4 == 0, AM_ERR_BAD_ARG,
                   "float32 rows must be 16-byte aligned with ld %% 4 == 0 (lda=%lld, ldb=%lld)", (long long)lda, (long long)ldb);
    const int64_t nwg = ceil_div(N, CS_SEG);
    AM_REQUIRE(nwg < ((int64_t)1 << 31), AM_ERR_BAD_SHAPE, "%lld rows exceed the grid", (long long)N);
    Carver c(ws, ws_bytes);
    double* partials = c.take<double>((size_t)nwg * 4);
    AM_REQUIRE(c.ok(), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes, have %zu", c.off, ws_bytes);
    switch (mode) {
        case AM_PAIR_COSINE: AM_TRY((launch_pairs<T, CsCosine>(nwg, st, A, lda, Bm, ldb, N, C, eps, rows_out, partials))); break;
        case AM_PAIR_KL_SOFTMAX: AM_TRY((launch_pairs<T, CsKlSoftmax>(nwg, st, A, lda, Bm, ldb, N, C, eps, rows_out, partials))); break;
        case AM_PAIR_KL_SIGMOID: AM_TRY((launch_pairs<T, CsKlSigmoid>(nwg, st, A, lda, Bm, ldb, N, C, eps, rows_out, partials))); break;
        default: AM_TRY((launch_pairs<T, CsKlBernoulli>(nwg, st, A, lda, Bm, ldb, N, C, eps, rows_out, partials))); break;
    }
    hipLaunchKernelGGL(cs_sums_kernel, dim3(1), dim3(256), 0, st, (const double*)partials, nwg, sums);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

}  // namespace am

using namespace am;

extern "C" size_t am_class_groups_workspace_bytes(int64_t n_total, int B, int C) {
    if (n_total < 1 || B < 1 || C < 1 || C > CS_MAX_C) return 0;
    Carver c(nullptr, 0);
    ClassBuffers w;
    carve_class(c, n_total, B, C, w);
    return c.off;
}

extern "C" int am_class_groups_f32(const float* L, int64_t N, int64_t ld, int C, const int64_t* idx, const int64_t* offsets, int B,
                                   double* out_rec, double* out_h, void* ws, size_t ws_bytes, am_stream_t stream) {
    return class_groups<float>(L, N, ld, C, idx, offsets, B, out_rec, out_h, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int am_class_groups_f64(const double* L, int64_t N, int64_t ld, int C, const int64_t* idx, const int64_t* offsets, int B,
                                   double* out_rec, double* out_h, void* ws, size_t ws_bytes, am_stream_t stream) {
    return class_groups<double>(L, N, ld, C, idx, offsets, B, out_rec, out_h, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" size_t am_row_pairs_workspace_bytes(int64_t N) {
    if (N < 1) return 0;
    Carver c(nullptr, 0);
    c.take<double>((size_t)ceil_div(N, CS_SEG) * 4);
    return c.off;
}

extern "C" int am_row_pairs_f32(const float* cand, int64_t ldc, const float* ref, int64_t ldr, int64_t N, int C, int mode, double eps,
                                double* rows_out, double* sums, void* ws, size_t ws_bytes, am_stream_t stream) {
    return row_pairs<float>(cand, ldc, ref, ldr, N, C, mode, eps, rows_out, sums, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int am_row_pairs_f64(const double* cand, int64_t ldc, const double* ref, int64_t ldr, int64_t N, int C, int mode, double eps,
                                double* rows_out, double* sums, void* ws, size_t ws_bytes, am_stream_t stream) {
    return row_pairs<double>(cand, ldc, ref, ldr, N, C, mode, eps, rows_out, sums, ws, ws_bytes, static_cast<hipStream_t>(stream));
}
