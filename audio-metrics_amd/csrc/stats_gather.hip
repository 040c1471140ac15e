// Means and unbiased covariances of B index-gathered subsets of one stored matrix (am_stats_gather_f32 / _f64): subset b is
// the rows X[idx[offsets[b] + j]], j < n_b.  No gathered copy is made - every kernel reads the rows it is told through the
// index list - and ONE call covers all B subsets with a fixed number of launches: the concatenated index list is cut into
// chunks of R rows that never straddle a subset (subset b owns ceil(n_b / R) consecutive chunks), and a workgroup finds
// its (subset, chunk) from the device copy of the offsets.
//
//   pass 1  column sums per chunk in f64, rows read whole (D * 4 contiguous bytes); every index is checked against [0, N)
//           here: a row outside is never dereferenced, its position is left in the flag word at the start of the workspace
//   pass 2  means[b] = (sum of the subset's chunk sums, in chunk order) / n_b
//   pass 3  centred scatter per (chunk, upper-triangular tile): the arithmetic of am_stats_f32 - x - (float)mean in f32,
//           products on v_mfma_f32_32x32x2_f32 in chains of 256 rows, the chains added in f64 (float64 rows: every
//           step in f64 on v_mfma_f64_16x16x4_f64, as am_stats_f64)
//   pass 4  covs[b] = (sum of the subset's partial tiles, in chunk order) / (n_b - 1), mirrored; n_b == 1 -> 0
// All sums run in a fixed order: the result is deterministic for a given index list.
#include "am_common.h"
#include "groups_common.h"
#include "tile_engine.h"
#include <algorithm>
#include <vector>

namespace am {

constexpr int SG_ROWS = 16;          // gathered rows per stage
constexpr int SG_Q = SG_ROWS / 8;    // rows a thread stages per operand
constexpr int SG_LD = 128;           // LDS slab row stride (floats)
constexpr int SG_SLAB = SG_ROWS * SG_LD;
constexpr int SG_FLUSH = 16;         // stages per f32 chain (256 rows, as am_stats_f32)
constexpr int SG64_TILE = 32;

typedef double sg_f64x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void sg_tri_decode(int t, int T, int& tp, int& tq) {   // t-th pair with tp <= tq
    tp = 0;
    int rem = t;
    while (rem >= T - tp) { rem -= T - tp; ++tp; }
    tq = tp + rem;
}

// chunk -> (subset, position of its first index, number of rows).  Wave-uniform scalar scan over the B offsets.
struct SgChunk {
    int set;
    int64_t pos0, cnt;
};
__device__ __forceinline__ SgChunk sg_locate(const int64_t* __restrict__ offs, int B, int64_t R, int64_t chunk) {
    SgChunk c{0, 0, 0};
    int64_t first = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t n = offs[b + 1] - offs[b];
        const int64_t nch = (n + R - 1) / R;
        if (chunk < first + nch) {
            const int64_t r0 = (chunk - first) * R;
            c.set = b;
            c.pos0 = offs[b] + r0;
            c.cnt = n - r0 < R ? n - r0 : R;
            return c;
        }
        first += nch;
    }
    return c;                        // (not reached: the grid holds exactly the chunks of the B subsets)
}
// first chunk and chunk count of subset b
__device__ __forceinline__ void sg_chunks_of(const int64_t* __restrict__ offs, int b, int64_t R, int64_t& first, int64_t& nch, int64_t& n) {
    first = 0;
    for (int s = 0; s < b; ++s) first += (offs[s + 1] - offs[s] + R - 1) / R;
    n = offs[b + 1] - offs[b];
    nch = (n + R - 1) / R;
}

// ---------------------------------------------------------------- pass 1: column sums of a chunk, index validation
// VEC columns per thread (4 floats = one 16-byte load; float64 rows carry no alignment rule: 1)
template <class T, int VEC>
__global__ void __launch_bounds__(256) sg_colsum_kernel(const T* __restrict__ X, int64_t N, int64_t ld, int D, const int64_t* __restrict__ idx,
                                                        const int64_t* __restrict__ offs, int B, int64_t R, double* __restrict__ partial,
                                                        unsigned long long* __restrict__ flag) {
    __shared__ double red[256 * VEC];
    const int tid = threadIdx.x;
    const SgChunk ch = sg_locate(offs, B, R, blockIdx.x);
    const int cgs = (D + VEC - 1) / VEC;
    const int cpp = cgs < 256 ? cgs : 256;
    const int rpar = 256 / cpp;
    const int my_cg = tid % cpp, my_r = tid / cpp;
    for (int cg0 = 0; cg0 < cgs; cg0 += cpp) {
        const int cg = cg0 + my_cg;
        double s[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) s[e] = 0.0;
        if (cg < cgs && my_r < rpar) {
            for (int64_t j0 = my_r; j0 < ch.cnt; j0 += 4 * rpar) {      // four rows in flight per thread, summed in row order
                T v[4][VEC];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t j = j0 + (int64_t)u * rpar;
                    const int64_t row = j < ch.cnt ? idx[ch.pos0 + j] : 0;
                    const bool ok = j < ch.cnt && (unsigned long long)row < (unsigned long long)N;
                    if (j < ch.cnt && !ok && cg == 0) atomicMax(flag, (unsigned long long)(ch.pos0 + j) + 1ull);
                    const T* p = X + (ok ? row : 0) * ld;
                    if constexpr (VEC == 4) {
                        const f32x4 w = load_k4(ok ? reinterpret_cast<const float*>(p) : nullptr, cg * 4, D);
                        v[u][0] = w.x; v[u][1] = w.y; v[u][2] = w.z; v[u][3] = w.w;
                    } else {
#pragma unroll
                        for (int e = 0; e < VEC; ++e) v[u][e] = (ok && cg * VEC + e < D) ? p[cg * VEC + e] : T(0);
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int e = 0; e < VEC; ++e) s[e] += (double)v[u][e];
            }
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) red[tid * VEC + e] = s[e];
        __syncthreads();
        if (my_r == 0 && cg < cgs) {
            for (int rr = 1; rr < rpar; ++rr)
#pragma unroll
                for (int e = 0; e < VEC; ++e) s[e] += red[(rr * cpp + my_cg) * VEC + e];
            double* out = partial + (int64_t)blockIdx.x * D + cg * VEC;
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                if (cg * VEC + e < D) out[e] = s[e];
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- pass 2: means[b][d] = sum over the subset's chunks / n_b
__global__ void __launch_bounds__(256) sg_mean_kernel(const double* __restrict__ partial, const int64_t* __restrict__ offs, int64_t R, int D,
                                                      double* __restrict__ means) {
    const int b = blockIdx.y;
    const int d = blockIdx.x * 256 + threadIdx.x;
    int64_t first, nch, n;
    sg_chunks_of(offs, b, R, first, nch, n);
    if (d >= D) return;
    double s = 0.0;
    for (int64_t c = 0; c < nch; ++c) s += partial[(first + c) * D + d];
    means[(int64_t)b * D + d] = s / (double)n;
}

// ---------------------------------------------------------------- pass 3 (float32 rows): centred scatter of a chunk
// Workgroup = (chunk, upper-triangular 128 x 128 tile).  The scatter of am_stats_f32 with the row addresses taken from the
// index list: a thread stages 2 rows x one float4 column group per operand and stage, the indices of the next stage are
// fetched one stage ahead of the rows they name, and the rows' values are first touched after the stage's MFMAs.  Stages
// are 16 rows, half of am_stats_f32's: the indices and row offsets in flight have to fit beside the 128 f64 accumulator
// registers at two waves per SIMD.
__global__ void __launch_bounds__(ENGINE_THREADS, 2)
sg_scatter_kernel(const float* __restrict__ X, int64_t N, int64_t ld, int D, const int64_t* __restrict__ idx,
                  const int64_t* __restrict__ offs, int B, int64_t R, const double* __restrict__ means, int ntri,
                  double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float lds[4 * SG_SLAB];    // [2 stages][A slab, B slab]
    const LaneInfo L;
    const int T = (D + TB - 1) / TB;
    const int tri = blockIdx.x % ntri;
    const int64_t chunk = blockIdx.x / ntri;
    const SgChunk ch = sg_locate(offs, B, R, chunk);
    const double* mean = means + (int64_t)ch.set * D;
    int tp, tq;
    sg_tri_decode(tri, T, tp, tq);
    const int nstages = (int)((ch.cnt + SG_ROWS - 1) / SG_ROWS);

    const int srow = L.tid >> 5, sc4 = (L.tid & 31) * 4;
    const int colA = tp * TB + sc4, colB = tq * TB + sc4;
    f32x4 muA, muB;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        muA[e] = (float)mean[colA + e < D ? colA + e : D - 1];
        muB[e] = (float)mean[colB + e < D ? colB + e : D - 1];
    }
    // column groups past the row are read from column 0 and masked in commit(); rows past the chunk and rows whose index is
    // outside [0, N) are read from row 0 and masked likewise
    // (the host side admits matrices below 4 GiB here: a row's address is the uniform base plus ONE 32-bit element offset per
    // lane, and the index of a row fits 32 bits - with 64-bit addresses and indices in flight the kernel does not fit the
    // 256 registers of two waves per SIMD)
    const unsigned ldA = colA + 3 < ld ? colA : 0, ldB = colB + 3 < ld ? colB : 0;
    const unsigned ldu = (unsigned)ld;
    f32x4 ra[SG_Q], rb[SG_Q];
    unsigned rok = 0;                                   // bit q: row q of the stage in registers exists
    int next_row[SG_Q];                                 // -1: past the chunk or outside [0, N)
    auto fetch_idx = [&](int st) {
#pragma unroll
        for (int q = 0; q < SG_Q; ++q) {
            const int64_t j = (int64_t)st * SG_ROWS + q * 8 + srow;
            const int64_t row = j < ch.cnt ? idx[ch.pos0 + j] : -1;
            next_row[q] = (unsigned long long)row < (unsigned long long)N ? (int)row : -1;
        }
    };
    auto issue = [&](int st) {
        rok = 0;
#pragma unroll
        for (int q = 0; q < SG_Q; ++q) {
            const bool ok = next_row[q] >= 0;
            rok |= ok ? 1u << q : 0u;
            const unsigned base = ok ? (unsigned)next_row[q] * ldu : 0u;
            ra[q] = *reinterpret_cast<const f32x4*>(X + (base + ldA));
            rb[q] = *reinterpret_cast<const f32x4*>(X + (base + ldB));
        }
        if (st + 1 < nstages) fetch_idx(st + 1);
    };
    const bool fullA = colA + 3 < D, fullB = colB + 3 < D;
    auto centre = [&](const f32x4& v, const f32x4& mu, int col, bool full, bool row_ok) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (row_ok && (full || col + e < D)) ? v[e] - mu[e] : 0.f;
        return o;
    };
    auto commit = [&](int st) {
        float* s = lds + (st & 1) * 2 * SG_SLAB + srow * SG_LD + sc4;
#pragma unroll
        for (int q = 0; q < SG_Q; ++q) {
            *reinterpret_cast<f32x4*>(s + q * 8 * SG_LD) = centre(ra[q], muA, colA, fullA, (rok >> q) & 1u);
            *reinterpret_cast<f32x4*>(s + SG_SLAB + q * 8 * SG_LD) = centre(rb[q], muB, colB, fullB, (rok >> q) & 1u);
        }
    };

    f32x16 acc[2][2];
    zero_acc(acc);
    double acc64[2][2][16];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc64[a][b][i] = 0.0;

    if (nstages > 0) {
        fetch_idx(0);
        issue(0);
        commit(0);
    }
    __syncthreads();
    for (int st = 0; st < nstages; ++st) {
        const bool more = st + 1 < nstages;
        if (more) issue(st + 1);
        const float* sA = lds + (st & 1) * 2 * SG_SLAB + L.wm * 64 + L.r;
        const float* sB = sA - L.wm * 64 + SG_SLAB + L.wn * 64;
#pragma unroll
        for (int ks = 0; ks < SG_ROWS / 2; ++ks) {
            const int o = (ks * 2 + L.h) * SG_LD;
            const float a0 = sA[o], a1 = sA[o + 32];
            const float b0 = sB[o], b1 = sB[o + 32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if ((st % SG_FLUSH) == SG_FLUSH - 1 || !more) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc64[a][b][i] += (double)acc[a][b][i];
            zero_acc(acc);
        }
        if (more) commit(st + 1);
        __syncthreads();
    }
    double* out = partial + (chunk * ntri + tri) * (TB * TB);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int p = L.wm * 64 + mt * 32 + (i & 3) + 8 * (i >> 2) + 4 * L.h;
                const int q = L.wn * 64 + nt * 32 + L.r;
                out[p * TB + q] = acc64[mt][nt][i];
            }
}

// ---------------------------------------------------------------- pass 3 (float64 rows)
// Workgroup = (chunk, 32 x 32 block of the upper triangle), wave w the 16 x 16 tile (w >> 1, w & 1); lane (l15, l4) feeds
// gathered row j0 + l4, column c0 + l15 straight from memory, as am_stats_f64 does for consecutive rows
__global__ void __launch_bounds__(256) sg_scatter64_kernel(const double* __restrict__ X, int64_t N, int64_t ld, int D,
                                                           const int64_t* __restrict__ idx, const int64_t* __restrict__ offs, int B,
                                                           int64_t R, const double* __restrict__ means, int ntri,
                                                           double* __restrict__ partial) {
    const int T = (D + SG64_TILE - 1) / SG64_TILE;
    const int tri = (int)(blockIdx.x % ntri);
    const int64_t chunk = blockIdx.x / ntri;
    const SgChunk ch = sg_locate(offs, B, R, chunk);
    const double* mean = means + (int64_t)ch.set * D;
    int tp, tq;
    sg_tri_decode(tri, T, tp, tq);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int ca = tp * SG64_TILE + (wave >> 1) * 16 + l15, cb = tq * SG64_TILE + (wave & 1) * 16 + l15;
    const double ma = ca < D ? mean[ca] : 0.0, mb = cb < D ? mean[cb] : 0.0;
    sg_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int64_t j0 = 0; j0 < ch.cnt; j0 += 16) {
        double a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {                             // four independent row groups in flight
            const int64_t j = j0 + u * 4 + l4;
            const int64_t row = j < ch.cnt ? idx[ch.pos0 + j] : -1;
            const bool in = (unsigned long long)row < (unsigned long long)N;
            a[u] = (in && ca < D) ? X[row * ld + ca] - ma : 0.0;
            b[u] = (in && cb < D) ? X[row * ld + cb] - mb : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
    }
    double* out = partial + (chunk * ntri + tri) * (SG64_TILE * SG64_TILE);
#pragma unroll
    for (int r = 0; r < 4; ++r) out[((wave >> 1) * 16 + l4 + 4 * r) * SG64_TILE + (wave & 1) * 16 + l15] = acc[r];
}

// ---------------------------------------------------------------- pass 4: covs[b] = sum of the subset's partial tiles / (n_b - 1)
// grid (TILE * TILE / 256, ntri, B); one thread per element of an upper-triangular tile, mirrored write.  On the diagonal
// tiles the upper triangle decides, so the result is exactly symmetric.
template <int TILE>
__global__ void __launch_bounds__(256) sg_reduce_kernel(const double* __restrict__ partial, const int64_t* __restrict__ offs, int64_t R,
                                                        int ntri, int D, double* __restrict__ covs) {
    const int T = (D + TILE - 1) / TILE;
    const int tri = blockIdx.y, b = blockIdx.z;
    int tp, tq;
    sg_tri_decode(tri, T, tp, tq);
    int64_t first, nch, n;
    sg_chunks_of(offs, b, R, first, nch, n);
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int i = tp * TILE + e / TILE, j = tq * TILE + e % TILE;
    if (i >= D || j >= D) return;
    const int64_t step = (int64_t)ntri * (TILE * TILE);
    const double* src = partial + (first * ntri + tri) * (TILE * TILE) + e;
    double s = 0.0;
    int64_t c = 0;
    for (; c + 7 < nch; c += 8) {                  // eight loads in flight, summed in chunk order
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(c + u) * step];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; c < nch; ++c) s += src[c * step];
    s = n > 1 ? s * (1.0 / (double)(n - 1)) : 0.0;                 // one row -> zero covariance (data.py:40-42)
    double* out = covs + (int64_t)b * D * D;
    if (tp != tq || j >= i) out[(int64_t)i * D + j] = s;
    if (tp != tq || j > i) out[(int64_t)j * D + i] = s;
}

// ---------------------------------------------------------------- host side
struct GatherPlan {
    int64_t R;                 // rows per chunk
    int64_t max_chunks;        // bound on sum_b ceil(n_b / R) that needs only n_total and B
    int ntri, tile;
};

// float32: about four workgroups per CU in all (two resident at a time) and at least one full f32 chain per chunk;
// float64: about sixteen of the small workgroups per CU
static GatherPlan plan_gather(int64_t n_total, int B, int D, bool f64) {
    GatherPlan p;
    p.tile = f64 ? SG64_TILE : TB;
    const int T = (int)ceil_div(D, p.tile);
    p.ntri = T * (T + 1) / 2;
    const int64_t want_wg = f64 ? 4096 : 1024;
    const int64_t unit = SG_ROWS * SG_FLUSH;
    p.R = std::max<int64_t>(ceil_div(ceil_div(n_total * p.ntri, want_wg), unit) * unit, unit);
    p.max_chunks = n_total / p.R + B;
    return p;
}

struct GatherBuffers {
    GroupHead head;
    double *cs_part, *sc_part;
};

static bool carve_gather(Carver& c, int B, int D, const GatherPlan& p, GatherBuffers& g) {
    g.head = carve_group_head(c, B);
    g.cs_part = c.take<double>((size_t)p.max_chunks * D);
    g.sc_part = c.take<double>((size_t)p.max_chunks * p.ntri * p.tile * p.tile);
    return c.ok();
}

template <class T>
static int stats_gather(const T* X, int64_t N, int64_t ld, int D, const int64_t* idx, const int64_t* offsets, int B, double* means,
                        double* covs, void* ws, size_t ws_bytes, hipStream_t st) {
    constexpr bool F64 = sizeof(T) == 8;
    AM_REQUIRE(X && idx && offsets && means && covs, AM_ERR_BAD_ARG, "null pointer");
    AM_REQUIRE(N >= 1 && D >= 1 && B >= 1 && B <= 65535, AM_ERR_BAD_SHAPE, "X has shape %lld x %d, B=%d (1 <= B <= 65535)",
               (long long)N, D, B);
    AM_TRY(check_group_rows(X, N, ld, D));
    int64_t n_total;
    AM_TRY(check_group_offsets(offsets, B, 0, &n_total));
    const GatherPlan p = plan_gather(n_total, B, D, F64);
    int64_t chunks = 0;
    for (int b = 0; b < B; ++b) chunks += ceil_div(offsets[b + 1] - offsets[b], p.R);
    AM_REQUIRE(chunks * p.ntri < (int64_t)1 << 31 && p.ntri <= 65535, AM_ERR_BAD_SHAPE, "%lld chunks x %d tiles exceed the grid",
               (long long)chunks, p.ntri);
    Carver c(ws, ws_bytes);
    GatherBuffers g;
    AM_REQUIRE(carve_gather(c, B, D, p, g), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes, have %zu", c.off, ws_bytes);
    AM_TRY(upload_group_head(g.head, offsets, B, st));
    const int64_t* offs = g.head.offs;
    hipLaunchKernelGGL((sg_colsum_kernel<T, F64 ? 1 : 4>), dim3((unsigned)chunks), dim3(256), 0, st, X, N, ld, D, idx,
                       offs, B, p.R, g.cs_part, g.head.flag);
    AM_LAUNCH_CHECK();
    hipLaunchKernelGGL(sg_mean_kernel, dim3((unsigned)ceil_div(D, 256), (unsigned)B), dim3(256), 0, st, (const double*)g.cs_part,
                       offs, p.R, D, means);
    AM_LAUNCH_CHECK();
    if constexpr (F64) {
        hipLaunchKernelGGL(sg_scatter64_kernel, dim3((unsigned)(chunks * p.ntri)), dim3(256), 0, st, X, N, ld, D, idx,
                           offs, B, p.R, (const double*)means, p.ntri, g.sc_part);
        AM_LAUNCH_CHECK();
        hipLaunchKernelGGL(sg_reduce_kernel<SG64_TILE>, dim3(SG64_TILE * SG64_TILE / 256, (unsigned)p.ntri, (unsigned)B), dim3(256), 0,
                           st, (const double*)g.sc_part, offs, p.R, p.ntri, D, covs);
    } else {
        hipLaunchKernelGGL(sg_scatter_kernel, dim3((unsigned)(chunks * p.ntri)), dim3(ENGINE_THREADS), 0, st, X, N, ld, D, idx,
                           offs, B, p.R, (const double*)means, p.ntri, g.sc_part);
        AM_LAUNCH_CHECK();
        hipLaunchKernelGGL(sg_reduce_kernel<TB>, dim3(TB * TB / 256, (unsigned)p.ntri, (unsigned)B), dim3(256), 0, st,
                           (const double*)g.sc_part, offs, p.R, p.ntri, D, covs);
    }
    AM_LAUNCH_CHECK();
    return AM_OK;
}

}  // namespace am

using namespace am;

extern "C" size_t am_stats_gather_workspace_bytes(int64_t n_total, int B, int D) {
    if (n_total < 1 || B < 1 || D < 1) return 0;
    size_t need = 0;
    for (int f64 = 0; f64 < 2; ++f64) {                    // one query for both row types: the larger of the two layouts
        Carver c(nullptr, 0);
        GatherBuffers g;
        carve_gather(c, B, D, plan_gather(n_total, B, D, f64 != 0), g);
        need = std::max(need, c.off);
    }
    return need;
}

extern "C" int am_stats_gather_f32(const float* X, int64_t N, int64_t ld, int D, const int64_t* idx, const int64_t* offsets, int B,
                                   double* means, double* covs, void* ws, size_t ws_bytes, am_stream_t stream) {
    return stats_gather<float>(X, N, ld, D, idx, offsets, B, means, covs, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int am_stats_gather_f64(const double* X, int64_t N, int64_t ld, int D, const int64_t* idx, const int64_t* offsets, int B,
                                   double* means, double* covs, void* ws, size_t ws_bytes, am_stream_t stream) {
    return stats_gather<double>(X, N, ld, D, idx, offsets, B, means, covs, ws, ws_bytes, static_cast<hipStream_t>(stream));
}
