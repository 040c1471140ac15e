// Random Fourier features of the Gaussian kernel and their moment matrix (FKEA: Ospanov et al., NeurIPS 2024): the spectrum
// of K / n for n rows, K_ij = exp(-|x_i - x_j|^2 / (2 bw^2)), from a [2R][2R] matrix instead of an [n][n] one.
//
//   W        [R][D] float32 frequencies: a unit-bandwidth standard normal draw, independent of the bandwidth
//   z_il   = <w_l, x_i>                  f32 on the exact tile engine (the k order of tile_engine.h)
//   a_il   = (double) z_il * inv_bw      inv_bw = 1 / bw in f64: the host double, or 1 / sqrt((double) *bw2_dev) for the float32
//                                        DEVICE scalar of a median squared distance (am_pairwise_select_f32) - no host round trip
//   phi_i  = R^(-1/2) [cos a_i1 .. cos a_iR, sin a_i1 .. sin a_iR]     cos and sin in f64
//            <phi_i, phi_j> is an unbiased estimate of K_ij, |phi_i|^2 = 1
//   S      = (1 / n) sum_i phi_i phi_i^T     [2R][2R] f64, trace 1; its non-zero eigenvalues are those of Phi Phi^T / n ~ K / n
//
// FEATURES (am_rff_features_f32): F[l][i] = cos(a_il) / sqrt(R), F[R + l][i] = sin(a_il) / sqrt(R) for the rows [row0, row0 +
// nrows), feature-major with row stride ldo, i counted from row0.  The eighth epilogue of the exact f32 tile engine on the plan
// of swd.hip's projection (dense_pipeline_early with the production schedule, work_item / choose_chunks, the KTAIL
// instantiation for D % 32 != 0), the frequencies on the Q side and the rows of X on the P side: the lane index runs along rows
// of X, so finish() turns every accumulator register into two runs of 32 consecutive doubles per half-wave.  The bits of z do
// not depend on the tile position and cos / sin are functions of a alone: a feature has the same bits alone and among any
// other frequencies, and for any (row0, nrows) that covers its row.  A row with a NaN or an infinity writes zeros and is
// counted in the int64 at the head of the workspace (one wave per row looks at it before the tiles run).
//
// MOMENT (am_rff_moment_f32): the rows are cut into chunks of RFF_CHUNK_ROWS.  Per chunk: the features go to a workspace
// buffer [2R][chunk]; the Gram of that feature-major buffer runs on v_mfma_f64_16x16x4_f64 through f64_tile - "rows" of the
// engine = features, inner index = row of X, contiguous here, so nothing is transposed; workgroup = (upper 64 x 64 tile of S,
// split of the chunk's rows), every workgroup writes its own 64 x 64 partial; one workgroup per tile then adds the splits in
// split order to what S holds from the chunks before.  The last chunk's fold divides by n and writes the mirror: S is exactly
// symmetric.  Chunks run in stream order, so the sum is in chunk order; no floating-point atomics anywhere (the only atomic is
// the integer count of non-finite rows): two calls return the same bits.  The workspace is the feature buffer, the partials
// and the row flags of ONE chunk: it does not grow with n past RFF_CHUNK_ROWS rows.
#include "row_sweep.h"
#include "f64_engine.h"
#include <algorithm>
#include <cmath>

namespace am {
namespace rff {

constexpr size_t FEATURE_LDS_BYTES = ENGINE_LDS_FLOATS * sizeof(float);
static_assert(2 * FEATURE_LDS_BYTES <= 160 * 1024, "__launch_bounds__(ENGINE_THREADS, 2): two workgroups share the 160 KiB of a CU");
constexpr int MAX_FEATURES = 1024;        // R: the 2048 x 2048 eigenproblem is what am_eigh_sym_f64 is used with
constexpr int64_t CHUNK_ROWS = 4096;      // rows of X per chunk of the moment: [2R][4096] doubles = 64 MiB at R = 1024
constexpr int FLAG_THREADS = 256;

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// one wave per row i of [0, nrows): bad[i] = 1 if the row holds a NaN or an infinity, and the count of such rows
__global__ void __launch_bounds__(FLAG_THREADS)
rff_rowflag_kernel(const float* __restrict__ X, int64_t nrows, int64_t ldx, int D, int* __restrict__ bad,
                   unsigned long long* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (FLAG_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= nrows) return;
    const float* x = X + i * ldx;
    bool b = false;
    for (int k = lane; k < D; k += 64) b |= !finite_bits(x[k]);
    const bool any = __builtin_amdgcn_ballot_w64(b) != 0ull;
    if (lane == 0) {
        bad[i] = any ? 1 : 0;
        if (any) atomicAdd(count, 1ull);
    }
}

// sin and cos of one f64 argument in registers alone (the library routine's large-argument path keeps a table on the stack,
// which the tile kernel cannot afford 64 times per lane).  Cody-Waite reduction by n = rint(a 2 / pi) with pi / 2 as three
// doubles - the first product is exact in the fma, the second is carried as a (head, tail) pair - and the two polynomial
// kernels of fdlibm (k_sin.c / k_cos.c) on the reduced pair.  Measured against long double on 1.2e7 arguments up to 5e8:
// |error| <= 0.78 * 2^-53 for either function.  |a| >= 2^30 (or not finite) gives NaN: the float32 projection behind such an
// argument has an ulp of more than 2 pi in a, so there is no phase left to evaluate.
__device__ __forceinline__ void sincos_f64(double a, double& sn, double& cs) {
#pragma clang fp contract(off)
    constexpr double INV_PIO2 = 6.36619772367581382433e-01;
    constexpr double P1 = 1.5707963267948966, P2 = 6.123233995736766e-17, P3 = -1.4973849048591698e-33;
    const double n = rint(a * INV_PIO2);
    const double r = __builtin_fma(-n, P1, a);
    const double w = n * P2;
    const double y0 = r - w;
    const double bb = y0 - r;
    double y1 = (r - (y0 - bb)) + (-w - bb);
    y1 -= __builtin_fma(n, P2, -w);
    y1 = __builtin_fma(-n, P3, y1);
    const double z = y0 * y0;
    const double v = z * y0;
    const double ps = 8.33333333332248946124e-03 +
                      z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)));
    const double ks = y0 - ((z * (0.5 * y1 - v * ps) - y1) - v * -1.66666666666666324348e-01);
    const double z2 = z * z;
    const double pc = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * 2.48015872894767294178e-05)) +
                      (z2 * z2) * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11));
    const double hz = 0.5 * z;
    const double wc = 1.0 - hz;
    const double kc = wc + (((1.0 - wc) - hz) + (z * pc - y0 * y1));
    const bool in_range = fabs(a) < 1073741824.0;            // false for a NaN too
    const int q = in_range ? ((int)n & 3) : 0;
    const double s0 = (q & 1) ? kc : ks, c0 = (q & 1) ? ks : kc;
    const double nan = __builtin_nan("");
    sn = !in_range ? nan : (q & 2) ? -s0 : s0;
    cs = !in_range ? nan : ((q + 1) & 2) ? -c0 : c0;
}

struct FeatureEpilogue {
    double* F;
    int64_t ldo, n, half;          // half = R ldo: the distance from a cos row to its sin row
    int R;
    double inv_bw, rs;             // rs = R^(-1/2)
    const int* bad;
    const LaneInfo& L;
    int64_t prow0;

    __device__ __forceinline__ FeatureEpilogue(const LaneInfo& l) : L(l) {}
    __device__ __forceinline__ void aux_issue(int, int64_t) {}
    __device__ __forceinline__ void aux_commit(int) {}
    // register 4 g + e of acc[mt][nt] <-> frequency qtile * 128 + wm * 64 + mt * 32 + 8 g + 4 h + e, row prow0 + wn * 64 + nt * 32 + r
    __device__ __forceinline__ void finish(int, int64_t qtile, f32x16 (&acc)[2][2]) {
        const int64_t cbase = qtile * TB + L.wm * 64 + L.h * 4;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int64_t i = prow0 + L.wn * 64 + nt * 32 + L.r;
            if (i >= n) continue;
            const bool zero = bad[i] != 0;
            double* col = F + i;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int64_t c = cbase + mt * 32 + (reg & 3) + 8 * (reg >> 2);
                    if (c < R) {
                        double s, co;
                        sincos_f64((double)acc[mt][nt][reg] * inv_bw, s, co);
                        col[c * ldo] = zero ? 0.0 : co * rs;
                        col[c * ldo + half] = zero ? 0.0 : s * rs;
                    }
                }
            }
        }
    }
};

template <bool KTAIL>
__global__ void __launch_bounds__(ENGINE_THREADS, 2)
rff_features_kernel(const float* __restrict__ X, int64_t N, int64_t ldx, const float* __restrict__ W, int R, int64_t ldw, int D,
                    int nchunks, double inv_bw, const float* __restrict__ bw2_dev, const int* __restrict__ bad,
                    double* __restrict__ F, int64_t ldo) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LaneInfo L;
    const WorkItem w = work_item(((int64_t)R + TB - 1) / TB, nchunks);
    FeatureEpilogue epi(L);
    epi.F = F;
    epi.ldo = ldo;
    epi.n = N;
    epi.half = (int64_t)R * ldo;
    epi.R = R;
    epi.inv_bw = bw2_dev != nullptr ? 1.0 / sqrt((double)*bw2_dev) : inv_bw;
    epi.rs = 1.0 / sqrt((double)R);
    epi.bad = bad;
    epi.prow0 = w.prow0;
    dense_pipeline_early<EV_DEFAULT, KTAIL>(W, (int64_t)R, ldw, LinearTiles{w.qtile0}, X, N, ldx, w.prow0, w.ntiles, D, lds, L, epi);
}

// t-th tile (tq <= tp) of the T x T upper triangle, row by row
__device__ __forceinline__ void tri_decode(int t, int T, int& tq, int& tp) {
    tq = 0;
    while (t >= T - tq) { t -= T - tq; ++tq; }
    tp = tq + t;
}

// Workgroup = (upper tile, split of the chunk's rows): partial[split][tile][64][64] = the tile of F F^T over the split's rows.
// Features past 2R are zero rows of the engine, so the whole 64 x 64 block is written.
__global__ void __launch_bounds__(FTHREADS)
rff_gram_kernel(const double* __restrict__ F, int64_t ldo, int R2, int64_t rows, int splits, int TT, int ntri,
                double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) double lds64[];
    const FLane L;
    const int split = (int)(blockIdx.x % (unsigned)splits);
    const int tile = (int)(blockIdx.x / (unsigned)splits);
    int tq, tp;
    tri_decode(tile, TT, tq, tp);
    const int64_t r0 = rows * split / splits, r1 = rows * (split + 1) / splits;
    f64x4 acc[4];
    zero4(acc);
    f64_tile(DenseRows64{F + r0, ldo, R2, (int64_t)tq * FT}, DenseRows64{F + r0, ldo, R2, (int64_t)tp * FT}, (int)(r1 - r0), lds64, L, acc);
    double* dst = partial + ((int64_t)split * ntri + tile) * (FT * FT);
    const int cb = L.prow();
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[L.qrow(mt, r) * FT + cb] = acc[mt][r];
}

// One workgroup per upper tile: S[a][b] = (first ? 0 : S[a][b]) + (the splits' partials in split order); the last chunk's call
// divides by n and writes S[b][a] too.  On a diagonal tile only a <= b.
__global__ void __launch_bounds__(256)
rff_fold_kernel(const double* __restrict__ partial, int R2, int splits, int TT, int ntri, int first, int last, double n,
                double* __restrict__ S) {
    const int tile = (int)blockIdx.x;
    int tq, tp;
    tri_decode(tile, TT, tq, tp);
    for (int e = threadIdx.x; e < FT * FT; e += 256) {
        const int a = tq * FT + e / FT, b = tp * FT + e % FT;
        if (a >= R2 || b >= R2 || (tq == tp && b < a)) continue;
        double s = 0.0;
        for (int k = 0; k < splits; ++k) s += partial[((int64_t)k * ntri + tile) * (FT * FT) + e];
        double* out = S + (int64_t)a * R2 + b;
        if (!first) s = *out + s;
        if (last) {
            s /= n;
            if (a != b) S[(int64_t)b * R2 + a] = s;
        }
        *out = s;
    }
}

// ---------------------------------------------------------------- host side
static int check_width(double inv_bw, const float* bw2_dev) {
    if (bw2_dev == nullptr)
        AM_REQUIRE(std::isfinite(inv_bw) && inv_bw > 0.0, AM_ERR_BAD_ARG, "inv_bw=%g must be finite and positive (or bw2_dev given)", inv_bw);
    return AM_OK;
}
static bool features_shape_ok(int64_t nrows, int R, int D) {
    return nrows >= 1 && R >= 1 && R <= MAX_FEATURES && D >= 1 && ceil_div(nrows, TB) * 64 < (int64_t)0x7fffffff &&
           ceil_div(nrows, FLAG_THREADS / 64) < (int64_t)0x7fffffff;
}

// the features of rows X[0 .. nrows) (the caller has moved X to its first row); `count` is not cleared here
static int launch_features(const float* X, int64_t nrows, int64_t ldx, int D, const float* W, int R, int64_t ldw, double inv_bw,
                           const float* bw2_dev, int* bad, unsigned long long* count, double* F, int64_t ldo, hipStream_t st) {
    hipLaunchKernelGGL(rff_rowflag_kernel, dim3((unsigned)ceil_div(nrows, FLAG_THREADS / 64)), dim3(FLAG_THREADS), 0, st, X, nrows, ldx, D,
                       bad, count);
    AM_LAUNCH_CHECK();
    const int nchunks = choose_chunks(nrows, R);
    return launch_sweep(&rff_features_kernel<false>, &rff_features_kernel<true>, FEATURE_LDS_BYTES, nrows, nchunks, D, st, X, nrows, ldx, W,
                        R, ldw, D, nchunks, inv_bw, bw2_dev, bad, F, ldo);
}

struct FeatureBuffers {
    unsigned long long* count;
    int* bad;
};
static bool carve_features(Carver& c, int64_t nrows, FeatureBuffers& b) {
    b.count = c.take<unsigned long long>(1);
    b.bad = c.take<int>((size_t)nrows);
    return c.ok();
}

static int64_t moment_chunk_rows(int64_t n) { return std::min<int64_t>(n, CHUNK_ROWS); }
static int64_t moment_ldo(int64_t n) { return ceil_div(moment_chunk_rows(n), 16) * 16; }
static int moment_splits(int64_t n, int R) {
    // about 1024 workgroups over the upper tiles, at least 128 rows per split
    const int64_t T_ = ceil_div(2 * (int64_t)R, FT), ntri = T_ * (T_ + 1) / 2;
    int64_t s = std::min<int64_t>(ceil_div(1024, ntri), 64);
    s = std::min<int64_t>(s, std::max<int64_t>(1, moment_chunk_rows(n) / 128));
    return (int)s;
}

struct MomentBuffers {
    FeatureBuffers f;
    double *feat, *partial;
};
static bool carve_moment(Carver& c, int64_t n, int R, MomentBuffers& m) {
    const int64_t T_ = ceil_div(2 * (int64_t)R, FT), ntri = T_ * (T_ + 1) / 2;
    carve_features(c, moment_chunk_rows(n), m.f);
    m.feat = c.take<double>((size_t)(2 * R) * (size_t)moment_ldo(n));
    m.partial = c.take<double>((size_t)moment_splits(n, R) * (size_t)ntri * FT * FT);
    return c.ok();
}

}  // namespace rff
}  // namespace am

using namespace am;

extern "C" int am_rff_max_features(void) { return rff::MAX_FEATURES; }

extern "C" size_t am_rff_features_workspace_bytes(int64_t nrows) {
    if (nrows < 1) return 0;
    Carver c(nullptr, 0);
    rff::FeatureBuffers b;
    rff::carve_features(c, nrows, b);
    return c.off;
}

extern "C" int am_rff_features_f32(const float* X, int64_t N, int64_t ldx, int D, const float* W, int R, int64_t ldw, int64_t row0,
                                   int64_t nrows, double inv_bw, const float* bw2_dev, double* F, int64_t ldo, void* ws, size_t ws_bytes,
                                   am_stream_t stream) {
    int rc;
    if ((rc = check_matrix(X, N, ldx, D, "X")) != AM_OK) return rc;
    if ((rc = check_matrix(W, R, ldw, D, "W")) != AM_OK) return rc;
    AM_REQUIRE(F != nullptr, AM_ERR_BAD_ARG, "F is null");
    AM_REQUIRE(row0 >= 0 && nrows >= 1 && row0 <= N - nrows, AM_ERR_BAD_SHAPE, "rows [%lld, %lld + %lld) are not inside [0, %lld)",
               (long long)row0, (long long)row0, (long long)nrows, (long long)N);
    AM_REQUIRE(ldo >= nrows, AM_ERR_BAD_ARG, "ldo=%lld is smaller than nrows=%lld", (long long)ldo, (long long)nrows);
    AM_REQUIRE(R <= rff::MAX_FEATURES, AM_ERR_BAD_SHAPE, "R=%d exceeds am_rff_max_features() = %d", R, rff::MAX_FEATURES);
    AM_REQUIRE(rff::features_shape_ok(nrows, R, D), AM_ERR_BAD_SHAPE, "nrows=%lld R=%d: too large for one launch", (long long)nrows, R);
    if ((rc = rff::check_width(inv_bw, bw2_dev)) != AM_OK) return rc;
    Carver c(ws, ws_bytes);
    rff::FeatureBuffers b;
    AM_REQUIRE(rff::carve_features(c, nrows, b), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (am_rff_features_workspace_bytes), have %zu",
               c.off, ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AM_HIP_TRY(hipMemsetAsync(b.count, 0, sizeof(unsigned long long), st));
    return rff::launch_features(X + row0 * ldx, nrows, ldx, D, W, R, ldw, inv_bw, bw2_dev, b.bad, b.count, F, ldo, st);
}

extern "C" int am_rff_moment_chunks(int64_t n, int R) {
    if (n < 1 || R < 1 || R > rff::MAX_FEATURES) return 0;
    return (int)ceil_div(n, rff::CHUNK_ROWS);
}

extern "C" size_t am_rff_moment_workspace_bytes(int64_t n, int D, int R) {
    if (n < 1 || D < 1 || R < 1 || R > rff::MAX_FEATURES) return 0;
    Carver c(nullptr, 0);
    rff::MomentBuffers m;
    rff::carve_moment(c, n, R, m);
    return c.off;
}

extern "C" int am_rff_moment_f32(const float* X, int64_t N, int64_t ldx, int D, const float* W, int R, int64_t ldw, double inv_bw,
                                 const float* bw2_dev, double* out_s, void* ws, size_t ws_bytes, am_stream_t stream) {
    int rc;
    if ((rc = check_matrix(X, N, ldx, D, "X")) != AM_OK) return rc;
    if ((rc = check_matrix(W, R, ldw, D, "W")) != AM_OK) return rc;
    AM_REQUIRE(out_s != nullptr, AM_ERR_BAD_ARG, "out_s is null");
    AM_REQUIRE(R <= rff::MAX_FEATURES, AM_ERR_BAD_SHAPE, "R=%d exceeds am_rff_max_features() = %d", R, rff::MAX_FEATURES);
    AM_REQUIRE(N <= ((int64_t)1 << 40), AM_ERR_BAD_SHAPE, "N=%lld rows are too many", (long long)N);
    if ((rc = rff::check_width(inv_bw, bw2_dev)) != AM_OK) return rc;
    Carver c(ws, ws_bytes);
    rff::MomentBuffers m;
    AM_REQUIRE(rff::carve_moment(c, N, R, m), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (am_rff_moment_workspace_bytes), have %zu",
               c.off, ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AM_HIP_TRY(hipMemsetAsync(m.f.count, 0, sizeof(unsigned long long), st));
    const int R2 = 2 * R;
    const int T_ = (int)ceil_div(R2, FT), ntri = T_ * (T_ + 1) / 2;
    const int splits = rff::moment_splits(N, R);
    const int64_t ldo = rff::moment_ldo(N);
    const int64_t chunks = ceil_div(N, rff::CHUNK_ROWS);
    for (int64_t ch = 0; ch < chunks; ++ch) {
        const int64_t r0 = ch * rff::CHUNK_ROWS, rows = std::min<int64_t>(rff::CHUNK_ROWS, N - r0);
        if ((rc = rff::launch_features(X + r0 * ldx, rows, ldx, D, W, R, ldw, inv_bw, bw2_dev, m.f.bad, m.f.count, m.feat, ldo, st)) != AM_OK)
            return rc;
        hipLaunchKernelGGL(rff::rff_gram_kernel, dim3((unsigned)(ntri * splits)), dim3(FTHREADS), (size_t)FENGINE_DOUBLES * 8, st,
                           (const double*)m.feat, ldo, R2, rows, splits, T_, ntri, m.partial);
        AM_LAUNCH_CHECK();
        hipLaunchKernelGGL(rff::rff_fold_kernel, dim3((unsigned)ntri), dim3(256), 0, st, (const double*)m.partial, R2, splits, T_, ntri,
                           ch == 0 ? 1 : 0, ch + 1 == chunks ? 1 : 0, (double)N, out_s);
        AM_LAUNCH_CHECK();
    }
    return AM_OK;
}
