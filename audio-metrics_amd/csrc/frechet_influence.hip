// First-order influence of every row on the Frechet distance (am_frechet_influence_f32 / _f64): with c_i = x_i - mu,
//     psi_i = c_i^T B c_i + lin^T c_i + c0,        B symmetric [D][D], f64
// where B = I - A, lin = 2 (mu_x - mu_y) for a candidate row and B = I - A^-1, lin = -2 (mu_x - mu_y) for a reference row,
// A the Gaussian optimal-transport map of am_frechet_maps_f64.  From psi follow the standard error of FAD, the two-model
// test and the per-clip attribution (metrics/fad_stats.py).
//
//   fi_rows_kernel   one workgroup owns 64 rows and walks all 64-column tiles of B: T = C B on v_mfma_f64_16x16x4_f64
//                    (wave w the 32 x 32 quarter (w >> 1, w & 1) as 2 x 2 MFMA tiles, the layout of fg_gemm_kernel), and at
//                    the end of a column tile (T + lin) o C is folded into per-row partial sums in registers.  T never
//                    reaches memory: no N x D f64 intermediate exists.  Both operands are staged per 16-deep k slab in a
//                    double-buffered LDS ring (40 KiB: one barrier per slab, the loads of the next slab are in flight
//                    while this one multiplies); float32 rows are converted on load (exact) and centred in f64, so both
//                    row types share every later bit.  The kernel is bound by the f64 matrix cores (16 MFMAs per wave and
//                    slab against 4 LDS reads per k step), so the whole 64 x D centred tile is NOT kept in LDS: 64 x 256
//                    f64 would be 128 KiB and leave one workgroup per CU; the slab ring leaves room for three.
//                    The workgroup then adds its rows into {sum psi, sum psi^2, finite rows, non-finite rows}.
//   fi_sums_kernel   one workgroup adds the per-workgroup partials in a fixed order.
// No floating-point atomics and no data-dependent order anywhere: two calls return the same bits, and a row's psi depends
// on nothing but that row, mu, B, lin and c0 (not on N, ld or its position in the tile).
#include "am_common.h"

namespace am {

constexpr int FI_TILE = 64, FI_KT = 16, FI_LDT = 80;      // tile edge, k slab, LDS row stride (f64)

typedef double fi_f64x4 __attribute__((ext_vector_type(4)));
typedef float fi_f32x4 __attribute__((ext_vector_type(4)));

// four consecutive elements k .. k + 3 of one row, as loaded.  Every load is unconditional - an index past the end is
// clamped into the row and its value masked when the slab is staged - so the loads of a slab go out together and nothing
// waits for them before the MFMAs of the slab in between.  float32 rows: one 16-byte load (rows are 16-byte aligned with
// ld % 4 == 0 and k % 4 == 0, so the load stays inside the row's ld); float64 rows: scalar loads.
template <class T> struct FiRaw;
template <> struct FiRaw<float> { fi_f32x4 v; };
template <> struct FiRaw<double> { double v[4]; };

__device__ __forceinline__ void fi_load4(const float* __restrict__ row, int k, int D, FiRaw<float>& r) {
    r.v = *reinterpret_cast<const fi_f32x4*>(row + (k < D ? k : 0));
}

__device__ __forceinline__ void fi_load4(const double* __restrict__ row, int k, int D, FiRaw<double>& r) {
#pragma unroll
    for (int e = 0; e < 4; ++e) r.v[e] = row[min(k + e, D - 1)];
}

template <class T>
__global__ void __launch_bounds__(256, 2) fi_rows_kernel(const T* __restrict__ X, int64_t N, int64_t ld, int D, const double* __restrict__ mu,
                                                         const double* __restrict__ B, const double* __restrict__ lin, double c0,
                                                         double* __restrict__ psi, double* __restrict__ partials) {
    __shared__ double As[2][FI_KT * FI_LDT];      // [k][row], centred
    __shared__ double Bs[2][FI_KT * FI_LDT];      // [k][col]
    __shared__ double red[2][FI_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t row0 = (int64_t)blockIdx.x * FI_TILE;
    const int arow = tid & 63, ak = (tid >> 6) * 4;       // staging of C: 4 consecutive k of one row
    const int bk = tid >> 4, bc = (tid & 15) * 4;         // staging of B: 4 consecutive columns of one k
    const bool arow_ok = row0 + arow < N;
    const T* pa = X + (arow_ok ? row0 + arow : 0) * ld;
    const int nslab = (D + FI_KT - 1) / FI_KT, ctiles = (D + FI_TILE - 1) / FI_TILE;
    const int steps = nslab * ctiles;

    // fetch() only issues the loads; centring and masking wait until stage(), behind the MFMAs of the slab in between
    FiRaw<T> ar;
    double am[4], bv[4];
    int ak_next = 0, bk_next = 0, bc_next = 0;
    auto fetch = [&](int step) {                          // slab (step % nslab) of C, of column tile (step / nslab) of B
        const int k0 = (step % nslab) * FI_KT, col0 = (step / nslab) * FI_TILE;
        ak_next = k0 + ak;
        bk_next = k0 + bk;
        bc_next = col0 + bc;
        fi_load4(pa, ak_next, D, ar);
        const double* pb = B + (int64_t)min(bk_next, D - 1) * D;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            am[e] = mu[min(ak_next + e, D - 1)];
            bv[e] = pb[min(bc_next + e, D - 1)];
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            As[buf][(ak + e) * FI_LDT + arow] = (arow_ok && ak_next + e < D) ? (double)ar.v[e] - am[e] : 0.0;
            Bs[buf][bk * FI_LDT + bc + e] = (bk_next < D && bc_next + e < D) ? bv[e] : 0.0;
        }
    };

    fi_f64x4 acc[2][2];
    double part[2][4];                                    // this lane's share of rows wm * 32 + i * 16 + l4 + 4 r
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[i][r] = 0.0;
    const T* prow[2][4];                                  // the rows this lane folds (row 0 stands in for rows past N)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = row0 + wm * 32 + i * 16 + l4 + 4 * r;
            prow[i][r] = X + (row < N ? row : 0) * ld;
        }

    fetch(0);
    stage(0);
    __syncthreads();
    for (int step = 0; step < steps; ++step) {
        const int buf = step & 1, slab = step % nslab;
        if (slab == 0) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = fi_f64x4{0.0, 0.0, 0.0, 0.0};
        }
        if (step + 1 < steps) fetch(step + 1);
#pragma unroll
        for (int ks = 0; ks < FI_KT / 4; ++ks) {
            const int kk = (ks * 4 + l4) * FI_LDT;
            const double a0 = As[buf][kk + wm * 32 + l15], a1 = As[buf][kk + wm * 32 + 16 + l15];
            const double b0 = Bs[buf][kk + wn * 32 + l15], b1 = Bs[buf][kk + wn * 32 + 16 + l15];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (slab == nslab - 1) {                          // the column tile is complete: fold (T + lin) o C, columns ascending
            const int col0 = (step / nslab) * FI_TILE;
            double x[2][2][4], m[2], l[2];                // all loads first (a column past D is clamped, its term masked)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = min(col0 + wn * 32 + j * 16 + l15, D - 1);
                m[j] = mu[col];
                l[j] = lin[col];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) x[j][i][r] = (double)prow[i][r][col];
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const bool col_ok = col0 + wn * 32 + j * 16 + l15 < D;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double c = col_ok ? x[j][i][r] - m[j] : 0.0;
                        part[i][r] += (acc[i][j][r] + l[j]) * c;
                    }
            }
        }
        if (step + 1 < steps) stage(buf ^ 1);             // its last readers passed the barrier of the previous step
        __syncthreads();
    }

    // ---- a row's 2 x 16 lane partials: xor butterfly over the 16 lanes of a column group, then the two column halves
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double v = part[i][r];
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) v += __shfl_xor(v, off);
            if (l15 == 0) red[wn][wm * 32 + i * 16 + l4 + 4 * r] = v;
        }
    __syncthreads();
    if (wave == 0) {
        const int64_t row = row0 + lane;
        const bool valid = row < N;
        const double v = (red[0][lane] + red[1][lane]) + c0;
        const bool fin = v - v == 0.0;                    // a NaN or inf element makes every product of its row non-finite
        if (valid) psi[row] = fin ? v : __builtin_nan("");
        double s1 = (valid && fin) ? v : 0.0, s2 = (valid && fin) ? v * v : 0.0;
        double nf = (valid && fin) ? 1.0 : 0.0, nn = (valid && !fin) ? 1.0 : 0.0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            s1 += __shfl_xor(s1, off);
            s2 += __shfl_xor(s2, off);
            nf += __shfl_xor(nf, off);
            nn += __shfl_xor(nn, off);
        }
        if (lane == 0) {
            double* p = partials + (int64_t)blockIdx.x * 4;
            p[0] = s1; p[1] = s2; p[2] = nf; p[3] = nn;
        }
    }
}

// sums[q] = sum over the workgroups' partials: thread-strided, xor butterfly, the four waves in order
__global__ void __launch_bounds__(256) fi_sums_kernel(const double* __restrict__ partials, int64_t nwg, double* __restrict__ sums) {
    __shared__ double red[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t w = tid; w < nwg; w += 256)
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] += partials[w * 4 + q];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s[q] += __shfl_xor(s[q], off);
        if (lane == 0) red[wave][q] = s[q];
    }
    __syncthreads();
    if (tid < 4) sums[tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

template <class T>
static int frechet_influence(const T* X, int64_t N, int64_t ld, int D, const double* mu, const double* B, const double* lin, double c0,
                             double* psi, double* sums, void* ws, size_t ws_bytes, hipStream_t st) {
    AM_REQUIRE(X && mu && B && lin && psi && sums, AM_ERR_BAD_ARG, "null pointer");
    AM_REQUIRE(N >= 1 && D >= 1 && D <= 8192 && ld >= D, AM_ERR_BAD_SHAPE, "X has shape %lld x %d, ld=%lld (N >= 1, 1 <= D <= 8192, ld >= D)",
               (long long)N, D, (long long)ld);
    if (sizeof(T) == 4)
        AM_REQUIRE(aligned16(X) && ld % 4 == 0, AM_ERR_BAD_SHAPE, "float32 rows must be 16-byte aligned with ld %% 4 == 0 (ld=%lld)",
                   (long long)ld);
    const int64_t nwg = ceil_div(N, FI_TILE);
    AM_REQUIRE(nwg < ((int64_t)1 << 31), AM_ERR_BAD_SHAPE, "%lld rows exceed the grid", (long long)N);
    Carver c(ws, ws_bytes);
    double* partials = c.take<double>((size_t)nwg * 4);
    AM_REQUIRE(c.ok(), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes, have %zu", c.off, ws_bytes);
    hipLaunchKernelGGL(fi_rows_kernel<T>, dim3((unsigned)nwg), dim3(256), 0, st, X, N, ld, D, mu, B, lin, c0, psi, partials);
    AM_LAUNCH_CHECK();
    hipLaunchKernelGGL(fi_sums_kernel, dim3(1), dim3(256), 0, st, (const double*)partials, nwg, sums);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

}  // namespace am

using namespace am;

extern "C" size_t am_frechet_influence_workspace_bytes(int64_t N) {
    if (N < 1) return 0;
    Carver c(nullptr, 0);
    c.take<double>((size_t)ceil_div(N, FI_TILE) * 4);
    return c.off;
}

extern "C" int am_frechet_influence_f32(const float* X, int64_t N, int64_t ld, int D, const double* mu, const double* B, const double* lin,
                                        double c0, double* psi, double* sums, void* ws, size_t ws_bytes, am_stream_t stream) {
    return frechet_influence<float>(X, N, ld, D, mu, B, lin, c0, psi, sums, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int am_frechet_influence_f64(const double* X, int64_t N, int64_t ld, int D, const double* mu, const double* B, const double* lin,
                                        double c0, double* psi, double* sums, void* ws, size_t ws_bytes, am_stream_t stream) {
    return frechet_influence<double>(X, N, ld, D, mu, B, lin, c0, psi, sums, ws, ws_bytes, static_cast<hipStream_t>(stream));
}
