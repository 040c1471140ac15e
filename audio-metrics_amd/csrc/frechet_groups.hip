// Per-group Frechet distance in the dual (Gram) form (am_frechet_groups_f32 / _f64): B small groups of rows of one stored
// matrix, each scored on its own against one reference (mu_y, cov_y).  For a group of n rows with centred rows Xc the
// non-zero eigenvalues of cov_x cov_y are those of the symmetric positive semi-definite n x n matrix
//     M = Xc cov_y Xc^T / (n - 1)
// so tr sqrt(cov_x cov_y) = sum sqrt(lambda_i(M)): no D x D matrix is formed per group, and the eigenproblem fits in LDS.
//
//   pass 1  fg_centre_kernel   one workgroup per group: column means in f64 (rows added in list order), the centred rows
//                              Xc written to the workspace (float32 rows are converted on load, which is exact, so both
//                              row types share every later bit), |dmu|^2, tr cov_x = |Xc|_F^2 / (n - 1), tr cov_y; every
//                              index is checked against [0, N) - a row outside is never dereferenced, its position goes to
//                              the flag word at the start of the workspace and the row counts as zeros
//   pass 2  fg_gemm_kernel     Z = Xc cov_y over ALL gathered rows at once on v_mfma_f64_16x16x4_f64 (64 x 64 tiles)
//   pass 3  fg_solve_kernel    one workgroup per group: the upper triangle of M = Z Xc^T / (n - 1) on the f64 matrix cores,
//                              mirrored into LDS (exactly symmetric), then a cyclic Jacobi with round-robin ordering,
//                              eigenvalues only: a round holds m / 2 disjoint rotations, and A <- J^T A J is applied as
//                              (m / 2)^2 independent 2 x 2 blocks R_a^T B R_b, of which the a <= b half is computed and
//                              mirrored.  Three instantiations (up to 32, 64, 128 rows) so that small groups share a CU.
// Every reduction runs in a fixed order: the call is deterministic.
#include "am_common.h"
#include "groups_common.h"
#include "jacobi_lds.h"

namespace am {

constexpr int FG_MAX_ROWS = 128;      // 128 x 129 f64 = 129 KiB of the CU's 160 KiB LDS
constexpr int FG_TILE = 64, FG_KT = 16, FG_LDT = 80;  // pass 2: tile edge, k step, LDS row stride (f64)

typedef double fg_f64x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- pass 1: means, centred rows, the three scalar terms
template <class T>
__global__ void __launch_bounds__(256) fg_centre_kernel(const T* __restrict__ X, int64_t N, int64_t ld, int D, const int64_t* __restrict__ idx,
                                                        const int64_t* __restrict__ offs, const double* __restrict__ mu_y,
                                                        const double* __restrict__ cov_y, double* __restrict__ xc,
                                                        double* __restrict__ stats, unsigned long long* __restrict__ flag) {
    __shared__ double red[256];
    __shared__ int64_t rows[FG_MAX_ROWS];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int64_t pos0 = offs[b];
    const int n = (int)(offs[b + 1] - pos0);
    if (tid < n) {
        const int64_t row = idx ? idx[pos0 + tid] : pos0 + tid;
        const bool ok = (unsigned long long)row < (unsigned long long)N;
        if (!ok) atomicMax(flag, (unsigned long long)(pos0 + tid) + 1ull);
        rows[tid] = ok ? row : -1;
    }
    __syncthreads();
    double dmu2 = 0.0, sq = 0.0, try_ = 0.0;
    for (int d = tid; d < D; d += 256) {
        double s = 0.0;
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            const int64_t r = rows[j];
            s += r >= 0 ? (double)X[r * ld + d] : 0.0;
        }
        const double mean = s / (double)n;
        double q = 0.0;
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            const int64_t r = rows[j];
            const double c = r >= 0 ? (double)X[r * ld + d] - mean : 0.0;
            xc[(pos0 + j) * D + d] = c;
            q += c * c;
        }
        sq += q;
        const double dm = mean - mu_y[d];
        dmu2 += dm * dm;
        try_ += cov_y[(int64_t)d * D + d];
    }
    dmu2 = fg_block_sum(dmu2, red);
    sq = fg_block_sum(sq, red);
    try_ = fg_block_sum(try_, red);
    if (tid == 0) {
        stats[(int64_t)b * 3 + 0] = dmu2;
        stats[(int64_t)b * 3 + 1] = n > 1 ? sq / (double)(n - 1) : 0.0;       // one row -> zero covariance
        stats[(int64_t)b * 3 + 2] = try_;
    }
}

// ---------------------------------------------------------------- pass 2: Z = Xc cov_y
// Workgroup = one 64 x 64 tile of Z (column tiles vary fastest, so the row tile of Xc is reused from L2), wave w the 32 x 32
// quarter (w >> 1, w & 1) as 2 x 2 MFMA tiles.  Both operands are staged k-major in LDS: lane (l15, l4) of a k step of 4 reads
// element l15 of row k + l4, i.e. four runs of 16 consecutive f64.
__global__ void __launch_bounds__(256) fg_gemm_kernel(const double* __restrict__ xc, int64_t n_total, int D, const double* __restrict__ cov_y,
                                                      double* __restrict__ z, int ctiles) {
    __shared__ double As[FG_KT * FG_LDT];     // [k][row]
    __shared__ double Bs[FG_KT * FG_LDT];     // [k][col]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;
    const int ct = (int)(blockIdx.x % (unsigned)ctiles);
    const int64_t row0 = (int64_t)(blockIdx.x / (unsigned)ctiles) * FG_TILE;
    const int col0 = ct * FG_TILE;
    const int arow = tid & 63, ak = (tid >> 6) * 4;       // staging of A: 4 consecutive k of one row; a wave writes 64 adjacent rows of one k
    const int bk = tid >> 4, bc = (tid & 15) * 4;         // staging of B: 4 consecutive columns of one k
    const bool arow_ok = row0 + arow < n_total;
    const double* pa = xc + (arow_ok ? row0 + arow : 0) * D;
    fg_f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = fg_f64x4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < D; k0 += FG_KT) {
        double a[4], bv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ka = k0 + ak + e;
            a[e] = (arow_ok && ka < D) ? pa[ka] : 0.0;
            const int kb = k0 + bk, cb = col0 + bc + e;
            bv[e] = (kb < D && cb < D) ? cov_y[(int64_t)kb * D + cb] : 0.0;
        }
        __syncthreads();                                   // the previous step's reads are done
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            As[(ak + e) * FG_LDT + arow] = a[e];
            Bs[bk * FG_LDT + bc + e] = bv[e];
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < FG_KT / 4; ++ks) {
            const int kk = (ks * 4 + l4) * FG_LDT;
            const double a0 = As[kk + wm * 32 + l15], a1 = As[kk + wm * 32 + 16 + l15];
            const double b0 = Bs[kk + wn * 32 + l15], b1 = Bs[kk + wn * 32 + 16 + l15];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = row0 + wm * 32 + i * 16 + l4 + 4 * r;
                const int col = col0 + wn * 32 + j * 16 + l15;
                if (row < n_total && col < D) z[row * D + col] = acc[i][j][r];
            }
}

// ---------------------------------------------------------------- pass 3: M into LDS, Jacobi, the record
template <int MCAP>
__global__ void __launch_bounds__(256) fg_solve_kernel(const double* __restrict__ xc, const double* __restrict__ z,
                                                       const int64_t* __restrict__ offs, int D, const double* __restrict__ stats,
                                                       double* __restrict__ out) {
    constexpr int LDM = JacobiLds<MCAP>::LDM;
    constexpr int HCAP = JacobiLds<MCAP>::HCAP;
    __shared__ double M[MCAP * LDM];
    __shared__ double red[256];
    __shared__ double rc[HCAP], rs[HCAP], rt[HCAP];                    // the round's rotations: cos, sin, tan
    __shared__ int rp[HCAP], rq[HCAP];                                 // ... and their index pairs
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int b = blockIdx.x;
    const int64_t pos0 = offs[b];
    const int n = (int)(offs[b + 1] - pos0);
    if (n > MCAP || (MCAP > 32 && n <= MCAP / 2)) return;              // another instantiation's group
    const double dmu2 = stats[(int64_t)b * 3], trx = stats[(int64_t)b * 3 + 1], try_ = stats[(int64_t)b * 3 + 2];
    double* rec = out + (int64_t)b * 5;
    const double base = dmu2 + trx + try_;
    if (n == 1) {
        if (tid == 0) {
            const bool fin = base - base == 0.0;
            rec[0] = base; rec[1] = 0.0; rec[2] = 0.0; rec[3] = 0.0; rec[4] = fin ? 1.0 : 4.0;
        }
        return;
    }
    const int m = n + (n & 1);                                         // an odd group gets one all-zero dummy index
    for (int e = tid; e < m * LDM; e += 256) M[e] = 0.0;
    __syncthreads();

    // ---- M = Z Xc^T / (n - 1): 16 x 16 tiles of the upper triangle, wave w takes tiles w, w + 4, ...
    const int nt = (n + 15) / 16;
    const int ntile = ((nt + 1) / 2) * (nt + 1);
    const double inv = 1.0 / (double)(n - 1);
    for (int t = wave; t < ntile; t += 4) {
        int ti, tj;
        if (!fg_fold_decode(t, nt, ti, tj)) continue;
        const int ra = ti * 16 + l15, rb = tj * 16 + l15;
        const bool oka = ra < n, okb = rb < n;
        const double* pa = z + (pos0 + (oka ? ra : 0)) * D;
        const double* pb = xc + (pos0 + (okb ? rb : 0)) * D;
        fg_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < D; k0 += 16) {
            double av[4], bv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {                               // four independent loads per operand in flight
                const int k = k0 + 4 * u + l4;
                av[u] = (oka && k < D) ? pa[k] : 0.0;
                bv[u] = (okb && k < D) ? pb[k] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = ti * 16 + l4 + 4 * r, j = tj * 16 + l15;
            if (i < n && j < n) {
                const double v = acc[r] * inv;
                if (ti != tj || j >= i) M[i * LDM + j] = v;             // on diagonal tiles the upper triangle decides
                if (ti != tj || j > i) M[j * LDM + i] = v;
            }
        }
    }
    __syncthreads();

    // ---- the cyclic Jacobi of jacobi_lds.h; a non-finite scalar term stops the group as a non-finite M does
    double fro, off;
    int sweeps;
    const int stop = fg_jacobi_lds<MCAP>(M, JacobiLds<MCAP>{red, rc, rs, rt, rp, rq}, m, !(base - base == 0.0), fro, off, sweeps);

    // ---- eigenvalues at or below 4 n 2^-52 lambda_max count as zero; the rest add their square roots in index order
    if (tid == 0) {
        double lmax = 0.0;
        for (int i = 0; i < n; ++i) lmax = fmax(lmax, M[i * LDM + i]);
        red[0] = 4.0 * (double)n * FG_EPS * lmax;
    }
    __syncthreads();
    const double thr = red[0];
    __syncthreads();
    if (tid < n) {
        const double lam = M[tid * LDM + tid];
        red[tid] = lam > thr ? sqrt(lam) : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
        double tr = 0.0;
        for (int i = 0; i < n; ++i) tr += red[i];
        rec[0] = base - 2.0 * tr;
        rec[1] = tr;
        rec[2] = (double)sweeps;
        rec[3] = fro > 0.0 ? off / fro : 0.0;
        rec[4] = (double)stop;
    }
}

// ---------------------------------------------------------------- host side
struct GroupsBuffers {
    GroupHead head;
    double *stats, *xc, *z;
};

static bool carve_groups(Carver& c, int64_t n_total, int B, int D, GroupsBuffers& g) {
    g.head = carve_group_head(c, B, (size_t)B * 24);           // the tail: 3 scalars per group
    g.stats = reinterpret_cast<double*>(g.head.tail);
    g.xc = c.take<double>(2 * (size_t)n_total * D);
    g.z = g.xc ? g.xc + (size_t)n_total * D : nullptr;
    return c.ok();
}

template <class T>
static int frechet_groups(const T* X, int64_t N, int64_t ld, int D, const int64_t* idx, const int64_t* offsets, int B, const double* mu_y,
                          const double* cov_y, double* out, void* ws, size_t ws_bytes, hipStream_t st) {
    constexpr bool F64 = sizeof(T) == 8;
    AM_REQUIRE(X && offsets && mu_y && cov_y && out, AM_ERR_BAD_ARG, "null pointer");
    AM_REQUIRE(N >= 1 && D >= 1 && B >= 1, AM_ERR_BAD_SHAPE, "X has shape %lld x %d, B=%d (all must be >= 1)", (long long)N, D, B);
    AM_TRY(check_group_rows(X, N, ld, D));
    int64_t n_total;
    AM_TRY(check_group_offsets(offsets, B, FG_MAX_ROWS, &n_total));
    AM_TRY(check_stored_rows(idx, n_total, N));
    bool cls[3] = {false, false, false};                       // which of the three solve sizes the groups need
    for (int b = 0; b < B; ++b) {
        const int64_t n = offsets[b + 1] - offsets[b];
        cls[n <= 32 ? 0 : n <= 64 ? 1 : 2] = true;
    }
    const int ctiles = (int)ceil_div(D, FG_TILE);
    const int64_t gemm_wgs = ceil_div(n_total, FG_TILE) * ctiles;
    AM_REQUIRE(gemm_wgs < ((int64_t)1 << 31), AM_ERR_BAD_SHAPE, "%lld rows x %d columns exceed the grid", (long long)n_total, D);
    Carver c(ws, ws_bytes);
    GroupsBuffers g;
    AM_REQUIRE(carve_groups(c, n_total, B, D, g), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes, have %zu", c.off, ws_bytes);
    AM_TRY(upload_group_head(g.head, offsets, B, st));
    const int64_t* offs = g.head.offs;
    hipLaunchKernelGGL(fg_centre_kernel<T>, dim3((unsigned)B), dim3(256), 0, st, X, N, ld, D, idx, offs, mu_y, cov_y, g.xc,
                       g.stats, g.head.flag);
    AM_LAUNCH_CHECK();
    hipLaunchKernelGGL(fg_gemm_kernel, dim3((unsigned)gemm_wgs), dim3(256), 0, st, (const double*)g.xc, n_total, D, cov_y, g.z, ctiles);
    AM_LAUNCH_CHECK();
    if (cls[0]) {
        hipLaunchKernelGGL(fg_solve_kernel<32>, dim3((unsigned)B), dim3(256), 0, st, (const double*)g.xc, (const double*)g.z,
                           offs, D, (const double*)g.stats, out);
        AM_LAUNCH_CHECK();
    }
    if (cls[1]) {
        hipLaunchKernelGGL(fg_solve_kernel<64>, dim3((unsigned)B), dim3(256), 0, st, (const double*)g.xc, (const double*)g.z,
                           offs, D, (const double*)g.stats, out);
        AM_LAUNCH_CHECK();
    }
    if (cls[2]) {
        hipLaunchKernelGGL(fg_solve_kernel<FG_MAX_ROWS>, dim3((unsigned)B), dim3(256), 0, st, (const double*)g.xc, (const double*)g.z,
                           offs, D, (const double*)g.stats, out);
        AM_LAUNCH_CHECK();
    }
    return AM_OK;
}

}  // namespace am

using namespace am;

extern "C" int am_frechet_groups_max_rows(void) { return FG_MAX_ROWS; }

extern "C" size_t am_frechet_groups_workspace_bytes(int64_t n_total, int B, int D) {
    if (n_total < 1 || B < 1 || D < 1) return 0;
    Carver c(nullptr, 0);
    GroupsBuffers g;
    carve_groups(c, n_total, B, D, g);
    return c.off;
}

extern "C" int am_frechet_groups_f32(const float* X, int64_t N, int64_t ld, int D, const int64_t* idx, const int64_t* offsets, int B,
                                     const double* mu_y, const double* cov_y, double* out_dev, void* ws, size_t ws_bytes,
                                     am_stream_t stream) {
    return frechet_groups<float>(X, N, ld, D, idx, offsets, B, mu_y, cov_y, out_dev, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int am_frechet_groups_f64(const double* X, int64_t N, int64_t ld, int D, const int64_t* idx, const int64_t* offsets, int B,
                                     const double* mu_y, const double* cov_y, double* out_dev, void* ws, size_t ws_bytes,
                                     am_stream_t stream) {
    return frechet_groups<double>(X, N, ld, D, idx, offsets, B, mu_y, cov_y, out_dev, ws, ws_bytes, static_cast<hipStream_t>(stream));
}
