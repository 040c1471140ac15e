// The Vendi score (Friedman & Dieng 2023): exp of the entropy of the eigenvalues of M = K / n, K a similarity matrix of n rows
// with K_ii = 1 - "the effective number of distinct samples".  With G = X X^T accumulated in f64 (float32 rows are converted on
// load, which is exact, so both row types share every later bit):
//     cosine    K_ij = G_ij / (sqrt(G_ii) sqrt(G_jj))
//     gaussian  K_ij = exp(-gamma max(G_ii + G_jj - 2 G_ij, 0)),   gamma = 1 / (2 bw^2), rows as they are
// and K_ii = 1 exactly, so M is symmetric PSD with trace 1.
//
//   am_vendi_groups_*   B groups of up to 128 rows of one stored matrix (the group-list protocol of groups_common.h), one
//                       workgroup per group: the rows are gathered straight from X, the upper triangle of G comes from
//                       v_mfma_f64_16x16x4_f64 in 16 x 16 tiles and is mirrored into LDS, the kernel transform is applied in
//                       LDS, the cyclic Jacobi of jacobi_lds.h diagonalises M, and the group's eigenvalues (descending, those
//                       <= 4 n 2^-52 lambda_max written as 0), entropy, order-1 score and rank are written.  Three
//                       instantiations (up to 32, 64, 128 rows) so that small groups share a CU.
//   am_vendi_gram_*     M = K / n for up to 2048 rows as an [n][n] matrix on the 64 x 64 engine of f64_engine.h: upper tiles
//                       computed and mirrored, diagonal exactly 1 / n, every element written once.
//   am_vendi_moment_*   S = (1 / n) sum_i x_i x_i^T / |x_i|^2, [D][D]: the cosine kernel's dual form (K / n and S share their
//                       non-zero eigenvalues).  The inner dimension is the row index: the rows are cut into chunks, the chunks'
//                       partial matrices go to the workspace and are folded in chunk order.
// The eigenvalues of the two whole-set matrices come from am_eigh_sym_f64, whose null eigenvalues do not come out at 2^-52
// level (its pinned accuracy is 1e-10 lambda_0): callers of those routes threshold at 1e-10 lambda_max.
// A row of zero norm (cosine) or with a non-finite element: the group's record is NaN with stop code 4; the whole-set kernels
// count the row as zeros and report it through the second flag word of the workspace.
// No floating-point atomics; every reduction runs in a fixed order: the calls are deterministic.
#include "am_common.h"
#include "f64_engine.h"
#include "groups_common.h"
#include "jacobi_lds.h"
#include <algorithm>
#include <cmath>

namespace am {

constexpr int VG_MAX_ROWS = 128;          // 128 x 129 f64 = 129 KiB of the CU's 160 KiB LDS
constexpr int VG_GRAM_MAX_ROWS = 2048;
constexpr int VG_SIDE_NORM = 0, VG_SIDE_SQ = 1, VG_SIDE_RINV = 2;      // what vg_prep_kernel leaves per row

// four consecutive elements k .. k + 3 of a row as doubles; zeros past D and for a missing row (p == nullptr)
__device__ __forceinline__ void vg_load4(const float* p, int k, int D, double (&v)[4]) {
    if (p != nullptr && k + 3 < D) {                                   // 16-byte aligned: X is, ld % 4 == 0, k % 4 == 0
        const float4 f = *reinterpret_cast<const float4*>(p + k);
        v[0] = (double)f.x; v[1] = (double)f.y; v[2] = (double)f.z; v[3] = (double)f.w;
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = (p != nullptr && k + u < D) ? (double)p[k + u] : 0.0;
    }
}
__device__ __forceinline__ void vg_load4(const double* p, int k, int D, double (&v)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = (p != nullptr && k + u < D) ? p[k + u] : 0.0;
}

__device__ __forceinline__ double vg_gamma(double gamma, const float* __restrict__ gamma_dev) {
    return gamma_dev != nullptr ? 0.5 / (double)*gamma_dev : gamma;    // the device scalar holds a median squared distance
}

// ---------------------------------------------------------------- per-group kernel
template <class T, int MCAP>
__global__ void __launch_bounds__(256) vg_group_kernel(const T* __restrict__ X, int64_t N, int64_t ld, int D, const int64_t* __restrict__ idx,
                                                       const int64_t* __restrict__ offs, int kernel, double gamma,
                                                       const float* __restrict__ gamma_dev, double* __restrict__ out_rec,
                                                       double* __restrict__ out_evals, unsigned long long* __restrict__ flag) {
    constexpr int LDM = JacobiLds<MCAP>::LDM;
    constexpr int HCAP = JacobiLds<MCAP>::HCAP;
    __shared__ double M[MCAP * LDM];
    __shared__ double red[256];
    __shared__ double rc[HCAP], rs[HCAP], rt[HCAP];
    __shared__ int rp[HCAP], rq[HCAP];
    __shared__ int64_t rows[MCAP];
    __shared__ double diag[MCAP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int b = blockIdx.x;
    const int64_t pos0 = offs[b];
    const int n = (int)(offs[b + 1] - pos0);
    if (n > MCAP || (MCAP > 32 && n <= MCAP / 2)) return;              // another instantiation's group
    double* rec = out_rec + (int64_t)b * 8;
    if (tid < MCAP) {
        int64_t row = -1;
        if (tid < n) {
            row = idx ? idx[pos0 + tid] : pos0 + tid;
            if (!((unsigned long long)row < (unsigned long long)N)) {  // never dereferenced: the row counts as zeros
                atomicMax(flag, (unsigned long long)(pos0 + tid) + 1ull);
                row = -1;
            }
        }
        rows[tid] = row;
    }
    const int m = n + (n & 1);                                         // an odd group gets one all-zero dummy index
    for (int e = tid; e < m * LDM; e += 256) M[e] = 0.0;
    __syncthreads();

    // ---- G = X X^T: 16 x 16 tiles of the upper triangle, wave w takes tiles w, w + 4, ...; lane (l15, l4) feeds the four
    // elements k0 + 4 l4 .. + 3 of its row to four MFMA steps (both operands alike, so every inner index is met once)
    const int nt = (n + 15) / 16;
    const int ntile = ((nt + 1) / 2) * (nt + 1);
    for (int t = wave; t < ntile; t += 4) {
        int ti, tj;
        if (!fg_fold_decode(t, nt, ti, tj)) continue;
        const int64_t ra = rows[ti * 16 + l15], rb = rows[tj * 16 + l15];      // (16 nt <= MCAP; -1 past n)
        const T* pa = ra >= 0 ? X + ra * ld : nullptr;
        const T* pb = rb >= 0 ? X + rb * ld : nullptr;
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < D; k0 += 16) {
            double av[4], bv[4];
            vg_load4(pa, k0 + 4 * l4, D, av);
            vg_load4(pb, k0 + 4 * l4, D, bv);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = ti * 16 + l4 + 4 * r, j = tj * 16 + l15;
            if (i < n && j < n) {
                const double v = acc[r];
                if (ti != tj || j >= i) M[i * LDM + j] = v;             // on diagonal tiles the upper triangle decides
                if (ti != tj || j > i) M[j * LDM + i] = v;
            }
        }
    }
    __syncthreads();

    // ---- the diagonal, the rows that have no similarity, the kernel transform
    double bad = 0.0;
    if (tid < n) {
        const double g = M[tid * LDM + tid];
        bad = (!(g - g == 0.0) || (kernel == AM_VENDI_COSINE && g == 0.0)) ? 1.0 : 0.0;
        diag[tid] = kernel == AM_VENDI_COSINE ? sqrt(g) : g;
    }
    bad = fg_block_sum(bad, red);
    if (bad != 0.0) {
        const double nan = __builtin_nan("");
        if (tid < n) out_evals[pos0 + tid] = nan;
        if (tid == 0) {
            rec[0] = nan; rec[1] = nan; rec[2] = 0.0; rec[3] = nan; rec[4] = 0.0; rec[5] = 0.0; rec[6] = 4.0; rec[7] = 0.0;
        }
        return;
    }
    const double inv_n = 1.0 / (double)n;
    const double gm = vg_gamma(gamma, gamma_dev);
    for (int e = tid; e < n * n; e += 256) {
        const int i = e / n, j = e - i * n;
        const double g = M[i * LDM + j];
        double k;
        if (i == j) k = 1.0;
        else if (kernel == AM_VENDI_COSINE) k = g / (diag[i] * diag[j]);
        else k = exp(-gm * fmax((diag[i] + diag[j]) - 2.0 * g, 0.0));
        M[i * LDM + j] = k * inv_n;
    }
    __syncthreads();

    double fro, off;
    int sweeps;
    const int stop = fg_jacobi_lds<MCAP>(M, JacobiLds<MCAP>{red, rc, rs, rt, rp, rq}, m, false, fro, off, sweeps);

    // ---- eigenvalues in descending order (ties by index); those at or below 4 n 2^-52 lambda_max count as zero
    __syncthreads();
    if (tid < n) diag[tid] = M[tid * LDM + tid];
    __syncthreads();
    if (tid < n) {
        const double lam = diag[tid];
        int pos = 0;
        for (int j = 0; j < n; ++j) {
            const double o = diag[j];
            pos += (o > lam || (o == lam && j < tid)) ? 1 : 0;
        }
        red[pos] = lam;
    }
    __syncthreads();
    const double lmax = red[0];
    const double thr = 4.0 * (double)n * FG_EPS * lmax;
    if (tid < n) {
        const double lam = red[tid];
        const bool keep = lam > thr;
        diag[tid] = keep ? -(lam * log(lam)) : 0.0;
        out_evals[pos0 + tid] = stop == 4 ? __builtin_nan("") : (keep ? lam : 0.0);
    }
    __syncthreads();
    if (tid == 0) {
        double h = 0.0;
        int rank = 0;
        for (int i = 0; i < n; ++i) {
            h += diag[i];
            rank += red[i] > thr ? 1 : 0;
        }
        if (stop == 4) h = __builtin_nan("");
        rec[0] = exp(h);
        rec[1] = h;
        rec[2] = (double)rank;
        rec[3] = lmax;
        rec[4] = (double)sweeps;
        rec[5] = fro > 0.0 ? off / fro : 0.0;
        rec[6] = (double)stop;
        rec[7] = 0.0;
    }
}

// ---------------------------------------------------------------- whole set: one pass over the rows in front of the tiles
// One wave per listed row p (idx == nullptr: row p itself): g = |x|^2 as lane-strided partial sums and a butterfly, then
//   side[p] = sqrt(g) (VG_SIDE_NORM), g (VG_SIDE_SQ) or 1 / sqrt(g) (VG_SIDE_RINV), and the row as doubles in xg (if given).
// An index outside [0, N) goes to flags[0]; a row of zero norm (unless VG_SIDE_SQ) or with a non-finite element to flags[1]
// (1 + its position).  Either kind of row counts as zeros: side = 1, 0, 0, and zeros in xg.
template <class T>
__global__ void __launch_bounds__(256) vg_prep_kernel(const T* __restrict__ X, int64_t N, int64_t ld, int D, const int64_t* __restrict__ idx,
                                                      int64_t n, int what, double* __restrict__ side, double* __restrict__ xg,
                                                      unsigned long long* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= n) return;
    const int64_t row = idx ? idx[p] : p;
    const bool inside = (unsigned long long)row < (unsigned long long)N;
    const T* x = X + (inside ? row : 0) * ld;
    double g = 0.0;
    if (inside)
        for (int k = lane; k < D; k += 64) {
            const double v = (double)x[k];
            g = fma(v, v, g);
        }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) g += __shfl_xor(g, o);
    const bool bad = !(g - g == 0.0) || (what != VG_SIDE_SQ && g == 0.0);
    if (lane == 0) {
        if (!inside) atomicMax(flags, (unsigned long long)p + 1ull);
        else if (bad) atomicMax(flags + 1, (unsigned long long)p + 1ull);
        const bool zero = bad || !inside;
        side[p] = what == VG_SIDE_NORM ? (zero ? 1.0 : sqrt(g)) : what == VG_SIDE_SQ ? (zero ? 0.0 : g) : (zero ? 0.0 : 1.0 / sqrt(g));
    }
    if (xg != nullptr)
        for (int k = lane; k < D; k += 64) xg[p * D + k] = (bad || !inside) ? 0.0 : (double)x[k];
}

// t-th tile (tq <= tp) of the T x T upper triangle, row by row
__device__ __forceinline__ void vg_tri_decode(int t, int T, int& tq, int& tp) {
    tq = 0;
    while (t >= T - tq) { t -= T - tq; ++tq; }
    tp = tq + t;
}

// ---------------------------------------------------------------- whole set: M = K / n
// One workgroup per upper 64 x 64 tile (dist64_block_kernel's pattern): out[q][p] and its mirror out[p][q] are written by the
// lane that holds the pair, on diagonal tiles by the lane with p >= q, so every element is written once and M is symmetric.
__global__ void __launch_bounds__(FTHREADS) vg_gram_kernel(const double* __restrict__ xg, int64_t n, int D, const double* __restrict__ side,
                                                           int kernel, double gamma, const float* __restrict__ gamma_dev, int T,
                                                           double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double lds64[];
    const FLane L;
    int tq, tp;
    vg_tri_decode((int)blockIdx.x, T, tq, tp);
    f64x4 acc[4];
    zero4(acc);
    f64_tile(DenseRows64{xg, D, n, (int64_t)tq * FT}, DenseRows64{xg, D, n, (int64_t)tp * FT}, D, lds64, L, acc);
    const int64_t p = (int64_t)tp * FT + L.prow();
    if (p >= n) return;
    const double sp = side[p];
    const double inv_n = 1.0 / (double)n;
    const double gm = vg_gamma(gamma, gamma_dev);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t q = (int64_t)tq * FT + L.qrow(mt, r);
            if (q >= n || (tq == tp && p < q)) continue;
            double k;
            if (p == q) k = 1.0;
            else if (kernel == AM_VENDI_COSINE) k = acc[mt][r] / (side[q] * sp);
            else k = exp(-gm * fmax((side[q] + sp) - 2.0 * acc[mt][r], 0.0));
            const double v = k * inv_n;
            out[q * n + p] = v;
            if (p != q) out[p * n + q] = v;
        }
}

// ---------------------------------------------------------------- whole set: S = (1 / n) sum_i xh_i xh_i^T, xh_i = x_i / |x_i|
// Workgroup = (upper 64 x 64 tile of S, chunk of rows).  The engine's layout with the roles turned: the tile's "rows" are
// columns of X, the inner index is the row of X.  A slab is 16 rows of X: thread (kk = tid >> 4, c4 = 4 (tid & 15)) loads four
// consecutive columns of row kk for either operand, scales them by 1 / |x| and puts them at [column][kk] (stride 17), which is
// where f64_tile's fragment reads expect them.  Two stages, the loads of slab s + 1 under the MFMAs of slab s.
template <class T>
__global__ void __launch_bounds__(FTHREADS) vg_moment_kernel(const T* __restrict__ X, int64_t N, int64_t ld, int D, const double* __restrict__ rinv,
                                                             int chunks, int TT, double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) double lds64[];
    const FLane L;
    const int chunk = (int)(blockIdx.x % (unsigned)chunks);
    int tq, tp;
    vg_tri_decode((int)(blockIdx.x / (unsigned)chunks), TT, tq, tp);
    const int64_t r0 = N * chunk / chunks, r1 = N * (chunk + 1) / chunks;
    const int nslabs = (int)((r1 - r0 + FK - 1) / FK);
    const int kk = L.tid >> 4, c4 = (L.tid & 15) * 4;
    double qv[4], pv[4];
    auto fetch = [&](int s) {
        const int64_t row = r0 + (int64_t)s * FK + kk;
        const bool ok = row < r1;
        const double scale = ok ? rinv[row] : 0.0;
        const T* x = X + (ok ? row : 0) * ld;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cq = tq * FT + c4 + j, cp = tp * FT + c4 + j;
            qv[j] = (scale != 0.0 && cq < D) ? (double)x[cq] * scale : 0.0;      // scale == 0: a row that counts as zeros
            pv[j] = (scale != 0.0 && cp < D) ? (double)x[cp] * scale : 0.0;
        }
    };
    f64x4 acc[4];
    zero4(acc);
    if (nslabs > 0) fetch(0);
    for (int s = 0; s < nslabs; ++s) {
        double* st = lds64 + (s & 1) * 2 * FTILE;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            st[(c4 + j) * FLD + kk] = qv[j];
            st[FTILE + (c4 + j) * FLD + kk] = pv[j];
        }
        __syncthreads();
        if (s + 1 < nslabs) fetch(s + 1);
        const double* q = st + L.l15 * FLD + L.l4;
        const double* p = st + FTILE + (L.wave * 16 + L.l15) * FLD + L.l4;
#pragma unroll
        for (int ks = 0; ks < FK / 4; ++ks) {
            const double bv = p[ks * 4];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(q[mt * 16 * FLD + ks * 4], bv, acc[mt], 0, 0, 0);
        }
        // (no second barrier: the next slab goes to the other stage, as in f64_tile)
    }
    const int cb = tp * FT + L.prow();
    double* dst = partial + (int64_t)chunk * D * D;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ca = tq * FT + L.qrow(mt, r);
            if (ca < D && cb < D) dst[(int64_t)ca * D + cb] = acc[mt][r];
        }
}

// S[a][b] = S[b][a] = (sum over the chunks, in chunk order) / n for the pairs of the upper tiles; on a diagonal tile a <= b
__global__ void __launch_bounds__(256) vg_fold_kernel(const double* __restrict__ partial, int D, int chunks, int64_t n, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)D * D) return;
    const int a = (int)(e / D), b = (int)(e - (int64_t)a * D);
    const int ta = a / FT, tb = b / FT;
    if (ta > tb || (ta == tb && a > b)) return;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += partial[(int64_t)c * D * D + e];
    s /= (double)n;
    out[e] = s;
    if (a != b) out[(int64_t)b * D + a] = s;
}

// ---------------------------------------------------------------- host side
static int check_kernel_args(int kernel, double gamma, const float* gamma_dev) {
    AM_REQUIRE(kernel == AM_VENDI_COSINE || kernel == AM_VENDI_GAUSSIAN, AM_ERR_BAD_ARG, "kernel=%d (AM_VENDI_COSINE or AM_VENDI_GAUSSIAN)",
               kernel);
    if (kernel == AM_VENDI_GAUSSIAN && gamma_dev == nullptr)
        AM_REQUIRE(std::isfinite(gamma) && gamma > 0.0, AM_ERR_BAD_ARG, "gamma=%g must be finite and positive (or gamma_dev given)", gamma);
    return AM_OK;
}

template <class T>
static int vendi_groups(const T* X, int64_t N, int64_t ld, int D, const int64_t* idx, const int64_t* offsets, int B, int kernel, double gamma,
                        const float* gamma_dev, double* out_rec, double* out_evals, void* ws, size_t ws_bytes, hipStream_t st) {
    AM_REQUIRE(X && offsets && out_rec && out_evals, AM_ERR_BAD_ARG, "null pointer");
    AM_REQUIRE(N >= 1 && D >= 1 && B >= 1, AM_ERR_BAD_SHAPE, "X has shape %lld x %d, B=%d (all must be >= 1)", (long long)N, D, B);
    AM_TRY(check_kernel_args(kernel, gamma, gamma_dev));
    AM_TRY(check_group_rows(X, N, ld, D));
    int64_t n_total;
    AM_TRY(check_group_offsets(offsets, B, VG_MAX_ROWS, &n_total));
    AM_TRY(check_stored_rows(idx, n_total, N));
    bool cls[3] = {false, false, false};                       // which of the three sizes the groups need
    for (int b = 0; b < B; ++b) {
        const int64_t n = offsets[b + 1] - offsets[b];
        cls[n <= 32 ? 0 : n <= 64 ? 1 : 2] = true;
    }
    Carver c(ws, ws_bytes);
    const GroupHead head = carve_group_head(c, B);
    AM_REQUIRE(c.ok(), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes, have %zu", c.off, ws_bytes);
    AM_TRY(upload_group_head(head, offsets, B, st));
    const int64_t* offs = head.offs;
    if (cls[0]) {
        hipLaunchKernelGGL((vg_group_kernel<T, 32>), dim3((unsigned)B), dim3(256), 0, st, X, N, ld, D, idx, offs, kernel, gamma, gamma_dev, out_rec,
                           out_evals, head.flag);
        AM_LAUNCH_CHECK();
    }
    if (cls[1]) {
        hipLaunchKernelGGL((vg_group_kernel<T, 64>), dim3((unsigned)B), dim3(256), 0, st, X, N, ld, D, idx, offs, kernel, gamma, gamma_dev, out_rec,
                           out_evals, head.flag);
        AM_LAUNCH_CHECK();
    }
    if (cls[2]) {
        hipLaunchKernelGGL((vg_group_kernel<T, VG_MAX_ROWS>), dim3((unsigned)B), dim3(256), 0, st, X, N, ld, D, idx, offs, kernel, gamma, gamma_dev,
                           out_rec, out_evals, head.flag);
        AM_LAUNCH_CHECK();
    }
    return AM_OK;
}

// the whole-set workspaces open with two flag words: [0] an index outside [0, N), [1] a row without a similarity
struct GramBuffers {
    unsigned long long* flags;
    double *side, *xg;
};
static bool carve_gram(Carver& c, int64_t n, int D, GramBuffers& g) {
    g.flags = c.take<unsigned long long>(2);
    g.side = c.take<double>((size_t)n);
    g.xg = c.take<double>((size_t)n * D);
    return c.ok();
}

template <class T>
static int vendi_gram(const T* X, int64_t N, int64_t ld, int D, const int64_t* idx, int64_t n, int kernel, double gamma, const float* gamma_dev,
                      double* out_m, void* ws, size_t ws_bytes, hipStream_t st) {
    AM_REQUIRE(X && out_m, AM_ERR_BAD_ARG, "null pointer");
    AM_REQUIRE(N >= 1 && D >= 1 && n >= 1, AM_ERR_BAD_SHAPE, "X has shape %lld x %d, n=%lld (all must be >= 1)", (long long)N, D, (long long)n);
    AM_REQUIRE(n <= VG_GRAM_MAX_ROWS, AM_ERR_BAD_SHAPE, "n=%lld rows exceed am_vendi_gram_max_rows() = %d", (long long)n, VG_GRAM_MAX_ROWS);
    AM_TRY(check_kernel_args(kernel, gamma, gamma_dev));
    AM_TRY(check_group_rows(X, N, ld, D));
    AM_TRY(check_stored_rows(idx, n, N));
    Carver c(ws, ws_bytes);
    GramBuffers g;
    AM_REQUIRE(carve_gram(c, n, D, g), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes, have %zu", c.off, ws_bytes);
    AM_HIP_TRY(hipMemsetAsync(g.flags, 0, 2 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(vg_prep_kernel<T>, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, st, X, N, ld, D, idx, n,
                       kernel == AM_VENDI_COSINE ? VG_SIDE_NORM : VG_SIDE_SQ, g.side, g.xg, g.flags);
    AM_LAUNCH_CHECK();
    const int T_ = (int)ceil_div(n, FT);
    hipLaunchKernelGGL(vg_gram_kernel, dim3((unsigned)(T_ * (T_ + 1) / 2)), dim3(FTHREADS), (size_t)FENGINE_DOUBLES * 8, st, (const double*)g.xg, n, D,
                       (const double*)g.side, kernel, gamma, gamma_dev, T_, out_m);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

static int moment_chunks(int64_t n, int D) {
    // about 1024 workgroups over the upper tiles, at least 128 rows per chunk
    const int64_t T_ = ceil_div(D, FT), ntri = T_ * (T_ + 1) / 2;
    int64_t c = std::min<int64_t>(ceil_div(1024, ntri), 256);
    c = std::min<int64_t>(c, std::max<int64_t>(1, n / 128));
    return (int)c;
}

struct MomentBuffers {
    unsigned long long* flags;
    double *rinv, *partial;
};
static bool carve_moment(Carver& c, int64_t n, int D, MomentBuffers& g) {
    g.flags = c.take<unsigned long long>(2);
    g.rinv = c.take<double>((size_t)n);
    g.partial = c.take<double>((size_t)moment_chunks(n, D) * D * D);
    return c.ok();
}

template <class T>
static int vendi_moment(const T* X, int64_t N, int64_t ld, int D, double* out_s, void* ws, size_t ws_bytes, hipStream_t st) {
    AM_REQUIRE(X && out_s, AM_ERR_BAD_ARG, "null pointer");
    AM_REQUIRE(N >= 1 && D >= 1, AM_ERR_BAD_SHAPE, "X has shape %lld x %d (both must be >= 1)", (long long)N, D);
    AM_TRY(check_group_rows(X, N, ld, D));
    const int chunks = moment_chunks(N, D);
    const int64_t T_ = ceil_div(D, FT), ntri = T_ * (T_ + 1) / 2;
    AM_REQUIRE(ntri * chunks < ((int64_t)1 << 31), AM_ERR_BAD_SHAPE, "D=%d exceeds the grid", D);
    Carver c(ws, ws_bytes);
    MomentBuffers g;
    AM_REQUIRE(carve_moment(c, N, D, g), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes, have %zu", c.off, ws_bytes);
    AM_HIP_TRY(hipMemsetAsync(g.flags, 0, 2 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(vg_prep_kernel<T>, dim3((unsigned)ceil_div(N, 4)), dim3(256), 0, st, X, N, ld, D, (const int64_t*)nullptr, N, VG_SIDE_RINV,
                       g.rinv, (double*)nullptr, g.flags);
    AM_LAUNCH_CHECK();
    hipLaunchKernelGGL(vg_moment_kernel<T>, dim3((unsigned)(ntri * chunks)), dim3(FTHREADS), (size_t)FENGINE_DOUBLES * 8, st, X, N, ld, D,
                       (const double*)g.rinv, chunks, (int)T_, g.partial);
    AM_LAUNCH_CHECK();
    hipLaunchKernelGGL(vg_fold_kernel, dim3((unsigned)ceil_div((int64_t)D * D, 256)), dim3(256), 0, st, (const double*)g.partial, D, chunks, N, out_s);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

}  // namespace am

using namespace am;

extern "C" int am_vendi_groups_max_rows(void) { return VG_MAX_ROWS; }

extern "C" size_t am_vendi_groups_workspace_bytes(int64_t n_total, int B, int D) {
    if (n_total < 1 || B < 1 || D < 1) return 0;
    Carver c(nullptr, 0);
    carve_group_head(c, B);
    return c.off;
}

extern "C" int am_vendi_groups_f32(const float* X, int64_t N, int64_t ld, int D, const int64_t* idx, const int64_t* offsets, int B, int kernel,
                                   double gamma, const float* gamma_dev, double* out_rec, double* out_evals, void* ws, size_t ws_bytes,
                                   am_stream_t stream) {
    return vendi_groups<float>(X, N, ld, D, idx, offsets, B, kernel, gamma, gamma_dev, out_rec, out_evals, ws, ws_bytes,
                               static_cast<hipStream_t>(stream));
}

extern "C" int am_vendi_groups_f64(const double* X, int64_t N, int64_t ld, int D, const int64_t* idx, const int64_t* offsets, int B, int kernel,
                                   double gamma, const float* gamma_dev, double* out_rec, double* out_evals, void* ws, size_t ws_bytes,
                                   am_stream_t stream) {
    return vendi_groups<double>(X, N, ld, D, idx, offsets, B, kernel, gamma, gamma_dev, out_rec, out_evals, ws, ws_bytes,
                                static_cast<hipStream_t>(stream));
}

extern "C" int am_vendi_gram_max_rows(void) { return VG_GRAM_MAX_ROWS; }

extern "C" size_t am_vendi_gram_workspace_bytes(int64_t n, int D) {
    if (n < 1 || n > VG_GRAM_MAX_ROWS || D < 1) return 0;
    Carver c(nullptr, 0);
    GramBuffers g;
    carve_gram(c, n, D, g);
    return c.off;
}

extern "C" int am_vendi_gram_f32(const float* X, int64_t N, int64_t ld, int D, const int64_t* idx, int64_t n, int kernel, double gamma,
                                 const float* gamma_dev, double* out_m, void* ws, size_t ws_bytes, am_stream_t stream) {
    return vendi_gram<float>(X, N, ld, D, idx, n, kernel, gamma, gamma_dev, out_m, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int am_vendi_gram_f64(const double* X, int64_t N, int64_t ld, int D, const int64_t* idx, int64_t n, int kernel, double gamma,
                                 const float* gamma_dev, double* out_m, void* ws, size_t ws_bytes, am_stream_t stream) {
    return vendi_gram<double>(X, N, ld, D, idx, n, kernel, gamma, gamma_dev, out_m, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int am_vendi_moment_chunks(int64_t n, int D) {
    if (n < 1 || D < 1) return 0;
    return moment_chunks(n, D);
}

extern "C" size_t am_vendi_moment_workspace_bytes(int64_t n, int D) {
    if (n < 1 || D < 1) return 0;
    Carver c(nullptr, 0);
    MomentBuffers g;
    carve_moment(c, n, D, g);
    return c.off;
}

extern "C" int am_vendi_moment_f32(const float* X, int64_t N, int64_t ld, int D, double* out_s, void* ws, size_t ws_bytes, am_stream_t stream) {
    return vendi_moment<float>(X, N, ld, D, out_s, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int am_vendi_moment_f64(const double* X, int64_t N, int64_t ld, int D, double* out_s, void* ws, size_t ws_bytes, am_stream_t stream) {
    return vendi_moment<double>(X, N, ld, D, out_s, ws, ws_bytes, static_cast<hipStream_t>(stream));
}
