// Two-sided row sums of the Gaussian kernel blocks of the unbiased MMD^2 (am_mmd_rbf_rows_f32): what the closed-form
// standard error of KAD and the two-model comparison are built from, for the Gram and exp work of am_mmd_rbf_f32 itself.
//
//   w_i = sum_{j != i} k(x_i, x_j)   (XX)      c_i = sum_j k(x_i, y_j)   (XY)
//   v_j = sum_{l != j} k(y_j, y_l)   (YY)      r_j = sum_i k(x_i, y_j)   (XY)
//
// Arithmetic of one pair: that of MmdEpilogue::finish in kad.hip - d2 = max((|a|^2 + |b|^2) - 2 dot, 0) in f64, f64 norms,
// f32 matrix-core dot product, k = exp(-d2 gamma) in f64.
//
// Every 128 x 128 tile is computed once and summed along BOTH axes of the accumulator:
//   P rows (lane axis)      one f64 running sum per P row and lane over the Q tiles of the workgroup (RowEpilogue of
//                           kad_groups.hip); at the end fold_p_rows: the two halves of a wave, then the two wm waves through LDS
//                           -> pp[chunk][band slot][128]
//   Q rows (register axis)  per tile a lane holds 32 Q rows.  Their sums over the wave's 64 P rows are formed by a
//                           progressive butterfly: the values of the two nt sub-tiles are added in the lane, and every
//                           time two values of the same level exist, the lanes whose bit `level` is clear keep the earlier
//                           one and the others the later one, each adding its partner's copy (lane ^ (1 << level)).  One
//                           pending value per level (5) instead of 32 accumulators, 31 exchanges per tile instead of 160;
//                           after the 32nd value lane r holds the complete sum of Q row number r of the wave's 32 (per
//                           half-wave).  The two wn waves write separate slots -> qp[band slot][wn][Q row]
// XX and YY sweep the upper-triangular tiles (P tile tp against Q tiles 0 .. tp).  An off-diagonal tile feeds its P rows'
// sums and its Q rows' sums; the diagonal tile feeds the P side only, with q == p dropped by INDEX: row i gets its pairs
// with rows of tiles <= tile(i) from the P side and those with rows of later tiles from the Q side.  XY: P = X, Q = Y, every
// tile once - c is the P side, r the Q side.
//
// The P tiles are swept in bands of ROWS_BAND.  After each band one small kernel adds the band's Q-side slots to the running
// f64 sums in P-tile order (wn 0, then wn 1) and another adds each P tile's chunks in chunk order, so the workspace holds
// ROWS_BAND x 2 doubles per Q row whatever the number of P tiles, and the summation order is fixed: no floating-point
// atomics, two calls give the same bits, and a block's outputs do not depend on the other blocks of the call.
#include "am_common.h"
#include "kad_common.h"
#include "pairwise_common.h"
#include <algorithm>

namespace am {

constexpr int ROWS_BAND = 64;                        // P tiles per band: 1 KiB of Q-side slots per Q row
constexpr int64_t ROWS_MAX_CHUNKS = 64;              // most Q chunks of a P tile (the P-side partials are per row)
constexpr size_t ROWS_LDS_BYTES = ENGINE_LDS_FLOATS * sizeof(float);      // 73 728 B: two workgroups per CU

template <bool SYM>
struct RowsEpilogue {
    const double* qn;            // f64 squared norms of the Q rows
    int nq, ptile;
    double gamma;
    double sum[LaneInfo::NT];    // the running row sums of this lane's P rows
    double pnorm[LaneInfo::NT];  // +inf for padded rows: exp(-inf) = 0
    double* qout;                // this workgroup's (band slot, wn) slab of Q-side tile sums, by padded Q row
    const LaneInfo& L;
    __device__ __forceinline__ RowsEpilogue(const LaneInfo& l) : L(l) {}
    __device__ __forceinline__ void aux_issue(int, int64_t) {}
    __device__ __forceinline__ void aux_commit(int) {}
    // value number s (0 .. 31) of the tile enters the butterfly; returns the complete sum after s = 31
    __device__ __forceinline__ double push(double (&lvl)[5], int s, double v) const {
#pragma unroll
        for (int l = 0; l < 5; ++l) {
            if (((s >> l) & 1) == 0) {                                  // (s is a constant once the tile loops are unrolled)
                lvl[l] = v;
                break;
            }
            const bool later = ((L.r >> l) & 1) != 0;
            const double keep = later ? v : lvl[l], send = later ? lvl[l] : v;
            v = keep + __shfl_xor(send, 1 << l);
        }
        return v;
    }
    // (rows are indexed in 32 bits: N * ld * 4 < 4 GiB and ld >= 4 put N below 2^28)
    __device__ __forceinline__ void finish(int, int64_t qtile, f32x16 (&acc)[2][2]) {
        const bool diag = SYM && (int)qtile == ptile;                       // workgroup-uniform
        const int q0 = (int)qtile * TB + L.wm * 64 + 4 * L.h;
        // the diagonal tile: q == p where the Q row's offset in the wave's 64 equals self (no offset does elsewhere)
        const int self = diag ? (L.wn - L.wm) * 64 + L.r - 4 * L.h : -TB;
        double lvl[5], done = 0.0;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int qoff = mt * 32 + (i & 3) + 8 * (i >> 2);
                const double qnorm = q0 + qoff < nq ? qn[q0 + qoff] : INFINITY;
                double kq = 0.0;
#pragma unroll
                for (int nt = 0; nt < LaneInfo::NT; ++nt) {
                    double d2 = (qnorm + pnorm[nt]) - 2.0 * (double)acc[mt][nt][i];
                    d2 = d2 < 0.0 ? 0.0 : d2;
                    double k = exp(-d2 * gamma);
                    if constexpr (SYM) k = (self == qoff - nt * 32) ? 0.0 : k;     // dropped by INDEX (a select: NaN goes too)
                    sum[nt] += k;
                    kq = nt == 0 ? k : kq + k;
                }
                done = push(lvl, mt * 16 + i, kq);
                if ((i & 1) == 1) __builtin_amdgcn_sched_barrier(0);    // four exp chains at a time: more in flight spill
            }
        // lane r holds value number r: mt = r >> 4, i = r & 15.  The diagonal tile is the P side's alone.
        if (!diag) qout[q0 + (L.r >> 4) * 32 + (L.r & 3) + 8 * ((L.r & 15) >> 2)] = done;
    }
};

// grid: x = P tile of the band (tp0 + x), y = chunk of `chunk_tiles` Q tiles.
//   pp[(y * ROWS_BAND + x) * 128 + row]    P-side sums of the chunk
//   qp[(x * 2 + wn) * nq_pad + q]          Q-side sums of every tile of the chunk (SYM: but the diagonal one)
template <bool SYM, bool KTAIL>
__global__ void __launch_bounds__(ENGINE_THREADS, 2)
mmd_rows_kernel(const float* __restrict__ Q, int64_t nq, int64_t ldq, const double* __restrict__ qn, const float* __restrict__ P,
                int64_t np, int64_t ldp, const double* __restrict__ pn, int D, int tp0, int chunk_tiles,
                const float* __restrict__ bw2_dev, double gamma, double* __restrict__ pp, double* __restrict__ qp, int64_t nq_pad) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LaneInfo L;
    const int tp = tp0 + (int)blockIdx.x;
    const int64_t q0 = (int64_t)blockIdx.y * chunk_tiles;
    const int64_t qlast = SYM ? (int64_t)tp : (nq + TB - 1) / TB - 1;
    if (q0 > qlast) return;                                                 // the fold kernels know which chunks exist
    const int64_t left = qlast + 1 - q0;
    const int ntiles = left < chunk_tiles ? (int)left : chunk_tiles;
    RowsEpilogue<SYM> epi(L);
    epi.qn = qn;
    epi.nq = (int)nq;
    epi.ptile = tp;
    epi.gamma = bw2_dev != nullptr ? 0.5 / (double)*bw2_dev : gamma;        // the median feeds the sums without a host round trip
    epi.qout = qp + ((int64_t)blockIdx.x * 2 + L.wn) * nq_pad;
#pragma unroll
    for (int nt = 0; nt < LaneInfo::NT; ++nt) {
        const int64_t p = (int64_t)tp * TB + L.wn * 64 + nt * 32 + L.r;
        epi.sum[nt] = 0.0;
        epi.pnorm[nt] = p < np ? pn[p] : INFINITY;
    }
    dense_pipeline_early<EV_DEFAULT, KTAIL>(Q, nq, ldq, LinearTiles{q0}, P, np, ldp, (int64_t)tp * TB, ntiles, D, lds, L, epi);
    // (staging slabs are idle after the pipeline's last barrier)
    fold_p_rows(epi.sum, reinterpret_cast<double*>(lds), L, pp + ((int64_t)blockIdx.y * ROWS_BAND + blockIdx.x) * TB);
}

// pside[p] for the rows of the band's `ntp` P tiles: the tile's chunks in chunk order
__global__ void __launch_bounds__(256) mmd_rows_fold_p_kernel(const double* __restrict__ pp, int nch, int chunk_tiles, int sym, int tp0,
                                                              int ntp, int64_t np, double* __restrict__ pside) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int slot = (int)(e / TB), i = (int)(e % TB);
    if (slot >= ntp) return;
    const int tp = tp0 + slot;
    const int64_t p = (int64_t)tp * TB + i;
    if (p >= np) return;
    const int n = sym ? tp / chunk_tiles + 1 : nch;                         // sym: the chunks that start at or before the diagonal
    double s = 0.0;
    for (int y = 0; y < n; ++y) s += pp[((int64_t)y * ROWS_BAND + slot) * TB + i];
    pside[p] = s;
}

// run[q] (+)= the band's Q-side slots of row q in P-tile order, wn 0 then wn 1.  sym: P tile tp holds row q only for
// tp > tile(q), and the band that holds tile(q) is the first to touch run[q]; else every P tile, band 0 first.
__global__ void __launch_bounds__(256) mmd_rows_fold_q_kernel(const double* __restrict__ qp, int64_t nq_pad, int sym, int tp0, int ntp,
                                                              int64_t nq, double* __restrict__ run) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    const int tq = (int)(q / TB);
    int first = 0;
    bool init = tp0 == 0;
    if (sym) {
        if (tq >= tp0 + ntp) return;
        first = tq + 1 > tp0 ? tq + 1 - tp0 : 0;
        init = tq >= tp0;
    }
    double s = init ? 0.0 : run[q];
    for (int slot = first; slot < ntp; ++slot) {
        s += qp[((int64_t)slot * 2) * nq_pad + q];
        s += qp[((int64_t)slot * 2 + 1) * nq_pad + q];
    }
    run[q] = s;
}

// out[2 i] = a[i] (+ b[i])
__global__ void __launch_bounds__(256) mmd_rows_write_kernel(const double* __restrict__ a, const double* __restrict__ b, int64_t n,
                                                             double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[2 * i] = b != nullptr ? a[i] + b[i] : a[i];
}

// ---------------------------------------------------------------- host side
struct RowsBlock {               // one of XX (b = 0), YY (1), XY (2: P = X, Q = Y)
    int64_t np, nq, TP, TQ;
    int chunk, nch;
    bool sym;
};

static RowsBlock rows_block(int b, int64_t N1, int64_t N2) {
    RowsBlock k;
    k.sym = b < 2;
    k.np = b == 1 ? N2 : N1;
    k.nq = b == 0 ? N1 : N2;
    k.TP = ceil_div(k.np, TB);
    k.TQ = ceil_div(k.nq, TB);
    const int64_t total = k.sym ? k.TP * (k.TP + 1) / 2 : k.TP * k.TQ;
    // per-ROW partials on the P side: the number of chunks is capped where kad.hip's is not
    k.chunk = (int)std::max<int64_t>(kad_chunk(total, k.TQ), ceil_div(k.TQ, ROWS_MAX_CHUNKS));
    k.nch = (int)ceil_div(k.TQ, k.chunk);
    return k;
}

struct RowsWs {
    SetNorms n;
    double *pp, *qp, *pside, *run;
    size_t bytes;
    bool ok;
};

// the norms of the sets in use; the partials and running sums are shared by the blocks, which run one after the other
static RowsWs rows_carve(void* ws, size_t ws_bytes, int64_t N1, int64_t N2, unsigned blocks) {
    Carver c(ws, ws_bytes);
    RowsWs w{};
    w.n = carve_set_norms(c, N1, N2, blocks);
    size_t pp = 0, qp = 0, rows_p = 0, rows_q = 0;
    for (int b = 0; b < 3; ++b) {
        if (!(blocks & (1u << b))) continue;
        const RowsBlock k = rows_block(b, N1, N2);
        pp = std::max(pp, (size_t)k.nch * ROWS_BAND * TB);
        qp = std::max(qp, (size_t)std::min<int64_t>(k.TP, ROWS_BAND) * 2 * (size_t)(k.TQ * TB));
        rows_p = std::max(rows_p, (size_t)k.np);
        rows_q = std::max(rows_q, (size_t)k.nq);
    }
    w.pp = c.take<double>(pp);
    w.qp = c.take<double>(qp);
    w.pside = c.take<double>(rows_p);
    w.run = c.take<double>(rows_q);
    w.bytes = c.off;
    w.ok = c.ok();
    return w;
}

template <bool SYM>
static int rows_sweep(const RowsBlock& k, const float* Q, int64_t ldq, const double* qn, const float* P, int64_t ldp, const double* pn,
                      int D, const float* bw2_dev, double gamma, const RowsWs& w, hipStream_t st) {
    auto launch = [&](auto kernel) -> int {
        AM_HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), (int)ROWS_LDS_BYTES));
        const int64_t nq_pad = k.TQ * TB;
        for (int64_t tp0 = 0; tp0 < k.TP; tp0 += ROWS_BAND) {
            const int ntp = (int)std::min<int64_t>(ROWS_BAND, k.TP - tp0);
            const int nch = SYM ? (int)ceil_div(tp0 + ntp, k.chunk) : k.nch;            // chunks past the band's last diagonal are empty
            hipLaunchKernelGGL(kernel, dim3((unsigned)ntp, (unsigned)nch), dim3(ENGINE_THREADS), ROWS_LDS_BYTES, st, Q, k.nq, ldq, qn,
                               P, k.np, ldp, pn, D, (int)tp0, k.chunk, bw2_dev, gamma, w.pp, w.qp, nq_pad);
            AM_LAUNCH_CHECK();
            hipLaunchKernelGGL(mmd_rows_fold_p_kernel, dim3((unsigned)ceil_div((int64_t)ntp * TB, 256)), dim3(256), 0, st,
                               (const double*)w.pp, nch, k.chunk, SYM ? 1 : 0, (int)tp0, ntp, k.np, w.pside);
            AM_LAUNCH_CHECK();
            const int64_t qlim = SYM ? std::min<int64_t>(k.nq, (tp0 + ntp) * TB) : k.nq;
            hipLaunchKernelGGL(mmd_rows_fold_q_kernel, dim3((unsigned)ceil_div(qlim, 256)), dim3(256), 0, st, (const double*)w.qp,
                               nq_pad, SYM ? 1 : 0, (int)tp0, ntp, k.nq, w.run);
            AM_LAUNCH_CHECK();
        }
        return AM_OK;
    };
    return (D % BK) != 0 ? launch(&mmd_rows_kernel<SYM, true>) : launch(&mmd_rows_kernel<SYM, false>);
}

static int rows_write(const double* a, const double* b, int64_t n, double* out, hipStream_t st) {
    hipLaunchKernelGGL(mmd_rows_write_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, a, b, n, out);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

}  // namespace am

using namespace am;

extern "C" size_t am_mmd_rbf_rows_workspace_bytes(int64_t N1, int64_t N2, int D, unsigned blocks) {
    if (N1 < 1 || N2 < 1 || D < 1 || blocks == 0 || (blocks & ~7u) != 0) return 0;
    return rows_carve(nullptr, 0, N1, N2, blocks).bytes;
}

extern "C" int am_mmd_rbf_rows_f32(const float* X, int64_t N1, int64_t ldx, const float* Y, int64_t N2, int64_t ldy, int D,
                                   const float* bw2_dev, double gamma, unsigned blocks, double* out_x, double* out_y, void* ws,
                                   size_t ws_bytes, am_stream_t stream) {
    AM_REQUIRE(out_x || !(blocks & (AM_MMD_XX | AM_MMD_XY)), AM_ERR_BAD_ARG, "null pointer: out_x is written by AM_MMD_XX and AM_MMD_XY");
    AM_REQUIRE(out_y || !(blocks & (AM_MMD_YY | AM_MMD_XY)), AM_ERR_BAD_ARG, "null pointer: out_y is written by AM_MMD_YY and AM_MMD_XY");
    int rc = check_two_sets_f32(X, N1, ldx, Y, N2, ldy, D, blocks);
    if (rc != AM_OK) return rc;
    AM_REQUIRE(bw2_dev != nullptr || gamma >= 0.0, AM_ERR_BAD_ARG, "gamma must be >= 0 (or bw2_dev given)");
    const RowsWs w = rows_carve(ws, ws_bytes, N1, N2, blocks);
    AM_REQUIRE(w.ok, AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (am_mmd_rbf_rows_workspace_bytes), have %zu", w.bytes,
               ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = launch_set_norms(X, N1, ldx, Y, N2, ldy, D, w.n, st);
    if (rc == AM_OK && (blocks & AM_MMD_XX)) {
        rc = rows_sweep<true>(rows_block(0, N1, N2), X, ldx, w.n.n1, X, ldx, w.n.n1, D, bw2_dev, gamma, w, st);
        if (rc == AM_OK) rc = rows_write(w.pside, w.run, N1, out_x, st);
    }
    if (rc == AM_OK && (blocks & AM_MMD_YY)) {
        rc = rows_sweep<true>(rows_block(1, N1, N2), Y, ldy, w.n.n2, Y, ldy, w.n.n2, D, bw2_dev, gamma, w, st);
        if (rc == AM_OK) rc = rows_write(w.pside, w.run, N2, out_y, st);
    }
    if (rc == AM_OK && (blocks & AM_MMD_XY)) {
        rc = rows_sweep<false>(rows_block(2, N1, N2), Y, ldy, w.n.n2, X, ldx, w.n.n1, D, bw2_dev, gamma, w, st);
        if (rc == AM_OK) rc = rows_write(w.pside, nullptr, N1, out_x + 1, st);
        if (rc == AM_OK) rc = rows_write(w.run, nullptr, N2, out_y + 1, st);
    }
    return rc;
}
