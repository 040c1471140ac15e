// float64 forms of the three Kernel Audio Distance calls (kad.hip, kad_groups.hip) on the f64 tile engine (f64_engine.h:
// 64 x 64 tiles on v_mfma_f64_16x16x4_f64).  They are taken when BOTH sets hold float64 rows - what a float64 embedder
// yields and what the PCA projection hands on - and keep every step in f64, as the other float64 entry points do.
//
// Arithmetic of one pair, all in f64: dot = the MFMA chain, norms = the loop of row_sqnorm64_kernel,
//   select: d2 = clamp0d(fma(-2, dot, |a|^2 + |b|^2))          a NaN distance (a non-finite row) is carried as +inf
//   sums:   d2 = max(fma(-2, dot, |a|^2 + |b|^2), 0) with a NaN left in place, k = exp(-d2 gamma): as in the f32 forms a
//           non-finite row makes the sums it takes part in NaN instead of dropping out of them silently.
//
// am_pairwise_select_f64: the contract of the f32 form - the result is a FLOAT32, rn32 of the f64 order statistic (rounding
//   is monotone: select-then-round = round-then-select), so the bandwidth keeps its float32 device scalar.  Keys are
//   bits(rn32(d2)), NaN and overflow +inf; three radix passes of 11 / 10 / 10 bits over the upper-triangular tiles (P tile
//   tp against Q tiles 0 .. tp, a pair counts where p > q), a per-workgroup LDS histogram flushed once into 64-bit global
//   bins, a one-workgroup scan between passes, no host synchronisation.  Equal digits of a wave are combined before any
//   LDS atomic (hist_add: the reasoning is at the head of kad.hip).
// am_mmd_rbf_f64: Sxx, Syy (upper-triangular tiles, off-diagonal tiles weighted 2, diagonal entries dropped) and Sxy; one
//   f64 partial per workgroup in a slot of its own, summed by one workgroup in a fixed order: no atomics, same bits.
// Nothing that is independent of the element type is repeated here: the select's state, digits and scan, the reduce kernel,
// the grid plan, the chunk rules and the workspace carves are those of the f32 forms (kad_common.h), at 64-row tiles.
// am_mmd_rbf_groups_f64: the contract of kad_groups.hip by LIST POSITION p < n_total:
//   kadg64_prep_kernel    per position: its stored row (-1 for an index outside [0, N1): never dereferenced, the position
//                         goes to the flag word, the row counts as zeros), its squared norm and its group; the tail up to
//                         the next multiple of 64 is padding (row -1, group -1)
//   kadg64_rows_kernel    64 x 64 tiles.  P rows (lane axis) = 64 consecutive positions gathered through the row list - no
//                         gathered copy exists; Q rows = the dense reference rows (cross) or the positions of the tile's
//                         own groups gathered the same way (within: masked by gid[q] == gid[p] && q != p).  In this engine
//                         everything a lane accumulates belongs to ONE P row: a lane keeps one running sum, and the four
//                         lanes of a row (l4 = 0 .. 3) are added in a fixed order at the end -> partial[chunk][position]
//   kadg_rowsum_kernel    per position: its chunks in chunk order -> rows[p] = {w_p, c_p}               (kad_groups.hip)
//   kadg_finish_kernel    one workgroup per group: strided per-thread sums, then a tree -> out_groups[b] = {Sxx_b, Sxy_b}
//   The result depends on the list order only; two calls give the same bits.
// Rows need no alignment (8-byte loads) and no buffer descriptor is used: the 4 GiB limit of the f32 forms does not apply.
#include "am_common.h"
#include "f64_engine.h"
#include "groups_common.h"
#include "kad_common.h"
#include <algorithm>

namespace am {

// out[i] = |X[i]|^2 (one wave per row, fixed order: the loop of row_sqnorm64_kernel)
__device__ __forceinline__ double kad64_sqnorm(const double* __restrict__ x, int D, int lane) {
    double s = 0.0;
    if (x != nullptr)
        for (int k = lane; k < D; k += 64) s = fma(x[k], x[k], s);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

__global__ void __launch_bounds__(256) kad64_norms_kernel(const double* __restrict__ X, int64_t N, int64_t ld, int D,
                                                          double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const double s = kad64_sqnorm(X + row * ld, D, lane);
    if (lane == 0) out[row] = s;
}

// grid: x = P tile (heaviest first), y = chunk of `chunk_tiles` Q tiles; chunks past the diagonal have nothing to do
template <int PASS>
__global__ void __launch_bounds__(FTHREADS)
kad64_select_kernel(const double* __restrict__ X, int64_t N, int64_t ld, int D, const double* __restrict__ norm, int chunk_tiles,
                    const SelectState* __restrict__ state, unsigned long long* __restrict__ bins) {
    __shared__ __attribute__((aligned(16))) double stages[FENGINE_DOUBLES];
    __shared__ double qnorm[FT];
    __shared__ unsigned hist[KAD_BINS];
    const FLane L;
    const int64_t T = (N + FT - 1) / FT;
    const int64_t tp = T - 1 - (int64_t)blockIdx.x;
    const int64_t q0 = (int64_t)blockIdx.y * chunk_tiles;
    if (q0 > tp) return;
    const int64_t q1 = q0 + chunk_tiles < tp + 1 ? q0 + chunk_tiles : tp + 1;
    for (int b = L.tid; b < KAD_BINS; b += FTHREADS) hist[b] = 0u;      // visible after the first barrier of the first tile
    const unsigned prefix = PASS == 0 ? 0u : state->prefix;
    const int64_t p = tp * FT + L.prow();
    const bool pok = p < N;
    const double pn = pok ? norm[p] : 0.0;
    const DenseRows64 prows{X, ld, N, tp * FT};
    for (int64_t t = q0; t < q1; ++t) {
        if (L.tid < FT) {
            const int64_t j = t * FT + L.tid;
            qnorm[L.tid] = j < N ? norm[j] : 0.0;
        }
        f64x4 acc[4];
        zero4(acc);
        f64_tile(DenseRows64{X, ld, N, t * FT}, prows, D, stages, L, acc);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qr = L.qrow(m, r);
                const double d2 = clamp0d(fma(-2.0, acc[m][r], pn + qnorm[qr]));
                float kf = (float)d2;                                   // round to nearest: monotone
                kf = kf < INFINITY ? kf : INFINITY;                     // overflow: +inf (a NaN is +inf already)
                const unsigned key = __float_as_uint(kf) & 0x7fffffffu;
                bool live = pok && t * FT + qr < p;                     // each unordered pair once (q < p < N)
                unsigned digit;                                         // (in line, as in kad.hip)
                if constexpr (PASS == 0) {
                    digit = key >> 20;
                } else if constexpr (PASS == 1) {
                    live = live && (key >> 20) == prefix;
                    digit = (key >> 10) & 1023u;
                } else {
                    live = live && (key >> 10) == prefix;
                    digit = key & 1023u;
                }
                hist_add(hist, digit, live, L.lane);
            }
        __syncthreads();                                                // qnorm is rewritten by the next tile; the counters are complete
    }
    for (int b = L.tid; b < KAD_BINS; b += FTHREADS) {                  // one global flush per workgroup
        const unsigned c = hist[b];
        if (c != 0u) atomicAdd(bins + b, (unsigned long long)c);
    }
}

template <int PASS>
static int launch_select64_pass(const double* X, int64_t N, int64_t ld, int D, const double* norm, int chunk, SelectState* state,
                                unsigned long long* bins, unsigned long long rank0, float* out, hipStream_t st) {
    const int64_t T = ceil_div(N, FT);
    hipLaunchKernelGGL(kad64_select_kernel<PASS>, dim3((unsigned)T, (unsigned)ceil_div(T, chunk)), dim3(FTHREADS), 0, st, X, N, ld, D, norm,
                       chunk, (const SelectState*)state, bins + (size_t)PASS * KAD_BINS);
    AM_LAUNCH_CHECK();
    return launch_kad_scan(PASS, bins + (size_t)PASS * KAD_BINS, state, rank0, out, st);
}

// ------------------------------------------------------------------------------------------------ kernel sums
// grid: x = P tile, y = chunk of Q tiles; partial[y * gridDim.x + x] = this workgroup's weighted sum (0 for an empty chunk).
// Kxy[a][b] = k(x_a, y_b): Q rows (register axis) from set 1, P rows (lane axis) from set 2.
__global__ void __launch_bounds__(FTHREADS)
kad64_mmd_kernel(const double* __restrict__ Q, int64_t nq, int64_t ldq, const double* __restrict__ qn, const double* __restrict__ P,
                 int64_t np, int64_t ldp, const double* __restrict__ pn, int D, int sym, int chunk_tiles,
                 const float* __restrict__ bw2_dev, double gamma, double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) double stages[FENGINE_DOUBLES];
    __shared__ double qnorm[FT];
    __shared__ double red[4];
    const FLane L;
    const int64_t TQ = (nq + FT - 1) / FT, TP = (np + FT - 1) / FT;
    const int64_t tp = sym ? TP - 1 - (int64_t)blockIdx.x : (int64_t)blockIdx.x;
    const int64_t q0 = (int64_t)blockIdx.y * chunk_tiles;
    const int64_t qlast = sym ? tp : TQ - 1;
    const int64_t slot = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (q0 > qlast) {
        if (L.tid == 0) partial[slot] = 0.0;
        return;
    }
    const int64_t q1 = q0 + chunk_tiles < qlast + 1 ? q0 + chunk_tiles : qlast + 1;
    const double g = bw2_dev != nullptr ? 0.5 / (double)*bw2_dev : gamma;   // the median feeds the sums without a host round trip
    const int64_t p = tp * FT + L.prow();
    const bool pok = p < np;
    const double pnorm = pok ? pn[p] : 0.0;
    const DenseRows64 prows{P, ldp, np, tp * FT};
    double sum = 0.0;
    for (int64_t t = q0; t < q1; ++t) {
        if (L.tid < FT) {
            const int64_t j = t * FT + L.tid;
            qnorm[L.tid] = j < nq ? qn[j] : 0.0;
        }
        f64x4 acc[4];
        zero4(acc);
        f64_tile(DenseRows64{Q, ldq, nq, t * FT}, prows, D, stages, L, acc);
        const bool diag = sym && t == tp;
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qr = L.qrow(m, r);
                const int64_t q = t * FT + qr;
                double d2 = fma(-2.0, acc[m][r], pnorm + qnorm[qr]);
                d2 = d2 < 0.0 ? 0.0 : d2;
                const double k = exp(-d2 * g);
                s += (pok && q < nq && !(diag && q == p)) ? k : 0.0;    // a select: what a padded row gives is dropped
            }
        sum += (sym && !diag) ? 2.0 * s : s;
        __syncthreads();                                                // qnorm is rewritten by the next tile
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    if (L.lane == 0) red[L.wave] = sum;
    __syncthreads();
    if (L.tid == 0) partial[slot] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ------------------------------------------------------------------------------------------------ per-group sums
// one wave per list position (padding included)
__global__ void __launch_bounds__(256) kadg64_prep_kernel(const double* __restrict__ X, int64_t N1, int64_t ld, int D,
                                                          const int64_t* __restrict__ idx, const int64_t* __restrict__ offs, int B,
                                                          int64_t n_total, int64_t n_pad, int64_t* __restrict__ rowof,
                                                          double* __restrict__ norm, int* __restrict__ gid,
                                                          unsigned long long* __restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= n_pad) return;
    if (p >= n_total) {
        if (lane == 0) {
            rowof[p] = -1;
            norm[p] = 0.0;
            gid[p] = -1;
        }
        return;
    }
    const int64_t row = idx ? idx[p] : p;
    const bool ok = (unsigned long long)row < (unsigned long long)N1;
    const double s = kad64_sqnorm(ok ? X + row * ld : nullptr, D, lane);
    if (lane == 0) {
        if (!ok) atomicMax(flag, (unsigned long long)p + 1ull);
        rowof[p] = ok ? row : -1;
        norm[p] = s;
        gid[p] = group_of(offs, B, p);
    }
}

// rows gathered through the checked row list: local row -> X[rowof[pos0 + row]], a zero row where the list holds -1
// (pos0 + row stays inside the padded list)
struct ListRows64 {
    const double* base;
    int64_t ld;
    const int64_t* rowof;
    int64_t pos0;
    __device__ __forceinline__ const double* operator()(int row) const {
        const int64_t r = rowof[pos0 + row];
        return r >= 0 ? base + r * ld : nullptr;
    }
};

// grid: x = P tile (64 list positions), y = chunk of `chunk_tiles` Q tiles.  partial[y * n_pad + position].
template <bool WITHIN>
__global__ void __launch_bounds__(FTHREADS)
kadg64_rows_kernel(const double* __restrict__ X, int64_t ldx, const int64_t* __restrict__ rowof, const double* __restrict__ xn,
                   const int* __restrict__ gid, const int64_t* __restrict__ offs, int64_t n_total, int64_t n_pad,
                   const double* __restrict__ Y, int64_t N2, int64_t ldy, const double* __restrict__ yn, int D, int chunk_tiles,
                   const float* __restrict__ bw2_dev, double gamma, double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) double stages[FENGINE_DOUBLES];
    __shared__ double qnorm[FT];
    __shared__ int qgid[FT];
    const FLane L;
    const int64_t tp = (int64_t)blockIdx.x;
    double* out = partial + (int64_t)blockIdx.y * n_pad + tp * FT;
    int64_t qlo = 0, qhi = (N2 + FT - 1) / FT - 1;                          // cross: every reference tile
    if constexpr (WITHIN) {
        const int64_t pfirst = tp * FT, plast = (pfirst + FT < n_total ? pfirst + FT : n_total) - 1;
        qlo = offs[gid[pfirst]] / FT;
        qhi = (offs[gid[plast] + 1] - 1) / FT;
    }
    const int64_t q0 = qlo + (int64_t)blockIdx.y * chunk_tiles;
    if (q0 > qhi) {                                                         // within: this P tile's range has fewer chunks
        if (L.tid < FT) out[L.tid] = 0.0;
        return;
    }
    const int64_t q1 = q0 + chunk_tiles < qhi + 1 ? q0 + chunk_tiles : qhi + 1;
    const double g = bw2_dev != nullptr ? 0.5 / (double)*bw2_dev : gamma;   // the median feeds the sums without a host round trip
    const int64_t p = tp * FT + L.prow();                                   // < n_pad
    const double pnorm = xn[p];
    const int pg = p < n_total ? gid[p] : -2;                               // padding: equal to no Q row's group
    const ListRows64 prows{X, ldx, rowof, tp * FT};
    double sum = 0.0;
    for (int64_t t = q0; t < q1; ++t) {
        if (L.tid < FT) {
            const int64_t j = t * FT + L.tid;
            if constexpr (WITHIN) {
                qnorm[L.tid] = xn[j];                                       // the Q range ends inside the padded list
                qgid[L.tid] = gid[j];
            } else {
                qnorm[L.tid] = j < N2 ? yn[j] : 0.0;
                qgid[L.tid] = j < N2 ? 0 : -1;
            }
        }
        f64x4 acc[4];
        zero4(acc);
        if constexpr (WITHIN) f64_tile(ListRows64{X, ldx, rowof, t * FT}, prows, D, stages, L, acc);
        else f64_tile(DenseRows64{Y, ldy, N2, t * FT}, prows, D, stages, L, acc);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qr = L.qrow(m, r);
                double d2 = fma(-2.0, acc[m][r], pnorm + qnorm[qr]);
                d2 = d2 < 0.0 ? 0.0 : d2;
                const double k = exp(-d2 * g);
                // a select: a NaN of another group, or what a padded row gives, is dropped
                if constexpr (WITHIN) sum += (qgid[qr] == pg && t * FT + qr != p) ? k : 0.0;
                else sum += qgid[qr] == 0 ? k : 0.0;
            }
        __syncthreads();                                                    // qnorm / qgid are rewritten by the next tile
    }
    // the four lanes of a P row (l4 = 0 .. 3) saw disjoint Q rows: added in a fixed order
    const double s1 = sum + __shfl_xor(sum, 16);
    const double s2 = s1 + __shfl_xor(s1, 32);
    if (L.l4 == 0) out[L.prow()] = s2;
}

struct Groups64Plan {
    int64_t TP, TQ, n_pad;
    int chunk_c, nch_c;          // cross pass
};

static Groups64Plan groups64_plan(int64_t n_total, int64_t N2) {
    Groups64Plan p;
    p.TP = ceil_div(n_total, FT);
    p.TQ = ceil_div(N2, FT);
    p.n_pad = p.TP * FT;
    p.chunk_c = kadg_cross_chunk(p.TP, p.TQ);            // 64 doubles per (P tile, chunk)
    p.nch_c = (int)ceil_div(p.TQ, p.chunk_c);
    return p;
}

struct Groups64Ws {
    GroupHead head;
    int64_t* rowof;
    int* gid;
    double *xn, *yn, *rows, *pw, *pc;
};

static bool groups64_carve(Carver& c, int64_t n_total, int B, int64_t N2, const Groups64Plan& p, Groups64Ws& w) {
    w.head = carve_group_head(c, B);
    w.rowof = c.take<int64_t>((size_t)p.n_pad);
    w.gid = c.take<int>((size_t)p.n_pad);
    w.xn = c.take<double>((size_t)p.n_pad);
    w.yn = c.take<double>((size_t)N2);
    w.rows = c.take<double>(2 * (size_t)n_total);
    w.pw = c.take<double>((size_t)std::min<int64_t>(p.TP, KADG_WITHIN_CHUNKS) * (size_t)p.n_pad);
    w.pc = c.take<double>((size_t)p.nch_c * (size_t)p.n_pad);
    return c.ok();
}

}  // namespace am

using namespace am;

extern "C" size_t am_pairwise_select_f64_workspace_bytes(int64_t N, int D) {
    if (N < 2 || D < 1) return 0;
    return select_carve(nullptr, 0, N).bytes;
}

extern "C" int am_pairwise_select_f64(const double* X, int64_t N, int64_t ld, int D, int64_t rank, float* out_d2, void* ws,
                                      size_t ws_bytes, am_stream_t stream) {
    AM_REQUIRE(X && out_d2, AM_ERR_BAD_ARG, "null pointer");
    AM_REQUIRE(N >= 2 && D >= 1, AM_ERR_BAD_SHAPE, "N=%lld D=%d: an order statistic of pairwise distances needs two rows",
               (long long)N, D);
    AM_REQUIRE(N < ((int64_t)1 << 31), AM_ERR_BAD_SHAPE, "N=%lld: the pair count must fit 64 bits (N < 2^31)", (long long)N);
    AM_REQUIRE(ld >= D, AM_ERR_BAD_ARG, "ld < D (ld=%lld D=%d)", (long long)ld, D);
    const int64_t pairs = N * (N - 1) / 2;
    AM_REQUIRE(rank < pairs, AM_ERR_BAD_SHAPE, "rank %lld of %lld pairs", (long long)rank, (long long)pairs);
    if (rank < 0) rank = (pairs - 1) / 2;                // lower median (torch.median's convention)
    const SelectWs w = select_carve(ws, ws_bytes, N);
    AM_REQUIRE(w.ok, AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (am_pairwise_select_f64_workspace_bytes), have %zu", w.bytes,
               ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AM_HIP_TRY(hipMemsetAsync(w.bins, 0, (size_t)KAD_PASSES * KAD_BINS * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(kad64_norms_kernel, dim3((unsigned)ceil_div(N, 4)), dim3(256), 0, st, X, N, ld, D, w.norm);
    AM_LAUNCH_CHECK();
    const int64_t T = ceil_div(N, FT);
    const int chunk = kad_chunk(T * (T + 1) / 2, T);
    int rc = launch_select64_pass<0>(X, N, ld, D, w.norm, chunk, w.state, w.bins, (unsigned long long)rank, out_d2, st);
    if (rc == AM_OK) rc = launch_select64_pass<1>(X, N, ld, D, w.norm, chunk, w.state, w.bins, 0ull, out_d2, st);
    if (rc == AM_OK) rc = launch_select64_pass<2>(X, N, ld, D, w.norm, chunk, w.state, w.bins, 0ull, out_d2, st);
    return rc;
}

extern "C" size_t am_mmd_rbf_f64_workspace_bytes(int64_t N1, int64_t N2, int D, unsigned blocks) {
    if (N1 < 1 || N2 < 1 || D < 1 || (blocks & 7u) == 0) return 0;
    return mmd_carve(nullptr, 0, N1, N2, 1, blocks & 7u, mmd_plan(N1, N2, FT)).bytes;
}

extern "C" int am_mmd_rbf_f64(const double* X, int64_t N1, int64_t ldx, const double* Y, int64_t N2, int64_t ldy, int D,
                              const float* bw2_dev, double gamma, unsigned blocks, double* out_sums, void* ws, size_t ws_bytes,
                              am_stream_t stream) {
    AM_REQUIRE(X && Y && out_sums, AM_ERR_BAD_ARG, "null pointer");
    AM_REQUIRE(blocks != 0 && (blocks & ~7u) == 0, AM_ERR_BAD_ARG, "blocks = %u is not a mask of AM_MMD_XX | AM_MMD_YY | AM_MMD_XY", blocks);
    AM_REQUIRE(N1 >= 1 && N2 >= 1 && D >= 1, AM_ERR_BAD_SHAPE, "N1=%lld N2=%lld D=%d", (long long)N1, (long long)N2, D);
    AM_REQUIRE(N1 < ((int64_t)1 << 31) && N2 < ((int64_t)1 << 31), AM_ERR_BAD_SHAPE, "N1=%lld N2=%lld (each must stay below 2^31)",
               (long long)N1, (long long)N2);
    AM_REQUIRE(ldx >= D && ldy >= D, AM_ERR_BAD_ARG, "ld < D (ldx=%lld ldy=%lld D=%d)", (long long)ldx, (long long)ldy, D);
    AM_REQUIRE(bw2_dev != nullptr || gamma >= 0.0, AM_ERR_BAD_ARG, "gamma must be >= 0 (or bw2_dev given)");
    const MmdPlan plan = mmd_plan(N1, N2, FT);
    const MmdWs w = mmd_carve(ws, ws_bytes, N1, N2, 1, blocks, plan);
    AM_REQUIRE(w.ok, AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (am_mmd_rbf_f64_workspace_bytes), have %zu", w.bytes, ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (w.n.n1) hipLaunchKernelGGL(kad64_norms_kernel, dim3((unsigned)ceil_div(N1, 4)), dim3(256), 0, st, X, N1, ldx, D, w.n.n1);
    if (w.n.n2) hipLaunchKernelGGL(kad64_norms_kernel, dim3((unsigned)ceil_div(N2, 4)), dim3(256), 0, st, Y, N2, ldy, D, w.n.n2);
    AM_LAUNCH_CHECK();
    for (int b = 0; b < 3; ++b) {
        if (!(blocks & (1u << b))) continue;
        const bool q_is_y = b == 1, p_is_x = b == 0;
        hipLaunchKernelGGL(kad64_mmd_kernel, plan.grid[b], dim3(FTHREADS), 0, st, q_is_y ? Y : X, q_is_y ? N2 : N1, q_is_y ? ldy : ldx,
                           (const double*)(q_is_y ? w.n.n2 : w.n.n1), p_is_x ? X : Y, p_is_x ? N1 : N2, p_is_x ? ldx : ldy,
                           (const double*)(p_is_x ? w.n.n1 : w.n.n2), D, b < 2 ? 1 : 0, plan.chunk[b], bw2_dev, gamma, w.partial[b]);
        AM_LAUNCH_CHECK();
        AM_TRY(launch_mmd_reduce(w.partial[b], (int64_t)plan.slots[b], 1, out_sums + b, st));
    }
    return AM_OK;
}

extern "C" size_t am_mmd_rbf_groups_f64_workspace_bytes(int64_t n_total, int B, int64_t N2, int D) {
    if (n_total < 1 || B < 1 || N2 < 2 || D < 1 || n_total >= ((int64_t)1 << 30)) return 0;
    Carver c(nullptr, 0);
    Groups64Ws w;
    groups64_carve(c, n_total, B, N2, groups64_plan(n_total, N2), w);
    return c.off;
}

extern "C" int am_mmd_rbf_groups_f64(const double* X, int64_t N1, int64_t ldx, const int64_t* idx, const int64_t* offsets, int B,
                                     const double* Y, int64_t N2, int64_t ldy, int D, const float* bw2_dev, double gamma,
                                     double* out_groups, double* out_rows, void* ws, size_t ws_bytes, am_stream_t stream) {
    AM_REQUIRE(X && offsets && Y && out_groups, AM_ERR_BAD_ARG, "null pointer (X, offsets, Y, out_groups)");
    AM_REQUIRE(N1 >= 1 && D >= 1 && B >= 1, AM_ERR_BAD_SHAPE, "X has shape %lld x %d, B=%d (all must be >= 1)", (long long)N1, D, B);
    AM_REQUIRE(N2 >= 2 && N2 < ((int64_t)1 << 31), AM_ERR_BAD_SHAPE,
               "N2=%lld: the unbiased MMD^2 needs two reference rows (and fewer than 2^31)", (long long)N2);
    AM_TRY(check_group_rows(X, N1, ldx, D));
    AM_REQUIRE(ldy >= D, AM_ERR_BAD_ARG, "ldy < D (ldy=%lld, D=%d)", (long long)ldy, D);
    AM_REQUIRE(bw2_dev != nullptr || gamma >= 0.0, AM_ERR_BAD_ARG, "gamma must be >= 0 (or bw2_dev given)");
    int64_t n_total;
    AM_TRY(check_group_offsets(offsets, B, 0, &n_total));
    AM_REQUIRE(n_total < ((int64_t)1 << 30), AM_ERR_BAD_SHAPE, "offsets name %lld list positions (must stay below 2^30)", (long long)n_total);
    AM_TRY(check_stored_rows(idx, n_total, N1));
    const Groups64Plan plan = groups64_plan(n_total, N2);
    Carver c(ws, ws_bytes);
    Groups64Ws w;
    AM_REQUIRE(groups64_carve(c, n_total, B, N2, plan, w), AM_ERR_WORKSPACE,
               "workspace too small: need %zu bytes (am_mmd_rbf_groups_f64_workspace_bytes), have %zu", c.off, ws_bytes);
    const int64_t span = kadg_within_span(offsets, plan.TP, n_total, FT);
    const int chunk_w = kadg_within_chunk(span);
    const int nch_w = (int)ceil_div(span, chunk_w);      // <= min(TP, KADG_WITHIN_CHUNKS)
    hipStream_t st = static_cast<hipStream_t>(stream);
    AM_TRY(upload_group_head(w.head, offsets, B, st));
    const int64_t* offs = w.head.offs;
    hipLaunchKernelGGL(kad64_norms_kernel, dim3((unsigned)ceil_div(N2, 4)), dim3(256), 0, st, Y, N2, ldy, D, w.yn);
    AM_LAUNCH_CHECK();
    hipLaunchKernelGGL(kadg64_prep_kernel, dim3((unsigned)ceil_div(plan.n_pad, 4)), dim3(256), 0, st, X, N1, ldx, D, idx, offs, B, n_total,
                       plan.n_pad, w.rowof, w.xn, w.gid, w.head.flag);
    AM_LAUNCH_CHECK();
    hipLaunchKernelGGL(kadg64_rows_kernel<false>, dim3((unsigned)plan.TP, (unsigned)plan.nch_c), dim3(FTHREADS), 0, st, X, ldx,
                       (const int64_t*)w.rowof, (const double*)w.xn, (const int*)w.gid, offs, n_total, plan.n_pad, Y, N2, ldy,
                       (const double*)w.yn, D, plan.chunk_c, bw2_dev, gamma, w.pc);
    AM_LAUNCH_CHECK();
    hipLaunchKernelGGL(kadg64_rows_kernel<true>, dim3((unsigned)plan.TP, (unsigned)nch_w), dim3(FTHREADS), 0, st, X, ldx,
                       (const int64_t*)w.rowof, (const double*)w.xn, (const int*)w.gid, offs, n_total, plan.n_pad, Y, N2, ldy,
                       (const double*)w.yn, D, chunk_w, bw2_dev, gamma, w.pw);
    AM_LAUNCH_CHECK();
    double* rows = out_rows ? out_rows : w.rows;
    AM_TRY(launch_kadg_rowsum(w.pw, nch_w, w.pc, plan.nch_c, plan.n_pad, n_total, rows, st));
    return launch_kadg_finish(rows, offs, B, out_groups, st);
}
