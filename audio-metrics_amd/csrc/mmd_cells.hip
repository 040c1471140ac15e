// Unit-pair sums of the Gaussian kernel blocks of the unbiased MMD^2 (am_mmd_rbf_cells_f32): what a permutation test of the
// MMD^2 is built from.  A relabelling of exchangeable units only regroups pair sums, so ONE Gram sweep that keeps a sum per
// pair of units prices any number of permutations at one small f64 matmul on the host side of the library.
//
// A set is a list of POSITIONS (position p of X is row idx_x[p]; no list: the rows in stored order).  Cell a of a set is its
// positions [32 a, 32 a + 32), and the value of the cell pair (a, b) is sum k(p, q) over its positions, p != q inside one set.
//
// Arithmetic of one pair: that of MmdEpilogue::finish in kad.hip - d2 = max((|a|^2 + |b|^2) - 2 dot, 0) in f64, f64 norms,
// f32 matrix-core dot product, k = exp(-d2 gamma) in f64.
//
//   cells_prep_kernel    per position: the byte offset of its stored row and its f64 squared norm (the loop of
//                        kad_norms_kernel).  An index outside [0, N) is an EMPTY position: never dereferenced (offset HOLE,
//                        the load returns 0), norm +inf -> k = 0; any such value but -1 also goes to the flag word.  The tail up
//                        to the next multiple of 128 is empty too.
//   mmd_cells_kernel     128 x 128 tiles on the f32 tile engine, BOTH operands gathered through the offset tables (dense and
//                        listed input take the one path).  The accumulator tile of a wave is 2 x 2 sub-blocks of 32 x 32 =
//                        four cell pairs, each held entirely by the wave: 16 values per lane, added in register order, then
//                        ONE xor tree over the 64 lanes for all four (the lanes split the four values between them in the
//                        first two steps: 7 exchanges, the additions of a plain tree per value).  Every cell pair belongs to
//                        exactly one wave of one workgroup and is written once - no partials, no fold, no atomics.
//                        XX / YY sweep the upper-triangular tiles and mirror every value ([a][b] and [b][a] hold one value
//                        written twice); of the diagonal tile the cells a <= b are kept, q == p dropped by POSITION.  XY: P = X,
//                        Q = Y, every tile once.
//   cells_units_kernel   with unit offsets: out[u][v] = the cells of the unit pair in row-major cell order, one thread each.
#include "am_common.h"
#include "groups_common.h"
#include "kad_common.h"
#include "pairwise_common.h"
#include <algorithm>

namespace am {

constexpr unsigned CELLS_HOLE = 0xffffffffu;         // voffset past every descriptor: the load returns 0
constexpr int CELL = AM_MMD_CELL;
constexpr size_t CELLS_LDS_BYTES = ENGINE_LDS_FLOATS * sizeof(float);      // 73 728 B: two workgroups per CU
static_assert(CELL == 32 && TB == 4 * CELL, "a 128 x 128 tile is 4 x 4 cells, one per 32 x 32 accumulator sub-block");

// one wave per position of the padded list
__global__ void __launch_bounds__(256) cells_prep_kernel(const float* __restrict__ X, int64_t N, int64_t ld, int D,
                                                         const int64_t* __restrict__ idx, int64_t n_pos, int64_t n_pad,
                                                         unsigned* __restrict__ rowoff, double* __restrict__ norm,
                                                         unsigned long long* __restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= n_pad) return;
    const int64_t row = p < n_pos ? (idx ? idx[p] : p) : -1;
    const bool ok = (unsigned long long)row < (unsigned long long)N;
    double acc = 0.0;
    if (ok) {
        const float* x = X + row * ld;
        for (int k = lane * 4; k < D; k += 256) {
            const f32x4 v = load_k4(x, k, D);
            acc += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) {
        if (!ok && row != -1) atomicMax(flag, (unsigned long long)p + 1ull);       // (an integer maximum: order-free)
        rowoff[p] = ok ? (unsigned)(row * ld * 4) : CELLS_HOLE;                    // N * ld * 4 < 4 GiB
        norm[p] = ok ? acc : INFINITY;
    }
}

template <bool SYM>
struct CellsEpilogue {
    const double* qn;            // f64 squared norms of the padded Q positions (+inf for empty ones: exp(-inf) = 0)
    int qtile0, ptile;
    int cq, cp;                  // cells of the Q / P list
    int64_t ldo;                 // row stride of out: SYM cp (= cq); else cq (out[P cell][Q cell])
    double gamma;
    double pnorm[LaneInfo::NT];
    double* out;
    const LaneInfo& L;
    __device__ __forceinline__ CellsEpilogue(const LaneInfo& l) : L(l) {}
    __device__ __forceinline__ void aux_issue(int, int64_t) {}
    __device__ __forceinline__ void aux_commit(int) {}
    // (positions are indexed in 32 bits: n_pos < 2^30)
    __device__ __forceinline__ void finish(int t, int64_t, f32x16 (&acc)[2][2]) {
        const int qtile = qtile0 + t;
        const bool diag = SYM && qtile == ptile;                            // workgroup-uniform
        const int qc0 = qtile * 4 + L.wm * 2, pc0 = ptile * 4 + L.wn * 2;   // the wave's first Q / P cell
        const int q0 = qc0 * CELL + 4 * L.h;
        double s[2][LaneInfo::NT];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
            for (int nt = 0; nt < LaneInfo::NT; ++nt) s[mt][nt] = 0.0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int qoff = (i & 3) + 8 * (i >> 2);                    // + 4 h: the Q position inside its cell
                const double qnorm = qn[q0 + mt * CELL + qoff];             // the Q range ends inside the padded list
#pragma unroll
                for (int nt = 0; nt < LaneInfo::NT; ++nt) {
                    double d2 = (qnorm + pnorm[nt]) - 2.0 * (double)acc[mt][nt][i];
                    d2 = d2 < 0.0 ? 0.0 : d2;
                    double k = exp(-d2 * gamma);
                    // the diagonal cell of the diagonal tile: q == p dropped by POSITION (a select: NaN goes too)
                    if constexpr (SYM) k = (diag && qc0 + mt == pc0 + nt && qoff + 4 * L.h == L.r) ? 0.0 : k;
                    s[mt][nt] += k;
                }
                if ((i & 1) == 1) __builtin_amdgcn_sched_barrier(0);        // four exp chains at a time: more in flight spill
            }
        }
        // One xor tree (1, 2, 4, .. 32) for the four values: value j = 2 mt + nt ends in the lanes with (lane & 3) == j.
        // Step 1 serves two values per lane, step 2 one; each addition has the operands a tree of its own would have.
        const bool b0 = (L.lane & 1) != 0, b1 = (L.lane & 2) != 0;
        const double a0 = (b0 ? s[0][1] : s[0][0]) + __shfl_xor(b0 ? s[0][0] : s[0][1], 1);
        const double a1 = (b0 ? s[1][1] : s[1][0]) + __shfl_xor(b0 ? s[1][0] : s[1][1], 1);
        double v = (b1 ? a1 : a0) + __shfl_xor(b1 ? a0 : a1, 2);
#pragma unroll
        for (int off = 4; off <= 32; off <<= 1) v += __shfl_xor(v, off);
        if (L.lane < 4) {
            const int qc = qc0 + (L.lane >> 1), pc = pc0 + (L.lane & 1);
            if (qc < cq && pc < cp) {
                if constexpr (SYM) {
                    if (qc <= pc) {                                         // (off the diagonal tile: always)
                        out[(int64_t)qc * ldo + pc] = v;
                        out[(int64_t)pc * ldo + qc] = v;
                    }
                } else {
                    out[(int64_t)pc * ldo + qc] = v;
                }
            }
        }
    }
};

// one buffer descriptor spans a stored matrix; rows are reached through 32-bit byte offsets
__device__ __forceinline__ TileRsrc cells_matrix_rsrc(const float* X, int64_t N, int64_t ld) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(reinterpret_cast<uintptr_t>(X) & 0xffffffffu));
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(reinterpret_cast<uintptr_t>(X) >> 32));
    const unsigned bytes = __builtin_amdgcn_readfirstlane((unsigned)((uint64_t)N * (uint64_t)ld * 4u));
    TileRsrc r;
    r.rsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>((static_cast<uintptr_t>(hi) << 32) | lo), 0, (int)bytes,
                                               0x00020000);
    return r;
}

// grid: x = P tile (SYM: heaviest first), y = chunk of `chunk_tiles` Q tiles (SYM: chunks past the diagonal have nothing to do)
template <bool SYM, bool KTAIL>
__global__ void __launch_bounds__(ENGINE_THREADS, 2)
mmd_cells_kernel(const float* __restrict__ Q, int64_t nq_rows, int64_t ldq, const unsigned* __restrict__ qoff,
                 const double* __restrict__ qn, int64_t nq_pos, const float* __restrict__ P, int64_t np_rows, int64_t ldp,
                 const unsigned* __restrict__ poff, const double* __restrict__ pn, int64_t np_pos, int D, int chunk_tiles,
                 const float* __restrict__ bw2_dev, double gamma, double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LaneInfo L;
    const int64_t TQ = (nq_pos + TB - 1) / TB, TP = (np_pos + TB - 1) / TB;
    const int tp = SYM ? (int)(TP - 1) - (int)blockIdx.x : (int)blockIdx.x;
    const int64_t q0 = (int64_t)blockIdx.y * chunk_tiles;
    const int64_t qlast = SYM ? (int64_t)tp : TQ - 1;
    if (q0 > qlast) return;
    const int64_t left = qlast + 1 - q0;
    const int ntiles = left < chunk_tiles ? (int)left : chunk_tiles;

    const int srow = L.tid >> 3, scol = (L.tid & 7) * 4;
    const TileRsrc qr = cells_matrix_rsrc(Q, nq_rows, ldq), pr = cells_matrix_rsrc(P, np_rows, ldp);
    auto gathered = [&](const TileRsrc& rs, const unsigned* __restrict__ table, int64_t tile, bool live) {
        TileAddr a;
        a.rs = rs;
        unsigned ro[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) ro[q] = table[(live ? tile : 0) * TB + q * 32 + srow];     // four independent loads
#pragma unroll
        for (int q = 0; q < 4; ++q) a.vo[q] = (live && ro[q] != CELLS_HOLE) ? ro[q] + (unsigned)(scol * 4) : CELLS_HOLE;
        return a;
    };
    const TileAddr pa = gathered(pr, poff, tp, true);

    CellsEpilogue<SYM> epi(L);
    epi.qn = qn;
    epi.qtile0 = (int)q0;
    epi.ptile = tp;
    epi.cq = (int)((nq_pos + CELL - 1) / CELL);
    epi.cp = (int)((np_pos + CELL - 1) / CELL);
    epi.ldo = SYM ? epi.cp : epi.cq;
    epi.gamma = bw2_dev != nullptr ? 0.5 / (double)*bw2_dev : gamma;        // the median feeds the sums without a host round trip
    epi.out = out;
#pragma unroll
    for (int nt = 0; nt < LaneInfo::NT; ++nt) epi.pnorm[nt] = pn[(int64_t)tp * TB + L.wn * 64 + nt * 32 + L.r];   // < the padded length
    auto qaddr = [&](int t) { return gathered(qr, qoff, q0 + t, t < ntiles); };               // the pipeline prefetches past the last tile
    addr_pipeline_early<EV_DEFAULT, KTAIL>(qaddr, pa, ntiles, D, 0, lds, L, epi);
}

// out[u][v] = the cells [ua[u], ua[u + 1]) x [ub[v], ub[v + 1]) in row-major order; a null offset table: unit = cell
__global__ void __launch_bounds__(256) cells_units_kernel(const double* __restrict__ cells, int64_t ldc, const int64_t* __restrict__ ua,
                                                          int64_t U1, const int64_t* __restrict__ ub, int64_t U2,
                                                          double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= U1 * U2) return;
    const int64_t u = e / U2, v = e % U2;
    const int64_t a0 = ua ? ua[u] : u, a1 = ua ? ua[u + 1] : u + 1, b0 = ub ? ub[v] : v, b1 = ub ? ub[v + 1] : v + 1;
    double s = 0.0;
    for (int64_t a = a0; a < a1; ++a)
        for (int64_t b = b0; b < b1; ++b) s += cells[a * ldc + b];
    out[e] = s;
}

// ---------------------------------------------------------------- host side
struct CellsSet {                // one side of the call
    int64_t n_pos, n_pad, C;
    unsigned* rowoff;
    double* norm;
    int64_t* units;              // device copy of the U + 1 offsets (room for C + 1), or unused
};

struct CellsWs {
    unsigned long long* flag;
    CellsSet s[2];
    double* cells[3];            // the cell matrices of XX, YY, XY when units fold them
    size_t bytes;
    bool ok;
};

static CellsWs cells_carve(void* ws, size_t ws_bytes, int64_t n1_pos, int64_t n2_pos, unsigned blocks) {
    Carver c(ws, ws_bytes);
    CellsWs w{};
    w.flag = reinterpret_cast<unsigned long long*>(c.take<char>(8));
    const int64_t n[2] = {n1_pos, n2_pos};
    const unsigned uses[2] = {AM_MMD_XX | AM_MMD_XY, AM_MMD_YY | AM_MMD_XY};
    for (int k = 0; k < 2; ++k) {
        CellsSet& s = w.s[k];
        s.n_pos = n[k];
        s.C = ceil_div(n[k], CELL);
        s.n_pad = ceil_div(n[k], TB) * TB;
        if (!(blocks & uses[k])) continue;
        s.rowoff = c.take<unsigned>((size_t)s.n_pad);
        s.norm = c.take<double>((size_t)s.n_pad);
        s.units = c.take<int64_t>((size_t)s.C + 1);
    }
    const size_t c1 = (size_t)w.s[0].C, c2 = (size_t)w.s[1].C;
    if (blocks & AM_MMD_XX) w.cells[0] = c.take<double>(c1 * c1);
    if (blocks & AM_MMD_YY) w.cells[1] = c.take<double>(c2 * c2);
    if (blocks & AM_MMD_XY) w.cells[2] = c.take<double>(c1 * c2);
    w.bytes = c.off;
    w.ok = c.ok();
    return w;
}

static int check_cell_units(const int64_t* units, int U, int64_t C, const char* name) {
    if (units == nullptr) return AM_OK;
    AM_REQUIRE(U >= 1 && U <= C, AM_ERR_BAD_SHAPE, "%s names %d units of %lld cells (1 <= units <= cells)", name, U, (long long)C);
    AM_REQUIRE(units[0] == 0 && units[U] == C, AM_ERR_BAD_ARG, "%s must start at 0 and end at the number of cells, %lld (got %lld .. %lld)",
               name, (long long)C, (long long)units[0], (long long)units[U]);
    for (int u = 0; u < U; ++u)
        AM_REQUIRE(units[u + 1] > units[u], AM_ERR_BAD_SHAPE, "%s: unit %d holds %lld cells (offsets must increase strictly)", name, u,
                   (long long)(units[u + 1] - units[u]));
    return AM_OK;
}

static int check_cell_positions(const int64_t* idx, int64_t n_pos, int64_t N, const char* name) {
    AM_REQUIRE(n_pos >= 1 && n_pos < ((int64_t)1 << 30), AM_ERR_BAD_SHAPE, "%s names %lld positions (1 <= positions < 2^30)", name,
               (long long)n_pos);
    AM_REQUIRE(idx || n_pos == N, AM_ERR_BAD_SHAPE, "no index list: %s must equal the %lld stored rows (got %lld)", name, (long long)N,
               (long long)n_pos);
    return AM_OK;
}

template <bool SYM>
static int cells_sweep(const float* Q, int64_t nq_rows, int64_t ldq, const CellsSet& q, const float* P, int64_t np_rows, int64_t ldp,
                       const CellsSet& p, int D, const float* bw2_dev, double gamma, double* out, hipStream_t st) {
    const int64_t TQ = q.n_pad / TB, TP = p.n_pad / TB;
    const int chunk = kad_chunk(SYM ? TP * (TP + 1) / 2 : TP * TQ, TQ);
    const dim3 grid((unsigned)TP, (unsigned)ceil_div(TQ, chunk));
    auto launch = [&](auto kernel) -> int {
        AM_HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), (int)CELLS_LDS_BYTES));
        hipLaunchKernelGGL(kernel, grid, dim3(ENGINE_THREADS), CELLS_LDS_BYTES, st, Q, nq_rows, ldq, (const unsigned*)q.rowoff,
                           (const double*)q.norm, q.n_pos, P, np_rows, ldp, (const unsigned*)p.rowoff, (const double*)p.norm, p.n_pos,
                           D, chunk, bw2_dev, gamma, out);
        AM_LAUNCH_CHECK();
        return AM_OK;
    };
    return (D % BK) != 0 ? launch(&mmd_cells_kernel<SYM, true>) : launch(&mmd_cells_kernel<SYM, false>);
}

static int cells_fold(const double* cells, int64_t ldc, const int64_t* ua, int64_t U1, const int64_t* ub, int64_t U2, double* out,
                      hipStream_t st) {
    hipLaunchKernelGGL(cells_units_kernel, dim3((unsigned)ceil_div(U1 * U2, 256)), dim3(256), 0, st, cells, ldc, ua, U1, ub, U2, out);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

}  // namespace am

using namespace am;

extern "C" size_t am_mmd_rbf_cells_workspace_bytes(int64_t n1_pos, int64_t n2_pos, int D, unsigned blocks) {
    const int64_t lim = (int64_t)1 << 30;
    if (n1_pos < 1 || n2_pos < 1 || n1_pos >= lim || n2_pos >= lim || D < 1 || blocks == 0 || (blocks & ~7u) != 0) return 0;
    return cells_carve(nullptr, 0, n1_pos, n2_pos, blocks).bytes;
}

extern "C" int am_mmd_rbf_cells_f32(const float* X, int64_t N1, int64_t ldx, const int64_t* idx_x, int64_t n1_pos,
                                    const int64_t* units_x, int U1, const float* Y, int64_t N2, int64_t ldy, const int64_t* idx_y,
                                    int64_t n2_pos, const int64_t* units_y, int U2, int D, const float* bw2_dev, double gamma,
                                    unsigned blocks, double* out_xx, double* out_yy, double* out_xy, void* ws, size_t ws_bytes,
                                    am_stream_t stream) {
    int rc = check_two_sets_f32(X, N1, ldx, Y, N2, ldy, D, blocks);
    if (rc != AM_OK) return rc;
    AM_REQUIRE(out_xx || !(blocks & AM_MMD_XX), AM_ERR_BAD_ARG, "null pointer: out_xx is written by AM_MMD_XX");
    AM_REQUIRE(out_yy || !(blocks & AM_MMD_YY), AM_ERR_BAD_ARG, "null pointer: out_yy is written by AM_MMD_YY");
    AM_REQUIRE(out_xy || !(blocks & AM_MMD_XY), AM_ERR_BAD_ARG, "null pointer: out_xy is written by AM_MMD_XY");
    AM_REQUIRE(bw2_dev != nullptr || gamma >= 0.0, AM_ERR_BAD_ARG, "gamma must be >= 0 (or bw2_dev given)");
    AM_TRY(check_cell_positions(idx_x, n1_pos, N1, "n1_pos"));
    AM_TRY(check_cell_positions(idx_y, n2_pos, N2, "n2_pos"));
    AM_TRY(check_cell_units(units_x, U1, ceil_div(n1_pos, CELL), "units_x"));
    AM_TRY(check_cell_units(units_y, U2, ceil_div(n2_pos, CELL), "units_y"));
    const CellsWs w = cells_carve(ws, ws_bytes, n1_pos, n2_pos, blocks);
    AM_REQUIRE(w.ok, AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (am_mmd_rbf_cells_workspace_bytes), have %zu", w.bytes,
               ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const CellsSet &sx = w.s[0], &sy = w.s[1];
    const bool fold_x = units_x != nullptr && sx.rowoff != nullptr, fold_y = units_y != nullptr && sy.rowoff != nullptr;
    AM_HIP_TRY(hipMemsetAsync(w.flag, 0, sizeof(unsigned long long), st));
    if (fold_x) AM_HIP_TRY(hipMemcpyAsync(sx.units, units_x, ((size_t)U1 + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (fold_y) AM_HIP_TRY(hipMemcpyAsync(sy.units, units_y, ((size_t)U2 + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (sx.rowoff) {
        hipLaunchKernelGGL(cells_prep_kernel, dim3((unsigned)ceil_div(sx.n_pad, 4)), dim3(256), 0, st, X, N1, ldx, D, idx_x, sx.n_pos,
                           sx.n_pad, sx.rowoff, sx.norm, w.flag);
        AM_LAUNCH_CHECK();
    }
    if (sy.rowoff) {
        hipLaunchKernelGGL(cells_prep_kernel, dim3((unsigned)ceil_div(sy.n_pad, 4)), dim3(256), 0, st, Y, N2, ldy, D, idx_y, sy.n_pos,
                           sy.n_pad, sy.rowoff, sy.norm, w.flag);
        AM_LAUNCH_CHECK();
    }
    const int64_t* ux = fold_x ? sx.units : nullptr;
    const int64_t* uy = fold_y ? sy.units : nullptr;
    const int64_t nu1 = fold_x ? U1 : sx.C, nu2 = fold_y ? U2 : sy.C;
    if (blocks & AM_MMD_XX) {
        AM_TRY(cells_sweep<true>(X, N1, ldx, sx, X, N1, ldx, sx, D, bw2_dev, gamma, fold_x ? w.cells[0] : out_xx, st));
        if (fold_x) AM_TRY(cells_fold(w.cells[0], sx.C, ux, nu1, ux, nu1, out_xx, st));
    }
    if (blocks & AM_MMD_YY) {
        AM_TRY(cells_sweep<true>(Y, N2, ldy, sy, Y, N2, ldy, sy, D, bw2_dev, gamma, fold_y ? w.cells[1] : out_yy, st));
        if (fold_y) AM_TRY(cells_fold(w.cells[1], sy.C, uy, nu2, uy, nu2, out_yy, st));
    }
    if (blocks & AM_MMD_XY) {
        const bool fold = fold_x || fold_y;
        AM_TRY(cells_sweep<false>(Y, N2, ldy, sy, X, N1, ldx, sx, D, bw2_dev, gamma, fold ? w.cells[2] : out_xy, st));
        if (fold) AM_TRY(cells_fold(w.cells[2], sy.C, ux, nu1, uy, nu2, out_xy, st));
    }
    return AM_OK;
}
