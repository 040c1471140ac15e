// Row sums of the PRODUCT of two Gram matrices of paired sets (am_pair_dependence_f32): what distance covariance /
// correlation and HSIC / CKA are built from, without an N x N matrix.  Row i of X belongs to row i of Y (or, with `perm`,
// to row perm[i] of Y).  For every ordered pair i != j
//   a_ij = k(x_i, x_j)     b_ij = l(y_i, y_j)
//   A_i = sum_j a_ij   B_i = sum_j b_ij   H_i = sum_j a_ij b_ij   AA_i = sum_j a_ij^2   BB_i = sum_j b_ij^2
// with k, l of one kind, one bandwidth per side:
//   AM_MMD_ENERGY     +sqrt(d2)              (the distance itself: distance covariance)
//   AM_MMD_GAUSSIAN   exp(-d2 g),        g = 0.5 / bw2
//   AM_MMD_LAPLACIAN  exp(-sqrt(d2) h),  h = 1 / sqrt(bw2)
// Arithmetic of one value: that of MultiEpilogue::finish in mmd_multi.hip at scale 1 - d2 = max((|p|^2 + |q|^2) - 2 dot, 0)
// in f64, f64 squared norms, f32 matrix-core dot product; the product and all sums are f64.  i == j is dropped by INDEX, so
// duplicated rows stay each other's pairs.
//
// Two Grams on one tile.  A workgroup owns one 128-row P block and a chunk of consecutive Q tiles, and sweeps the FULL
// square (every ordered pair; the triangular sweep with the two-axis butterfly of mmd_rows.hip would halve the work and is
// not done here).  Its stage sequence alternates per Q tile: the Dx slabs of the X Gram, then the Dy slabs of the Y Gram of
// the same tile, each into an accumulator tile of its own (2 x 64 VGPRs): the X dot products stay parked, raw f32, while
// the Y slabs run, and only then are a and b evaluated and multiplied.  The stage loop is tile_pipeline's (tile_engine.h: two
// LDS stages, the loads of stage g + 1 issued before the MFMAs of stage g, one barrier per stage, running on across tiles
// and sides) with a slab count that depends on the side, each side with its own `% 32` tail, and with the LDS writes of the
// next slab placed BEFORE the epilogue so that the staging registers are dead while the exp / sqrt chains run.  Operands are
// fetched through one buffer descriptor per matrix and 32-bit byte offsets per row; the Y rows of both operands go through
// an offset table built from `perm` (identity without one) - no gathered copy is made.
//
// The P rows are the lane-local axis (RowEpilogue of kad_groups.hip): a lane keeps five f64 running sums per P row it holds;
// at the end they are combined in a fixed order (the two halves of a wave, then the two wm waves through LDS) and written to
// partial[chunk][sum][row].  pdep_rows_kernel adds a row's chunks in chunk order, pdep_sums_kernel the rows by strided
// per-thread sums and a tree.  No floating-point atomics; two calls give the same bits; at most PDEP_MAX_CHUNKS chunks.
//
// Non-finite rows: a row whose squared norm is not finite (either side) gets a NaN norm, so every value it takes part in is
// NaN whatever the kind; it is counted in out_sums[7].  An entry of perm outside [0, N) counts as such a row (it is never
// dereferenced).
//
// Registers: 252 (Gaussian), 256 (Laplacian), 252 (distance) VGPRs of the 256 that two waves per SIMD leave, no AGPRs, no
// scratch memory: two workgroups of four waves per CU (73 728 B of LDS each) - tests/test_dependence_cpu.py pins it.  Measured
// on the MI355X at 100 000 rows (tools/dependence_probe.py): 1.00 x (512 / 512) and 0.98 x (512 / 128) the sum of two
// am_mmd_multi_f32 energy XY passes over the same rows.
#include "am_common.h"
#include "kad_common.h"
#include "pairwise_common.h"
#include <algorithm>

namespace am {

constexpr unsigned PDEP_HOLE = 0xffffffffu;          // voffset past every descriptor: the load returns 0
constexpr int64_t PDEP_MAX_CHUNKS = 16;              // most Q chunks of a P block (the partials are per row and sum)
constexpr int PDEP_SUMS = 5;                         // A, B, H, AA, BB
constexpr size_t PDEP_LDS_BYTES = ENGINE_LDS_FLOATS * sizeof(float);      // 73 728 B: two workgroups per CU

// one wave per position p < n_pad: norm[p] = |row|^2 in f64 (the loop of kad_norms_kernel; NaN where it is not finite or
// perm[p] is outside [0, N); 0 for the padding p >= N) and, where `off` is given, the byte offset of the stored row
__global__ void __launch_bounds__(256) pdep_prep_kernel(const float* __restrict__ M, int64_t ld, int D, int64_t N, int64_t n_pad,
                                                        const int64_t* __restrict__ perm, unsigned* __restrict__ off,
                                                        double* __restrict__ norm) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= n_pad) return;
    if (p >= N) {
        if (lane == 0) {
            if (off != nullptr) off[p] = PDEP_HOLE;
            norm[p] = 0.0;
        }
        return;
    }
    const int64_t row = perm != nullptr ? perm[p] : p;
    const bool ok = (unsigned long long)row < (unsigned long long)N;
    double acc = 0.0;
    if (ok) {
        const float* x = M + row * ld;
        for (int k = lane * 4; k < D; k += 256) {
            const f32x4 v = load_k4(x, k, D);
            acc += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) {
        if (off != nullptr) off[p] = ok ? (unsigned)(row * ld * 4) : PDEP_HOLE;      // N * ld * 4 < 4 GiB
        norm[p] = (ok && acc < (double)INFINITY) ? acc : (double)NAN;                // (NaN < inf is false)
    }
}

template <int KIND>
__device__ __forceinline__ double pdep_value(double qnorm, double pnorm, float dot, double par) {
    double d2 = (qnorm + pnorm) - 2.0 * (double)dot;
    d2 = d2 < 0.0 ? 0.0 : d2;
    if constexpr (KIND == AM_MMD_GAUSSIAN) return exp(-d2 * par);
    else if constexpr (KIND == AM_MMD_LAPLACIAN) return exp(-sqrt(d2) * par);
    else return sqrt(d2);
}

// grid: x = P block (128 rows), y = chunk of `chunk_tiles` Q tiles.  partial[(y * 5 + sum) * n_pad + row].
template <int KIND>
__global__ void __launch_bounds__(ENGINE_THREADS, 2)
pdep_kernel(const float* __restrict__ X, int64_t ldx, int Dx, const float* __restrict__ Y, int64_t ldy, int Dy, int64_t N,
            int64_t n_pad, const unsigned* __restrict__ yoff, const double* __restrict__ xn, const double* __restrict__ yn,
            int chunk_tiles, const float* __restrict__ bw2x_dev, double bw2x, const float* __restrict__ bw2y_dev, double bw2y,
            double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LaneInfo L;
    const int tp = (int)blockIdx.x;
    const int TQ = (int)(n_pad / TB);
    const int q0 = (int)blockIdx.y * chunk_tiles;        // < TQ: the grid has ceil(TQ / chunk_tiles) chunks
    const int ntiles = TQ - q0 < chunk_tiles ? TQ - q0 : chunk_tiles;
    const int srow = L.tid >> 3, scol = (L.tid & 7) * 4;
    const int n = (int)N;                                // rows are indexed in 32 bits: N * ld * 4 < 4 GiB and ld >= 4 put N below 2^28
    const int nkx = (Dx + BK - 1) / BK, nky = (Dy + BK - 1) / BK;
    const int G = ntiles * (nkx + nky);

    // one buffer descriptor spans a stored matrix; rows are reached through 32-bit byte offsets
    auto whole = [&](const float* base, int64_t ld) {
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(reinterpret_cast<uintptr_t>(base) & 0xffffffffu));
        const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(reinterpret_cast<uintptr_t>(base) >> 32));
        const unsigned bytes = __builtin_amdgcn_readfirstlane((unsigned)((uint64_t)N * (uint64_t)ld * 4u));
        TileRsrc r;
        r.rsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>((static_cast<uintptr_t>(hi) << 32) | lo), 0, (int)bytes,
                                                    0x00020000);
        return r;
    };
    const TileRsrc xrs = whole(X, ldx), yrs = whole(Y, ldy);
    // the four staging rows of this thread in 128-row tile `tile` (< TQ) of side 0 (X) / 1 (Y): byte offset of its float4
    auto offsets = [&](int tile, int side, unsigned (&o)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t row = (int64_t)tile * TB + j * 32 + srow;         // < n_pad
            if (side == 0) {
                o[j] = row < N ? (unsigned)(row * ldx * 4) + (unsigned)(scol * 4) : PDEP_HOLE;
            } else {
                const unsigned v = yoff[row];
                o[j] = v != PDEP_HOLE ? v + (unsigned)(scol * 4) : PDEP_HOLE;
            }
        }
    };
    unsigned pxo[4], pyo[4], qo[4];
    offsets(tp, 0, pxo);
    offsets(tp, 1, pyo);
    offsets(q0, 0, qo);

    double par[2] = {0.0, 0.0};
    if constexpr (KIND != AM_MMD_ENERGY) {
        if (bw2x_dev != nullptr) bw2x = (double)*bw2x_dev;                  // the medians feed the sums without a host round trip
        if (bw2y_dev != nullptr) bw2y = (double)*bw2y_dev;
        // wave-uniform: kept in scalar registers
        auto uniform = [](double v) {
            const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
            return __hiloint2double(hi, lo);
        };
        par[0] = uniform(KIND == AM_MMD_GAUSSIAN ? 0.5 / bw2x : 1.0 / sqrt(bw2x));
        par[1] = uniform(KIND == AM_MMD_GAUSSIAN ? 0.5 / bw2y : 1.0 / sqrt(bw2y));
    }
    double sum[PDEP_SUMS][LaneInfo::NT], pnx[LaneInfo::NT], pny[LaneInfo::NT];
    int prow[LaneInfo::NT];
    bool pok[LaneInfo::NT];                              // false for a padded P row
#pragma unroll
    for (int nt = 0; nt < LaneInfo::NT; ++nt) {
        const int p = tp * TB + L.wn * 64 + nt * 32 + L.r;                  // < n_pad
        pok[nt] = p < n;
        prow[nt] = p;
        pnx[nt] = xn[p];
        pny[nt] = yn[p];
#pragma unroll
        for (int v = 0; v < PDEP_SUMS; ++v) sum[v][nt] = 0.0;
    }

    // ---- the stage sequence: per Q tile nkx slabs of the X Gram, then nky slabs of the Y Gram
    int ft = 0, fs = 0, fkt = 0;                         // (tile, side, slab) of the next fetch: one stage ahead of the MFMAs
    int mk = 0, mD = 0;                                  // first inner index and width of the slab held in rq / rp
    f32x4 rq[4], rp[4];
    auto issue = [&]() {
        const TileRsrc& rs = fs == 0 ? xrs : yrs;
        const unsigned so = (unsigned)(fkt * BK * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned po = fs == 0 ? pxo[j] : pyo[j];
            // the slab offset goes into the range-checked vector offset: a load past the matrix returns 0
            rq[j] = rsrc_load(rs, qo[j] != PDEP_HOLE ? qo[j] + so : PDEP_HOLE, 0);
            rp[j] = rsrc_load(rs, po != PDEP_HOLE ? po + so : PDEP_HOLE, 0);
        }
        mk = fkt * BK;
        mD = fs == 0 ? Dx : Dy;
        if (++fkt == (fs == 0 ? nkx : nky)) {            // wave-uniform
            fkt = 0;
            ft += fs;
            fs ^= 1;
            if (ft < ntiles) offsets(q0 + ft, fs, qo);
        }
    };
    auto commit = [&](int g) {
        if (mk + BK > mD) {                              // wave-uniform: zero the inner-dimension tail of a side's last slab
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool in = mk + scol + e < mD;
                    rq[j][e] = in ? rq[j][e] : 0.f;
                    rp[j][e] = in ? rp[j][e] : 0.f;
                }
        }
        float* s = lds + (g & 1) * STAGE_FLOATS + srow * LDK + scol;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            *reinterpret_cast<f32x4*>(s + j * 32 * LDK) = rq[j];
            *reinterpret_cast<f32x4*>(s + TILE_FLOATS + j * 32 * LDK) = rp[j];
        }
    };
    int g = 0;
    auto stage = [&](f32x16 (&acc)[2][2]) {
        const bool more = g + 1 < G;
        if (more) issue();
        const float* s = lds + (g & 1) * STAGE_FLOATS;
        compute_stage_v<EV_FRAGDB>(s, s + TILE_FLOATS, L, acc);
        if (more) commit(g + 1);                         // before the epilogue: rq / rp are dead while it runs
        __syncthreads();
        ++g;
    };

    f32x16 ax[2][2], ay[2][2];
    zero_acc(ax);
    zero_acc(ay);
    issue();
    commit(0);
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
        for (int kt = 0; kt < nkx; ++kt) stage(ax);      // the X dot products stay parked in ax, raw f32 ...
        for (int kt = 0; kt < nky; ++kt) stage(ay);      // ... while the Y Gram of the same tile is formed
        int et = L.tid;
        asm volatile("" : "+v"(et));                     // derived afresh per tile: nothing but the thread index lives across the stages
        const int qb = (q0 + t) * TB + (et >> 7) * 64 + 4 * ((et >> 5) & 1);            // wm, h of LaneInfo
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int q = qb + mt * 32 + (i & 3) + 8 * (i >> 2);       // < n_pad
                const bool qok = q < n;
                const double qnx = xn[q], qny = yn[q];
#pragma unroll
                for (int nt = 0; nt < LaneInfo::NT; ++nt) {
                    const bool keep = qok & pok[nt] & (q != prow[nt]);   // by INDEX; a select: padding never adds, NaN of a valid pair does
                    double a = pdep_value<KIND>(qnx, pnx[nt], ax[mt][nt][i], par[0]);
                    double b = pdep_value<KIND>(qny, pny[nt], ay[mt][nt][i], par[1]);
                    a = keep ? a : 0.0;
                    b = keep ? b : 0.0;
                    sum[0][nt] += a;
                    sum[1][nt] += b;
                    sum[2][nt] += a * b;
                    sum[3][nt] += a * a;
                    sum[4][nt] += b * b;
                    if constexpr (KIND == AM_MMD_LAPLACIAN) __builtin_amdgcn_sched_barrier(0);   // sqrt and exp: two chains at a time
                }
                __builtin_amdgcn_sched_barrier(0);       // four exp / sqrt chains at a time: more in flight spill
            }
        zero_acc(ax);
        zero_acc(ay);
    }

    // the two halves of a wave hold the same P rows against different Q rows (lane ^ 32); then the two wm waves, through
    // LDS (the staging slabs are idle after the pipeline's last barrier)
    double* red = reinterpret_cast<double*>(lds);        // [5][2][128]
    int tid = L.tid;
    asm volatile("" : "+v"(tid));                        // the fold's indices are derived afresh: none of them lives across the tile loop
    const int e_h = (tid >> 5) & 1, e_wm = tid >> 7, e_row = ((tid >> 6) & 1) * 64 + (tid & 31);
#pragma unroll
    for (int v = 0; v < PDEP_SUMS; ++v)
#pragma unroll
        for (int nt = 0; nt < LaneInfo::NT; ++nt) {
            const double w = sum[v][nt] + __shfl_xor(sum[v][nt], 32);
            if (e_h == 0) red[(v * 2 + e_wm) * TB + e_row + nt * 32] = w;
        }
    __syncthreads();
    double* out = partial + (int64_t)blockIdx.y * PDEP_SUMS * n_pad + (int64_t)blockIdx.x * TB;
    for (int e = tid; e < PDEP_SUMS * TB; e += ENGINE_THREADS) {
        const int v = e / TB, row = e % TB;
        out[(int64_t)v * n_pad + row] = red[(v * 2) * TB + row] + red[(v * 2 + 1) * TB + row];
    }
}

// out_rows[p] = {A, B, H, AA, BB}: a row's chunks in chunk order
__global__ void __launch_bounds__(256) pdep_rows_kernel(const double* __restrict__ partial, int nch, int64_t n_pad, int64_t N,
                                                        double* __restrict__ out_rows) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
#pragma unroll
    for (int v = 0; v < PDEP_SUMS; ++v) {
        double s = 0.0;
        for (int c = 0; c < nch; ++c) s += partial[((int64_t)c * PDEP_SUMS + v) * n_pad + p];
        out_rows[p * PDEP_SUMS + v] = s;
    }
}

// out_sums[j], one workgroup each: j < 5 the column sums of out_rows, 5 sum A_i B_i, 6 / 7 the finite / non-finite rows (by
// the norms of the prep kernel) - strided per-thread sums, then a tree
__global__ void __launch_bounds__(256) pdep_sums_kernel(const double* __restrict__ rows, const double* __restrict__ xn,
                                                        const double* __restrict__ yn, int64_t N, double* __restrict__ out_sums) {
    __shared__ double red[256];
    const int tid = threadIdx.x, j = blockIdx.x;
    double s = 0.0;
    for (int64_t p = tid; p < N; p += 256) {
        if (j < PDEP_SUMS) {
            s += rows[p * PDEP_SUMS + j];
        } else if (j == 5) {
            s += rows[p * PDEP_SUMS] * rows[p * PDEP_SUMS + 1];
        } else {
            const bool finite = xn[p] == xn[p] && yn[p] == yn[p];          // a non-finite row carries a NaN norm
            s += (finite == (j == 6)) ? 1.0 : 0.0;
        }
    }
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) out_sums[j] = red[0];
}

// ---------------------------------------------------------------- host side
struct PdepPlan {
    int64_t T, n_pad;            // 128-row tiles of either axis
    int chunk, nch;
};

static PdepPlan pdep_plan(int64_t N) {
    PdepPlan p;
    p.T = ceil_div(N, TB);
    p.n_pad = p.T * TB;
    // per-ROW partials of five sums: the number of chunks is capped where kad.hip's is not
    p.chunk = (int)std::max<int64_t>(kad_chunk(p.T * p.T, p.T), ceil_div(p.T, PDEP_MAX_CHUNKS));
    p.nch = (int)ceil_div(p.T, p.chunk);
    return p;
}

struct PdepWs {
    double *xn, *yn, *partial;
    unsigned* yoff;
    size_t bytes;
    bool ok;
};

static PdepWs pdep_carve(void* ws, size_t ws_bytes, const PdepPlan& p) {
    Carver c(ws, ws_bytes);
    PdepWs w{};
    w.xn = c.take<double>((size_t)p.n_pad);
    w.yn = c.take<double>((size_t)p.n_pad);
    w.yoff = c.take<unsigned>((size_t)p.n_pad);
    w.partial = c.take<double>((size_t)p.nch * PDEP_SUMS * (size_t)p.n_pad);
    w.bytes = c.off;
    w.ok = c.ok();
    return w;
}

static bool pdep_bw_ok(double v) { return v > 0.0 && v < (double)INFINITY; }

}  // namespace am

using namespace am;

extern "C" size_t am_pair_dependence_workspace_bytes(int64_t N, int Dx, int Dy) {
    if (N < 4 || Dx < 1 || Dy < 1 || N >= ((int64_t)1 << 28)) return 0;
    return pdep_carve(nullptr, 0, pdep_plan(N)).bytes;
}

extern "C" int am_pair_dependence_f32(const float* X, int64_t N, int64_t ldx, int Dx, const float* Y, int64_t ldy, int Dy,
                                      const int64_t* perm, int kernel, const float* bw2x_dev, double bw2x, const float* bw2y_dev,
                                      double bw2y, double* out_rows, double* out_sums, void* ws, size_t ws_bytes, am_stream_t stream) {
    AM_REQUIRE(X && Y && out_rows && out_sums, AM_ERR_BAD_ARG, "null pointer (X, Y, out_rows, out_sums)");
    AM_REQUIRE(kernel == AM_MMD_GAUSSIAN || kernel == AM_MMD_LAPLACIAN || kernel == AM_MMD_ENERGY, AM_ERR_BAD_ARG,
               "kernel = %d is not one of AM_MMD_GAUSSIAN, AM_MMD_LAPLACIAN, AM_MMD_ENERGY", kernel);
    AM_REQUIRE(N >= 4 && Dx >= 1 && Dy >= 1, AM_ERR_BAD_SHAPE, "N=%lld Dx=%d Dy=%d: the unbiased statistics need N >= 4 paired rows",
               (long long)N, Dx, Dy);
    AM_REQUIRE(aligned16(X) && aligned16(Y) && ldx % 4 == 0 && ldy % 4 == 0 && ldx >= Dx && ldy >= Dy, AM_ERR_BAD_ARG,
               "X/Y must be 16-byte aligned with ld %% 4 == 0 and ld >= D (ldx=%lld, Dx=%d, ldy=%lld, Dy=%d)", (long long)ldx, Dx,
               (long long)ldy, Dy);
    AM_REQUIRE(!kad_too_large(N, ldx) && !kad_too_large(N, ldy), AM_ERR_BAD_SHAPE,
               "N * ld * 4 bytes of a set >= 4 GiB: one buffer descriptor spans a matrix");
    if (kernel != AM_MMD_ENERGY) {
        AM_REQUIRE(bw2x_dev != nullptr || pdep_bw_ok(bw2x), AM_ERR_BAD_ARG, "bw2x = %g must be finite and positive (or bw2x_dev given)", bw2x);
        AM_REQUIRE(bw2y_dev != nullptr || pdep_bw_ok(bw2y), AM_ERR_BAD_ARG, "bw2y = %g must be finite and positive (or bw2y_dev given)", bw2y);
    }
    const PdepPlan plan = pdep_plan(N);
    const PdepWs w = pdep_carve(ws, ws_bytes, plan);
    AM_REQUIRE(w.ok, AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (am_pair_dependence_workspace_bytes), have %zu", w.bytes,
               ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 prep((unsigned)ceil_div(plan.n_pad, 4));
    hipLaunchKernelGGL(pdep_prep_kernel, prep, dim3(256), 0, st, X, ldx, Dx, N, plan.n_pad, (const int64_t*)nullptr, (unsigned*)nullptr,
                       w.xn);
    AM_LAUNCH_CHECK();
    hipLaunchKernelGGL(pdep_prep_kernel, prep, dim3(256), 0, st, Y, ldy, Dy, N, plan.n_pad, perm, w.yoff, w.yn);
    AM_LAUNCH_CHECK();
    auto launch = [&](auto kern) -> int {
        AM_HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(kern), (int)PDEP_LDS_BYTES));
        hipLaunchKernelGGL(kern, dim3((unsigned)plan.T, (unsigned)plan.nch), dim3(ENGINE_THREADS), PDEP_LDS_BYTES, st, X, ldx, Dx, Y, ldy,
                           Dy, N, plan.n_pad, (const unsigned*)w.yoff, (const double*)w.xn, (const double*)w.yn, plan.chunk, bw2x_dev,
                           bw2x, bw2y_dev, bw2y, w.partial);
        AM_LAUNCH_CHECK();
        return AM_OK;
    };
    const int rc = kernel == AM_MMD_GAUSSIAN    ? launch(&pdep_kernel<AM_MMD_GAUSSIAN>)
                   : kernel == AM_MMD_LAPLACIAN ? launch(&pdep_kernel<AM_MMD_LAPLACIAN>)
                                                : launch(&pdep_kernel<AM_MMD_ENERGY>);
    if (rc != AM_OK) return rc;
    hipLaunchKernelGGL(pdep_rows_kernel, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, st, (const double*)w.partial, plan.nch,
                       plan.n_pad, N, out_rows);
    AM_LAUNCH_CHECK();
    hipLaunchKernelGGL(pdep_sums_kernel, dim3(8), dim3(256), 0, st, (const double*)out_rows, (const double*)w.xn, (const double*)w.yn, N,
                       out_sums);
    AM_LAUNCH_CHECK();
    return AM_OK;
}
