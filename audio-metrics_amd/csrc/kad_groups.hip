// Per-group Kernel Audio Distance (am_mmd_rbf_groups_f32): the Gaussian kernel sums of B groups of candidate rows, each
// against the one reference set, from ROW sums of the kernel matrix instead of one scalar per workgroup.
//
//   c_i = sum_j k(x_i, y_j)                              (cross pass)          Sxy_b = sum_{i in b} c_i
//   w_i = sum_{j in group(i), j != i} k(x_i, x_j)        (within pass)         Sxx_b = sum_{i in b} w_i
//
// Arithmetic of one pair: that of MmdEpilogue::finish in kad.hip - d2 = max((|a|^2 + |b|^2) - 2 dot, 0) in f64, f64 norms,
// f32 matrix-core dot product, k = exp(-d2 gamma) in f64.
//
// Everything is indexed by LIST POSITION p < n_total (the position in idx, group-sorted by construction of the offsets):
//   kadg_prep_kernel    per position: the byte offset of its stored row (HOLE for an index outside [0, N1): never
//                       dereferenced, its position goes to the flag word, the row counts as zeros), its f64 squared norm
//                       (the loop of kad_norms_kernel) and its group; the tail up to the next multiple of 128 is padding
//                       (HOLE, norm +inf -> k = 0, group -1)
//   kadg_rows_kernel    128 x 128 tiles on the f32 tile engine.  The P rows (lane axis) are 128 consecutive positions,
//                       gathered through the offsets - no gathered copy exists; the Q rows (register axis) are the dense
//                       reference rows (cross) or, gathered the same way, the positions of the tile's own groups (within:
//                       from the tile of the first position of its first group to the tile of the last position of its
//                       last group, masked by gid[q] == gid[p] && q != p).  A workgroup owns one P tile and a chunk of
//                       consecutive Q tiles; a lane keeps one f64 running sum per P row it holds (LaneInfo::NT), and at the
//                       end the sums are combined in a fixed order (fold_p_rows: the two halves of a wave, lane ^ 32, then
//                       the two wm waves through LDS) and written to partial[chunk][position].  No atomics.
//   kadg_rowsum_kernel  per position: its chunks added in chunk order -> rows[p] = {w_p, c_p}
//   kadg_finish_kernel  one workgroup per group: strided per-thread sums, then a tree -> out_groups[b] = {Sxx_b, Sxy_b}
//                       (both serve am_mmd_rbf_groups_f64 too, through their launchers in kad_common.h)
// The result depends on the list order and on nothing about where the rows are stored; two calls give the same bits.
#include "am_common.h"
#include "groups_common.h"
#include "kad_common.h"
#include "pairwise_common.h"
#include <algorithm>

namespace am {

constexpr unsigned KADG_HOLE = 0xffffffffu;          // voffset past every descriptor: the load returns 0
constexpr size_t KADG_LDS_BYTES = ENGINE_LDS_FLOATS * sizeof(float);      // 73 728 B: two workgroups per CU

// one wave per list position (padding included)
__global__ void __launch_bounds__(256) kadg_prep_kernel(const float* __restrict__ X, int64_t N1, int64_t ld, int D,
                                                        const int64_t* __restrict__ idx, const int64_t* __restrict__ offs, int B,
                                                        int64_t n_total, int64_t n_pad, unsigned* __restrict__ rowoff,
                                                        double* __restrict__ norm, int* __restrict__ gid,
                                                        unsigned long long* __restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= n_pad) return;
    if (p >= n_total) {
        if (lane == 0) {
            rowoff[p] = KADG_HOLE;
            norm[p] = INFINITY;
            gid[p] = -1;
        }
        return;
    }
    const int64_t row = idx ? idx[p] : p;
    const bool ok = (unsigned long long)row < (unsigned long long)N1;
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
        if (!ok) atomicMax(flag, (unsigned long long)p + 1ull);
        rowoff[p] = ok ? (unsigned)(row * ld * 4) : KADG_HOLE;      // N1 * ld * 4 < 4 GiB
        norm[p] = acc;
        gid[p] = group_of(offs, B, p);
    }
}

template <bool WITHIN>
struct RowEpilogue {
    const double* qn;            // f64 squared norms of the Q rows: reference rows (cross), padded positions (within)
    const int* gid;              // within: group of every padded position
    int nq, qtile0, ptile;
    double gamma;
    double sum[LaneInfo::NT];    // the running row sums of this lane's P rows
    double pnorm[LaneInfo::NT];  // +inf for padded positions: exp(-inf) = 0
    int pg[LaneInfo::NT];        // within: group of the P rows (-2 for padding: equal to no Q row's)
    const LaneInfo& L;
    __device__ __forceinline__ RowEpilogue(const LaneInfo& l) : L(l) {}
    __device__ __forceinline__ void aux_issue(int, int64_t) {}
    __device__ __forceinline__ void aux_commit(int) {}
    // (rows and positions are indexed in 32 bits: N * ld * 4 < 4 GiB and ld >= 4 put N below 2^28, n_total is checked)
    __device__ __forceinline__ void finish(int t, int64_t, f32x16 (&acc)[2][2]) {
        const int q0 = (qtile0 + t) * TB + L.wm * 64 + 4 * L.h, p0 = ptile * TB + L.wn * 64 + L.r;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int q = q0 + mt * 32 + (i & 3) + 8 * (i >> 2);
                double qnorm;
                int qg = 0;
                if constexpr (WITHIN) {
                    qnorm = qn[q];                                      // the Q range ends inside the padded list
                    qg = gid[q];
                } else {
                    qnorm = q < nq ? qn[q] : INFINITY;
                }
#pragma unroll
                for (int nt = 0; nt < LaneInfo::NT; ++nt) {
                    double d2 = (qnorm + pnorm[nt]) - 2.0 * (double)acc[mt][nt][i];
                    d2 = d2 < 0.0 ? 0.0 : d2;
                    const double k = exp(-d2 * gamma);
                    if constexpr (WITHIN) sum[nt] += (qg == pg[nt] && q != p0 + nt * 32) ? k : 0.0;   // a select: a NaN of another group is dropped
                    else sum[nt] += k;
                }
                if ((i & 1) == 1) __builtin_amdgcn_sched_barrier(0);    // four exp chains at a time: more in flight spill
            }
    }
};

// grid: x = P tile (128 list positions), y = chunk of `chunk_tiles` Q tiles.  partial[y * n_pad + position].
template <bool WITHIN, bool KTAIL>
__global__ void __launch_bounds__(ENGINE_THREADS, 2)
kadg_rows_kernel(const float* __restrict__ X, int64_t N1, int64_t ldx, const unsigned* __restrict__ rowoff,
                 const double* __restrict__ xn, const int* __restrict__ gid, const int64_t* __restrict__ offs, int64_t n_total,
                 int64_t n_pad, const float* __restrict__ Y, int64_t N2, int64_t ldy, const double* __restrict__ yn, int D,
                 int chunk_tiles, const float* __restrict__ bw2_dev, double gamma, double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LaneInfo L;
    const int tp = (int)blockIdx.x;
    double* out = partial + (int64_t)blockIdx.y * n_pad + (int64_t)tp * TB;
    int64_t qlo = 0, qhi = (N2 + TB - 1) / TB - 1;                          // cross: every reference tile
    if constexpr (WITHIN) {
        const int64_t pfirst = (int64_t)tp * TB, plast = (pfirst + TB < n_total ? pfirst + TB : n_total) - 1;
        qlo = offs[gid[pfirst]] / TB;
        qhi = (offs[gid[plast] + 1] - 1) / TB;
    }
    const int64_t q0 = qlo + (int64_t)blockIdx.y * chunk_tiles;
    if (q0 > qhi) {                                                         // within: this P tile's range has fewer chunks
        if (L.tid < TB) out[L.tid] = 0.0;
        return;
    }
    const int64_t left = qhi + 1 - q0;
    const int ntiles = left < chunk_tiles ? (int)left : chunk_tiles;

    const int srow = L.tid >> 3, scol = (L.tid & 7) * 4;
    // one buffer descriptor spans the stored matrix; rows are reached through 32-bit byte offsets
    TileRsrc xr;
    {
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(reinterpret_cast<uintptr_t>(X) & 0xffffffffu));
        const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(reinterpret_cast<uintptr_t>(X) >> 32));
        const unsigned bytes = __builtin_amdgcn_readfirstlane((unsigned)((uint64_t)N1 * (uint64_t)ldx * 4u));
        xr.rsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>((static_cast<uintptr_t>(hi) << 32) | lo), 0, (int)bytes,
                                                    0x00020000);
    }
    auto gathered = [&](int64_t tile, bool live) {
        TileAddr a;
        a.rs = xr;
        unsigned ro[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) ro[q] = rowoff[(live ? tile : 0) * TB + q * 32 + srow];     // four independent loads
#pragma unroll
        for (int q = 0; q < 4; ++q) a.vo[q] = (live && ro[q] != KADG_HOLE) ? ro[q] + (unsigned)(scol * 4) : KADG_HOLE;
        return a;
    };
    const TileAddr pa = gathered(tp, true);

    RowEpilogue<WITHIN> epi(L);
    epi.qn = WITHIN ? xn : yn;
    epi.gid = gid;
    epi.nq = (int)N2;
    epi.qtile0 = (int)q0;
    epi.ptile = tp;
    epi.gamma = bw2_dev != nullptr ? 0.5 / (double)*bw2_dev : gamma;        // the median feeds the sums without a host round trip
#pragma unroll
    for (int nt = 0; nt < LaneInfo::NT; ++nt) {
        const int p = tp * TB + L.wn * 64 + nt * 32 + L.r;                  // < n_pad
        epi.sum[nt] = 0.0;
        epi.pnorm[nt] = xn[p];
        epi.pg[nt] = p < n_total ? gid[p] : -2;
    }
    if constexpr (WITHIN) {
        auto qaddr = [&](int t) { return gathered(q0 + t, t < ntiles); };  // the pipeline prefetches past the last tile
        addr_pipeline_early<EV_DEFAULT, KTAIL>(qaddr, pa, ntiles, D, 0, lds, L, epi);
    } else {
        unsigned voq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) voq[q] = (unsigned)(((int64_t)(q * 32 + srow) * ldy + scol) * 4);
        auto qaddr = [&](int t) {                                           // past the last tile: zero valid rows
            TileAddr a;
            a.rs = make_tile_rsrc(Y, ldy, N2, t < ntiles ? (q0 + t) * TB : N2);
#pragma unroll
            for (int q = 0; q < 4; ++q) a.vo[q] = voq[q];
            return a;
        };
        addr_pipeline_early<EV_DEFAULT, KTAIL>(qaddr, pa, ntiles, D, 0, lds, L, epi);
    }
    fold_p_rows(epi.sum, reinterpret_cast<double*>(lds), L, out);          // staging slabs are idle after the pipeline's last barrier
}

// rows[p] = {w_p, c_p}: a position's chunks in chunk order
__global__ void __launch_bounds__(256) kadg_rowsum_kernel(const double* __restrict__ pw, int nw, const double* __restrict__ pc, int nc,
                                                          int64_t n_pad, int64_t n_total, double* __restrict__ rows) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_total) return;
    double w = 0.0, c = 0.0;
    for (int j = 0; j < nw; ++j) w += pw[(int64_t)j * n_pad + p];
    for (int j = 0; j < nc; ++j) c += pc[(int64_t)j * n_pad + p];
    rows[2 * p] = w;
    rows[2 * p + 1] = c;
}

// out[b] = {Sxx_b, Sxy_b}: strided per-thread sums over the group's positions, then a tree
__global__ void __launch_bounds__(256) kadg_finish_kernel(const double* __restrict__ rows, const int64_t* __restrict__ offs,
                                                          double* __restrict__ out) {
    __shared__ double redw[256], redc[256];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t p1 = offs[b + 1];
    double w = 0.0, c = 0.0;
    for (int64_t p = offs[b] + tid; p < p1; p += 256) {
        w += rows[2 * p];
        c += rows[2 * p + 1];
    }
    redw[tid] = w;
    redc[tid] = c;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) {
            redw[tid] += redw[tid + s];
            redc[tid] += redc[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        out[2 * b] = redw[0];
        out[2 * b + 1] = redc[0];
    }
}

// ---------------------------------------------------------------- host side
int launch_kadg_rowsum(const double* pw, int nw, const double* pc, int nc, int64_t n_pad, int64_t n_total, double* rows, hipStream_t st) {
    hipLaunchKernelGGL(kadg_rowsum_kernel, dim3((unsigned)ceil_div(n_total, 256)), dim3(256), 0, st, pw, nw, pc, nc, n_pad, n_total, rows);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

int launch_kadg_finish(const double* rows, const int64_t* offs, int B, double* out, hipStream_t st) {
    hipLaunchKernelGGL(kadg_finish_kernel, dim3((unsigned)B), dim3(256), 0, st, rows, offs, out);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

struct GroupsPlan {
    int64_t TP, TQ, n_pad;
    int chunk_c, nch_c;          // cross pass
    size_t slots_c;              // P tiles x chunks the workspace holds for it: monotone in TP and TQ, >= TP * nch_c
};

static GroupsPlan groups_plan(int64_t n_total, int64_t N2) {
    GroupsPlan p;
    p.TP = ceil_div(n_total, TB);
    p.TQ = ceil_div(N2, TB);
    p.n_pad = p.TP * TB;
    p.chunk_c = kadg_cross_chunk(p.TP, p.TQ);            // 128 doubles per (P tile, chunk)
    p.nch_c = (int)ceil_div(p.TQ, p.chunk_c);
    p.slots_c = (size_t)std::min<int64_t>(p.TP * p.TQ, std::max<int64_t>(KADG_CROSS_CHUNKS * p.TP, KADG_CROSS_SLOTS));
    return p;
}

struct GroupsWs {
    GroupHead head;
    unsigned* rowoff;
    int* gid;
    double *xn, *yn, *rows, *pw, *pc;
};

static bool groups_carve(Carver& c, int64_t n_total, int B, int64_t N2, const GroupsPlan& p, GroupsWs& w) {
    w.head = carve_group_head(c, B);
    w.rowoff = c.take<unsigned>((size_t)p.n_pad);
    w.gid = c.take<int>((size_t)p.n_pad);
    w.xn = c.take<double>((size_t)p.n_pad);
    w.yn = c.take<double>((size_t)N2);
    w.rows = c.take<double>(2 * (size_t)n_total);
    w.pw = c.take<double>((size_t)std::min<int64_t>(p.TP, KADG_WITHIN_CHUNKS) * (size_t)p.n_pad);
    w.pc = c.take<double>(p.slots_c * TB);
    return c.ok();
}

}  // namespace am

using namespace am;

extern "C" size_t am_mmd_rbf_groups_workspace_bytes(int64_t n_total, int B, int64_t N2, int D) {
    if (n_total < 1 || B < 1 || N2 < 2 || D < 1 || n_total >= ((int64_t)1 << 30)) return 0;
    Carver c(nullptr, 0);
    GroupsWs w;
    groups_carve(c, n_total, B, N2, groups_plan(n_total, N2), w);
    return c.off;
}

extern "C" int am_mmd_rbf_groups_f32(const float* X, int64_t N1, int64_t ldx, const int64_t* idx, const int64_t* offsets, int B,
                                     const float* Y, int64_t N2, int64_t ldy, int D, const float* bw2_dev, double gamma,
                                     double* out_groups, double* out_rows, void* ws, size_t ws_bytes, am_stream_t stream) {
    AM_REQUIRE(X && offsets && Y && out_groups, AM_ERR_BAD_ARG, "null pointer (X, offsets, Y, out_groups)");
    AM_REQUIRE(N1 >= 1 && D >= 1 && B >= 1, AM_ERR_BAD_SHAPE, "X has shape %lld x %d, B=%d (all must be >= 1)", (long long)N1, D, B);
    AM_REQUIRE(N2 >= 2, AM_ERR_BAD_SHAPE, "N2=%lld: the unbiased MMD^2 needs two reference rows", (long long)N2);
    AM_TRY(check_group_rows(X, N1, ldx, D));
    AM_REQUIRE(aligned16(Y) && ldy % 4 == 0 && ldy >= D, AM_ERR_BAD_ARG,
               "Y must be 16-byte aligned with ld %% 4 == 0 and ld >= D (ldy=%lld, D=%d)", (long long)ldy, D);
    AM_REQUIRE(!kad_too_large(N2, ldy), AM_ERR_BAD_SHAPE, "N2 * ldy * 4 bytes >= 4 GiB: one buffer descriptor spans the reference set");
    AM_REQUIRE(bw2_dev != nullptr || gamma >= 0.0, AM_ERR_BAD_ARG, "gamma must be >= 0 (or bw2_dev given)");
    int64_t n_total;
    AM_TRY(check_group_offsets(offsets, B, 0, &n_total));
    AM_REQUIRE(n_total < ((int64_t)1 << 30), AM_ERR_BAD_SHAPE, "offsets name %lld list positions (must stay below 2^30)", (long long)n_total);
    AM_TRY(check_stored_rows(idx, n_total, N1));
    const GroupsPlan plan = groups_plan(n_total, N2);
    Carver c(ws, ws_bytes);
    GroupsWs w;
    AM_REQUIRE(groups_carve(c, n_total, B, N2, plan, w), AM_ERR_WORKSPACE,
               "workspace too small: need %zu bytes (am_mmd_rbf_groups_workspace_bytes), have %zu", c.off, ws_bytes);
    const int64_t span = kadg_within_span(offsets, plan.TP, n_total, TB);
    const int chunk_w = kadg_within_chunk(span);
    const int nch_w = (int)ceil_div(span, chunk_w);      // <= min(TP, KADG_WITHIN_CHUNKS)
    hipStream_t st = static_cast<hipStream_t>(stream);
    AM_TRY(upload_group_head(w.head, offsets, B, st));
    const int64_t* offs = w.head.offs;
    int rc = launch_kad_norms(Y, ldy, D, N2, w.yn, st);
    if (rc != AM_OK) return rc;
    hipLaunchKernelGGL(kadg_prep_kernel, dim3((unsigned)ceil_div(plan.n_pad, 4)), dim3(256), 0, st, X, N1, ldx, D, idx,
                       offs, B, n_total, plan.n_pad, w.rowoff, w.xn, w.gid, w.head.flag);
    AM_LAUNCH_CHECK();
    auto launch = [&](auto cross, auto within) -> int {
        AM_HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(cross), (int)KADG_LDS_BYTES));
        AM_HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(within), (int)KADG_LDS_BYTES));
        hipLaunchKernelGGL(cross, dim3((unsigned)plan.TP, (unsigned)plan.nch_c), dim3(ENGINE_THREADS), KADG_LDS_BYTES, st, X, N1, ldx,
                           (const unsigned*)w.rowoff, (const double*)w.xn, (const int*)w.gid, offs, n_total, plan.n_pad,
                           Y, N2, ldy, (const double*)w.yn, D, plan.chunk_c, bw2_dev, gamma, w.pc);
        AM_LAUNCH_CHECK();
        hipLaunchKernelGGL(within, dim3((unsigned)plan.TP, (unsigned)nch_w), dim3(ENGINE_THREADS), KADG_LDS_BYTES, st, X, N1, ldx,
                           (const unsigned*)w.rowoff, (const double*)w.xn, (const int*)w.gid, offs, n_total, plan.n_pad,
                           Y, N2, ldy, (const double*)w.yn, D, chunk_w, bw2_dev, gamma, w.pw);
        AM_LAUNCH_CHECK();
        return AM_OK;
    };
    rc = (D % BK) != 0 ? launch(&kadg_rows_kernel<false, true>, &kadg_rows_kernel<true, true>)
                       : launch(&kadg_rows_kernel<false, false>, &kadg_rows_kernel<true, false>);
    if (rc != AM_OK) return rc;
    double* rows = out_rows ? out_rows : w.rows;
    AM_TRY(launch_kadg_rowsum(w.pw, nch_w, w.pc, plan.nch_c, plan.n_pad, n_total, rows, st));
    return launch_kadg_finish(rows, offs, B, out_groups, st);
}
