// Kernel Audio Distance support: an exact order statistic over the pairwise squared distances of a set, and the three
// full-set Gaussian kernel sums of the unbiased MMD^2 (Chung et al. 2025: bandwidth = median pairwise distance of the
// reference set).  Neither materialises a Gram matrix: both recompute 128 x 128 tiles on the f32 tile engine
// (tile_engine.h) and reduce them in the epilogue.
//
// Arithmetic of one pair, the same in both halves (KdEpilogue::finish_rbf):
//   d2 = max((|a|^2 + |b|^2) - 2 dot(a, b), 0) in f64, f64 squared norms (kad_norms_kernel), f32 matrix-core dot product.
//
// am_pairwise_select_f32: radix select on key = bits(rn32(d2)) - non-negative floats order as unsigned integers; NaN and
//   +inf both become +inf.  31 significant bits in three passes of 11 / 10 / 10 bits.  A pass sweeps the upper-triangular
//   tiles (P tile tp against Q tiles 0 .. tp; on the diagonal tile only p > q), bins the digit of every key that matches
//   the prefix found so far into a per-workgroup LDS histogram, and adds its non-zero counters to 64-bit global bins once,
//   at the end of the workgroup.  A one-workgroup scan kernel then turns (bins, rank) into the next prefix and the rank
//   inside that bin, in device memory: the call never synchronises with the host.
//   Contention: real embedding sets put nearly all distances within a factor of two, i.e. into a handful of the first
//   pass's bins.  Before any LDS atomic a wave combines equal digits: the first live lane's digit is broadcast, the lanes
//   that hold the same digit are counted with a ballot and ONE lane adds the count; after KAD_AGG_ROUNDS such rounds the
//   lanes still live (digits spread over many bins: passes 2 and 3) add 1 each.
//
// am_mmd_rbf_f32: Sxx, Syy (ordered pairs i != j: upper-triangular tiles, off-diagonal tiles weighted 2, the valid
//   diagonal dropped) and Sxy (all tiles) of K = exp(-d2 gamma) in f64.  One f64 partial per workgroup, written to its own
//   slot and summed by one workgroup in a fixed order (mmd_multi_reduce_kernel, through launch_mmd_reduce): identical inputs
//   give identical bits.  (kad_mmd_kernel is the Gaussian one-scale case of mmd_multi_kernel in all but 0.15 % of run time:
//   routed through that kernel, mmd_rbf_sums at 20 000 x 20 000 x 512 took 7.280 ms against 7.270 ms, so it stays.)
//
// This file also defines what the family shares and kad_common.h declares: the f32 norms and the scan kernel behind their
// launchers, the chunk rules, the grid plan of the three whole-set blocks, the workspace carves and the validation of two f32
// sets.
#include "am_common.h"
#include "kad_common.h"
#include "pairwise_common.h"
#include <algorithm>

namespace am {

// 73 728 B of staging slabs + 8 192 B of counters = 81 920 B: exactly two workgroups in a CU's 160 KiB
constexpr size_t KAD_SELECT_LDS_BYTES = ENGINE_LDS_FLOATS * sizeof(float) + KAD_BINS * sizeof(unsigned);
constexpr size_t KAD_MMD_LDS_BYTES = ENGINE_LDS_FLOATS * sizeof(float);

// out[i] = |X[i]|^2 in f64 (one wave per row)
__global__ void __launch_bounds__(256) kad_norms_kernel(const float* __restrict__ X, int64_t ld, int D, int64_t N,
                                                        double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= N) return;
    const float* x = X + e * ld;
    double acc = 0.0;
    for (int k = lane * 4; k < D; k += 256) {
        const f32x4 v = load_k4(x, k, D);
        acc += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) out[e] = acc;
}

template <int PASS>
struct SelectEpilogue {
    const double* norm;
    int64_t n, ptile;
    unsigned prefix;
    unsigned* hist;
    double pnorm[2];
    bool pok[2];
    const LaneInfo& L;
    __device__ __forceinline__ SelectEpilogue(const LaneInfo& l) : L(l) {}
    __device__ __forceinline__ void aux_issue(int, int64_t) {}
    __device__ __forceinline__ void aux_commit(int) {}
    __device__ __forceinline__ void finish(int, int64_t qtile, f32x16 (&acc)[2][2]) {
        const bool diag = qtile == ptile;                               // Q tiles run 0 .. ptile: elsewhere p > q holds
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int64_t q = qtile * TB + L.wm * 64 + mt * 32 + (i & 3) + 8 * (i >> 2) + 4 * L.h;
                const bool qok = q < n;
                const double qnorm = qok ? norm[q] : 0.0;
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const int64_t p = ptile * TB + L.wn * 64 + nt * 32 + L.r;
                    double d2 = (qnorm + pnorm[nt]) - 2.0 * (double)acc[mt][nt][i];
                    d2 = d2 < 0.0 ? 0.0 : d2;
                    float kf = (float)d2;                               // round to nearest: monotone, so select-then-round = round-then-select
                    kf = kf < INFINITY ? kf : INFINITY;                 // NaN (a non-finite row) and overflow: +inf
                    const unsigned key = __float_as_uint(kf) & 0x7fffffffu;
                    bool live = qok && pok[nt] && (!diag || p > q);
                    // (the digits stay in line here and in kad64_select_kernel: behind a shared helper, by value or by
                    // reference, both kernels compile to other code - 1% more or fewer instructions, two more registers)
                    unsigned digit;
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
            }
    }
};

// grid: x = P tile (heaviest first), y = chunk of `chunk_tiles` Q tiles; chunks past the diagonal have nothing to do
template <int PASS, bool KTAIL>
__global__ void __launch_bounds__(ENGINE_THREADS, 2)
kad_select_kernel(const float* __restrict__ X, int64_t N, int64_t ld, int D, const double* __restrict__ norm, int chunk_tiles,
                  const SelectState* __restrict__ state, unsigned long long* __restrict__ bins) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LaneInfo L;
    const int64_t T = (N + TB - 1) / TB;
    const int64_t tp = T - 1 - (int64_t)blockIdx.x;
    const int64_t q0 = (int64_t)blockIdx.y * chunk_tiles;
    if (q0 > tp) return;
    const int64_t left = tp + 1 - q0;
    const int ntiles = left < chunk_tiles ? (int)left : chunk_tiles;
    unsigned* hist = reinterpret_cast<unsigned*>(lds + ENGINE_LDS_FLOATS);
    for (int b = L.tid; b < KAD_BINS; b += ENGINE_THREADS) hist[b] = 0u;      // visible after the pipeline's first barrier
    SelectEpilogue<PASS> epi(L);
    epi.norm = norm;
    epi.n = N;
    epi.ptile = tp;
    epi.prefix = PASS == 0 ? 0u : state->prefix;
    epi.hist = hist;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int64_t p = tp * TB + L.wn * 64 + nt * 32 + L.r;
        epi.pok[nt] = p < N;
        epi.pnorm[nt] = p < N ? norm[p] : 0.0;
    }
    dense_pipeline_early<EV_DEFAULT, KTAIL>(X, N, ld, LinearTiles{q0}, X, N, ld, tp * TB, ntiles, D, lds, L, epi);
    // (the pipeline's last stage ends with a barrier: the counters are complete) - one global flush per workgroup
    for (int b = L.tid; b < KAD_BINS; b += ENGINE_THREADS) {
        const unsigned c = hist[b];
        if (c != 0u) atomicAdd(bins + b, (unsigned long long)c);
    }
}

// One workgroup: the bin that holds the wanted rank -> next prefix, rank inside that bin; the last pass writes the value.
template <int PASS>
__global__ void __launch_bounds__(256) kad_scan_kernel(const unsigned long long* __restrict__ bins, SelectState* state,
                                                       unsigned long long rank0, float* __restrict__ out) {
    __shared__ unsigned long long part[256];
    const int tid = threadIdx.x;
    constexpr int PER = KAD_BINS / 256;
    unsigned long long c[PER], sum = 0ull;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        c[j] = bins[tid * PER + j];
        sum += c[j];
    }
    part[tid] = sum;
    const unsigned long long rank = PASS == 0 ? rank0 : state->rank;
    const unsigned prefix = PASS == 0 ? 0u : state->prefix;
    __syncthreads();                                  // every thread holds the old state before one of them replaces it
    if (tid == 0) {
        unsigned long long run = 0ull;
        for (int t = 0; t < 256; ++t) {
            const unsigned long long v = part[t];
            part[t] = run;
            run += v;
        }
    }
    __syncthreads();
    unsigned long long cum = part[tid];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        if (rank >= cum && rank < cum + c[j]) {       // exactly one (thread, j): the bins hold every pair once
            const unsigned digit = (unsigned)(tid * PER + j);
            const unsigned next = PASS == 0 ? digit : ((prefix << 10) | digit);
            state->rank = rank - cum;
            state->prefix = next;
            if (PASS == KAD_PASSES - 1) *out = __uint_as_float(next);
        }
        cum += c[j];
    }
}

// ------------------------------------------------------------------------------------------------ kernel sums

struct MmdEpilogue {
    const double* qn;            // f64 squared norms of the Q / P rows
    int64_t nq, np, ptile;
    double gamma;
    bool sym;                    // Q and P are the same set: tile (tq, tp), tq < tp, stands for its mirror image too
    double sum;
    double pnorm[2];             // +inf for padded rows: exp(-inf) = 0, they contribute exactly 0
    const LaneInfo& L;
    __device__ __forceinline__ MmdEpilogue(const LaneInfo& l) : L(l) {}
    __device__ __forceinline__ void aux_issue(int, int64_t) {}
    __device__ __forceinline__ void aux_commit(int) {}
    // (rows are indexed in 32 bits: N * ld * 4 < 4 GiB and ld >= 4 put N below 2^28)
    __device__ __forceinline__ void finish(int, int64_t qtile, f32x16 (&acc)[2][2]) {
        const bool diag = sym && qtile == ptile;
        const int q0 = (int)qtile * TB + L.wm * 64 + 4 * L.h, p0 = (int)ptile * TB + L.wn * 64 + L.r;
        double s = 0.0;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int q = q0 + mt * 32 + (i & 3) + 8 * (i >> 2);
                const double qnorm = q < (int)nq ? qn[q] : INFINITY;
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    double d2 = (qnorm + pnorm[nt]) - 2.0 * (double)acc[mt][nt][i];
                    d2 = d2 < 0.0 ? 0.0 : d2;
                    const double k = exp(-d2 * gamma);
                    s += (diag && p0 + nt * 32 == q) ? 0.0 : k;
                }
                if ((i & 1) == 1) __builtin_amdgcn_sched_barrier(0);    // four exp chains at a time: more in flight spill
            }
        sum += (sym && !diag) ? 2.0 * s : s;
    }
};

// grid: x = P tile, y = chunk of Q tiles; partial[y * gridDim.x + x] = this workgroup's weighted sum (0 for an empty chunk).
// Kxy[a][b] = k(x_a, y_b): Q rows (register axis) from set 1, P rows (lane axis) from set 2.
template <bool KTAIL>
__global__ void __launch_bounds__(ENGINE_THREADS, 2)
kad_mmd_kernel(const float* __restrict__ Q, int64_t nq, int64_t ldq, const double* __restrict__ qn, const float* __restrict__ P,
               int64_t np, int64_t ldp, const double* __restrict__ pn, int D, int sym, int chunk_tiles,
               const float* __restrict__ bw2_dev, double gamma, double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LaneInfo L;
    const int64_t TQ = (nq + TB - 1) / TB, TP = (np + TB - 1) / TB;
    const int64_t tp = sym ? TP - 1 - (int64_t)blockIdx.x : (int64_t)blockIdx.x;
    const int64_t q0 = (int64_t)blockIdx.y * chunk_tiles;
    const int64_t qlast = sym ? tp : TQ - 1;
    const int64_t slot = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (q0 > qlast) {
        if (L.tid == 0) partial[slot] = 0.0;
        return;
    }
    const int64_t left = qlast + 1 - q0;
    const int ntiles = left < chunk_tiles ? (int)left : chunk_tiles;
    MmdEpilogue epi(L);
    epi.qn = qn;
    epi.nq = nq;
    epi.np = np;
    epi.ptile = tp;
    epi.gamma = bw2_dev != nullptr ? 0.5 / (double)*bw2_dev : gamma;      // the median feeds the sums without a host round trip
    epi.sym = sym != 0;
    epi.sum = 0.0;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int64_t p = tp * TB + L.wn * 64 + nt * 32 + L.r;
        epi.pnorm[nt] = p < np ? pn[p] : INFINITY;
    }
    dense_pipeline_early<EV_DEFAULT, KTAIL>(Q, nq, ldq, LinearTiles{q0}, P, np, ldp, tp * TB, ntiles, D, lds, L, epi);
    double v = epi.sum;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    double* red = reinterpret_cast<double*>(lds);          // staging slabs are idle after the pipeline's last barrier
    if (L.lane == 0) red[L.tid >> 6] = v;
    __syncthreads();
    if (L.tid == 0) partial[slot] = ((red[0] + red[1]) + red[2]) + red[3];
}

// Q tiles per workgroup (kad_common.h)
int kad_chunk(int64_t tiles_total, int64_t q_tiles) {
    int64_t ch = std::min<int64_t>(KAD_MAX_CHUNK, std::max<int64_t>(1, tiles_total / 2048));
    while (ceil_div(q_tiles, ch) > 65535) ch *= 2;
    return (int)ch;
}

bool kad_too_large(int64_t N, int64_t ld) { return (uint64_t)N * (uint64_t)ld * 4u >= 0xffffffffull; }

int launch_kad_norms(const float* X, int64_t ld, int D, int64_t N, double* out, hipStream_t st) {
    hipLaunchKernelGGL(kad_norms_kernel, dim3((unsigned)ceil_div(N, 4)), dim3(256), 0, st, X, ld, D, N, out);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

int launch_kad_scan(int pass, const unsigned long long* bins, SelectState* state, unsigned long long rank0, float* out, hipStream_t st) {
    auto kernel = pass == 0 ? &kad_scan_kernel<0> : pass == 1 ? &kad_scan_kernel<1> : &kad_scan_kernel<2>;
    hipLaunchKernelGGL(kernel, dim3(1), dim3(256), 0, st, bins, state, rank0, out);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

SelectWs select_carve(void* ws, size_t ws_bytes, int64_t N) {
    Carver c(ws, ws_bytes);
    SelectWs w{};
    w.norm = c.take<double>((size_t)N);
    w.bins = c.take<unsigned long long>((size_t)KAD_PASSES * KAD_BINS);
    w.state = c.take<SelectState>(1);
    w.bytes = c.off;
    w.ok = c.ok();
    return w;
}

template <int PASS>
static int launch_select_pass(const float* X, int64_t N, int64_t ld, int D, const double* norm, int chunk, SelectState* state,
                              unsigned long long* bins, unsigned long long rank0, float* out, hipStream_t st) {
    const int64_t T = ceil_div(N, TB);
    const dim3 grid((unsigned)T, (unsigned)ceil_div(T, chunk));
    auto launch = [&](auto kernel) -> int {
        AM_HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), (int)KAD_SELECT_LDS_BYTES));
        hipLaunchKernelGGL(kernel, grid, dim3(ENGINE_THREADS), KAD_SELECT_LDS_BYTES, st, X, N, ld, D, norm, chunk,
                           (const SelectState*)state, bins + (size_t)PASS * KAD_BINS);
        AM_LAUNCH_CHECK();
        return AM_OK;
    };
    const int rc = (D % BK) != 0 ? launch(&kad_select_kernel<PASS, true>) : launch(&kad_select_kernel<PASS, false>);
    if (rc != AM_OK) return rc;
    return launch_kad_scan(PASS, bins + (size_t)PASS * KAD_BINS, state, rank0, out, st);
}

// ------------------------------------------------------------------------------------------------ shared host side (kad_common.h)
MmdPlan mmd_plan(int64_t N1, int64_t N2, int tile_rows) {
    MmdPlan p;
    const int64_t T1 = ceil_div(N1, tile_rows), T2 = ceil_div(N2, tile_rows);
    const int64_t tq[3] = {T1, T2, T1}, tp[3] = {T1, T2, T2};
    for (int b = 0; b < 3; ++b) {
        const int64_t total = b < 2 ? tp[b] * (tp[b] + 1) / 2 : tq[b] * tp[b];
        p.chunk[b] = kad_chunk(total, tq[b]);
        p.grid[b] = dim3((unsigned)tp[b], (unsigned)ceil_div(tq[b], p.chunk[b]));
        p.slots[b] = (size_t)p.grid[b].x * p.grid[b].y;
    }
    return p;
}

SetNorms carve_set_norms(Carver& c, int64_t N1, int64_t N2, unsigned blocks) {
    SetNorms n{};
    if (blocks & (AM_MMD_XX | AM_MMD_XY)) n.n1 = c.take<double>((size_t)N1);
    if (blocks & (AM_MMD_YY | AM_MMD_XY)) n.n2 = c.take<double>((size_t)N2);
    return n;
}

int launch_set_norms(const float* X, int64_t N1, int64_t ldx, const float* Y, int64_t N2, int64_t ldy, int D, const SetNorms& n,
                     hipStream_t st) {
    int rc = n.n1 ? launch_kad_norms(X, ldx, D, N1, n.n1, st) : AM_OK;
    if (rc == AM_OK && n.n2) rc = launch_kad_norms(Y, ldy, D, N2, n.n2, st);
    return rc;
}

MmdWs mmd_carve(void* ws, size_t ws_bytes, int64_t N1, int64_t N2, int nscales, unsigned blocks, const MmdPlan& plan) {
    Carver c(ws, ws_bytes);
    MmdWs w{};
    w.n = carve_set_norms(c, N1, N2, blocks);
    for (int b = 0; b < 3; ++b)
        if (blocks & (1u << b)) w.partial[b] = c.take<double>(plan.slots[b] * (size_t)nscales);
    w.bytes = c.off;
    w.ok = c.ok();
    return w;
}

int kadg_cross_chunk(int64_t TP, int64_t TQ) {
    const int64_t cap = std::max<int64_t>(KADG_CROSS_CHUNKS, KADG_CROSS_SLOTS / TP);
    return (int)std::max<int64_t>(kad_chunk(TP * TQ, TQ), ceil_div(TQ, cap));
}

int64_t kadg_within_span(const int64_t* offsets, int64_t TP, int64_t n_total, int tile_rows) {
    int64_t span = 1;
    for (int64_t t = 0, g0 = 0, g1 = 0; t < TP; ++t) {
        const int64_t pfirst = t * tile_rows, plast = std::min<int64_t>(pfirst + tile_rows, n_total) - 1;
        while (offsets[g0 + 1] <= pfirst) ++g0;
        g1 = std::max(g1, g0);
        while (offsets[g1 + 1] <= plast) ++g1;
        span = std::max<int64_t>(span, (offsets[g1 + 1] - 1) / tile_rows - offsets[g0] / tile_rows + 1);
    }
    return span;
}

int kadg_within_chunk(int64_t span) { return (int)std::max<int64_t>(KAD_MAX_CHUNK, ceil_div(span, KADG_WITHIN_CHUNKS)); }

int check_two_sets_f32(const float* X, int64_t N1, int64_t ldx, const float* Y, int64_t N2, int64_t ldy, int D, unsigned blocks) {
    AM_REQUIRE(X && Y, AM_ERR_BAD_ARG, "null pointer");
    AM_REQUIRE(blocks != 0 && (blocks & ~7u) == 0, AM_ERR_BAD_ARG, "blocks = %u is not a mask of AM_MMD_XX | AM_MMD_YY | AM_MMD_XY", blocks);
    AM_REQUIRE(N1 >= 1 && N2 >= 1 && D >= 1, AM_ERR_BAD_SHAPE, "N1=%lld N2=%lld D=%d", (long long)N1, (long long)N2, D);
    AM_REQUIRE(aligned16(X) && aligned16(Y) && ldx % 4 == 0 && ldy % 4 == 0 && ldx >= D && ldy >= D, AM_ERR_BAD_ARG,
               "X/Y must be 16-byte aligned with ld %% 4 == 0 and ld >= D");
    AM_REQUIRE(!kad_too_large(N1, ldx) && !kad_too_large(N2, ldy), AM_ERR_BAD_SHAPE,
               "N * ld * 4 bytes of a set >= 4 GiB: one buffer descriptor spans a matrix");
    return AM_OK;
}

}  // namespace am

using namespace am;

extern "C" size_t am_pairwise_select_workspace_bytes(int64_t N, int D) {
    if (N < 2 || D < 1) return 0;
    return select_carve(nullptr, 0, N).bytes;
}

extern "C" int am_pairwise_select_f32(const float* X, int64_t N, int64_t ld, int D, int64_t rank, float* out_d2, void* ws,
                                      size_t ws_bytes, am_stream_t stream) {
    AM_REQUIRE(X && out_d2, AM_ERR_BAD_ARG, "null pointer");
    AM_REQUIRE(N >= 2 && D >= 1, AM_ERR_BAD_SHAPE, "N=%lld D=%d: an order statistic of pairwise distances needs two rows",
               (long long)N, D);
    AM_REQUIRE(aligned16(X) && ld % 4 == 0 && ld >= D, AM_ERR_BAD_ARG, "X must be 16-byte aligned with ld %% 4 == 0 and ld >= D");
    AM_REQUIRE(!kad_too_large(N, ld), AM_ERR_BAD_SHAPE, "N * ld * 4 = %llu bytes: one buffer descriptor spans the matrix (< 4 GiB)",
               (unsigned long long)N * (unsigned long long)ld * 4ull);
    const int64_t pairs = N * (N - 1) / 2;               // N < 2^28 (ld >= 4): no overflow
    AM_REQUIRE(rank < pairs, AM_ERR_BAD_SHAPE, "rank %lld of %lld pairs", (long long)rank, (long long)pairs);
    if (rank < 0) rank = (pairs - 1) / 2;                // lower median (torch.median's convention)
    const SelectWs w = select_carve(ws, ws_bytes, N);
    AM_REQUIRE(w.ok, AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (am_pairwise_select_workspace_bytes), have %zu", w.bytes,
               ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AM_HIP_TRY(hipMemsetAsync(w.bins, 0, (size_t)KAD_PASSES * KAD_BINS * sizeof(unsigned long long), st));
    int rc = launch_kad_norms(X, ld, D, N, w.norm, st);
    const int64_t T = ceil_div(N, TB);
    const int chunk = kad_chunk(T * (T + 1) / 2, T);
    if (rc == AM_OK) rc = launch_select_pass<0>(X, N, ld, D, w.norm, chunk, w.state, w.bins, (unsigned long long)rank, out_d2, st);
    if (rc == AM_OK) rc = launch_select_pass<1>(X, N, ld, D, w.norm, chunk, w.state, w.bins, 0ull, out_d2, st);
    if (rc == AM_OK) rc = launch_select_pass<2>(X, N, ld, D, w.norm, chunk, w.state, w.bins, 0ull, out_d2, st);
    return rc;
}

extern "C" size_t am_mmd_rbf_workspace_bytes(int64_t N1, int64_t N2, int D, unsigned blocks) {
    if (N1 < 1 || N2 < 1 || D < 1 || (blocks & 7u) == 0) return 0;
    return mmd_carve(nullptr, 0, N1, N2, 1, blocks & 7u, mmd_plan(N1, N2, TB)).bytes;
}

extern "C" int am_mmd_rbf_f32(const float* X, int64_t N1, int64_t ldx, const float* Y, int64_t N2, int64_t ldy, int D,
                              const float* bw2_dev, double gamma, unsigned blocks, double* out_sums, void* ws, size_t ws_bytes,
                              am_stream_t stream) {
    AM_REQUIRE(out_sums, AM_ERR_BAD_ARG, "null pointer");
    int rc = check_two_sets_f32(X, N1, ldx, Y, N2, ldy, D, blocks);
    if (rc != AM_OK) return rc;
    AM_REQUIRE(bw2_dev != nullptr || gamma >= 0.0, AM_ERR_BAD_ARG, "gamma must be >= 0 (or bw2_dev given)");
    const MmdPlan plan = mmd_plan(N1, N2, TB);
    const MmdWs w = mmd_carve(ws, ws_bytes, N1, N2, 1, blocks, plan);
    AM_REQUIRE(w.ok, AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (am_mmd_rbf_workspace_bytes), have %zu", w.bytes, ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = launch_set_norms(X, N1, ldx, Y, N2, ldy, D, w.n, st);
    if (rc != AM_OK) return rc;
    auto launch = [&](auto kernel) -> int {
        AM_HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), (int)KAD_MMD_LDS_BYTES));
        for (int b = 0; b < 3; ++b) {
            if (!(blocks & (1u << b))) continue;
            const bool q_is_y = b == 1, p_is_x = b == 0;
            hipLaunchKernelGGL(kernel, plan.grid[b], dim3(ENGINE_THREADS), KAD_MMD_LDS_BYTES, st,
                               q_is_y ? Y : X, q_is_y ? N2 : N1, q_is_y ? ldy : ldx, (const double*)(q_is_y ? w.n.n2 : w.n.n1),
                               p_is_x ? X : Y, p_is_x ? N1 : N2, p_is_x ? ldx : ldy, (const double*)(p_is_x ? w.n.n1 : w.n.n2),
                               D, b < 2 ? 1 : 0, plan.chunk[b], bw2_dev, gamma, w.partial[b]);
            AM_LAUNCH_CHECK();
            const int rr = launch_mmd_reduce(w.partial[b], (int64_t)plan.slots[b], 1, out_sums + b, st);
            if (rr != AM_OK) return rr;
        }
        return AM_OK;
    };
    return (D % BK) != 0 ? launch(&kad_mmd_kernel<true>) : launch(&kad_mmd_kernel<false>);
}
