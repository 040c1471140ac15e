// Exact k-nearest-neighbour SEARCH: for every row of X the k smallest distances to the rows of Y and the rows they
// belong to, without an N x M matrix.  The radii of the PRDC path (pairwise.hip: knn_partial_kernel / KnnEpilogue) keep
// lane-local sorted lists of the smallest d2 of a row and drop the column each value came from; this file keeps it.
//
// Arithmetic of one pair, exactly that of KnnEpilogue on the same 128 x 128 f32 tile engine (tile_engine.h,
// v_mfma_f32_32x32x2_f32, dense_pipeline_early with the production schedule):
//     d2 = max(fmaf(-2, <x, y>, |x|^2 + |y|^2), 0)       NaN -> +inf (clamp0); a padded column has |y|^2 = +inf
// with the f32 row norms of row_sqnorm_kernel (launch_norms of pairwise.hip).  Every reported squared
// distance therefore has the bits of the exact general kernel and of oracle/exact_c/pairwise_exact.c.
//
// Lists.  A list entry is ONE 64-bit key
//     key = (uint64)(bits(d2) & 0x7fffffff) << 32 | column
// Non-negative floats order like their bit patterns, so one unsigned compare orders by distance and then by column: ties
// go to the smallest column whatever the chunking, the tile order or the lane that saw the value - a call returns the
// same bits every time.  The column of accumulator register `reg` of tile mt is
//     qtile * 128 + wm * 64 + mt * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h
// = a per-tile base plus a compile-time constant; no index array lives in registers.  The two gates of KnnEpilogue are
// kept on the VALUE (the list's last distance is the high word of its last key): the tile minimum, then __any per
// element; after warm-up almost no tile reaches the 64-bit insert.  The gates are strict (d2 < last): a lane meets the
// columns of its chunk in increasing order and its list holds admissible columns only, so a value equal to the list's
// last distance always has the larger column and loses the tie anyway; the insert itself compares whole keys.
//
// Which columns a row skips is a POLICY (ByIndex, ByLabel below): what the kernel is handed, what the epilogue keeps
// for it, and three places of `finish`.  Everything else - the epilogue, the tile kernel's body with its two-pass list
// join, the merge kernels, the entry's validation, workspace and norms - exists once.
//
// Column chunks: the (row block) x (column chunk) plan of the radii (work_item / choose_chunks of pairwise_common.h).
// Partial lists: uint64 [nchunks][N][KCAP] in the caller's workspace; knn_search_merge_kernel takes the k smallest
// keys of a row and writes sqrt_rn(d2) (or d2) and the column as int64, -1 where the distance is +inf (fewer than k
// finite candidates: M < k, fewer than k admissible columns, non-finite rows).
//
// Register budget (lists are 2 rows x KCAP keys x 2 registers per lane, beside 64 accumulators and the staging /
// fragment registers of the pipeline; ByLabel has two label registers in place of ByIndex's diagonal bookkeeping; no
// instantiation of either policy uses scratch - tests/test_knn_search_resources_cpu.py):
//     KCAP  8:  32 list registers, __launch_bounds__(256, 2), two workgroups per CU
//     KCAP 16:  64 list registers, __launch_bounds__(256, 2), two workgroups per CU
//     KCAP 32: 128 list registers, __launch_bounds__(256, 1): ONE workgroup per CU (the lists alone are half of the 256
//              registers a wave has at two per SIMD)
#include "row_sweep.h"

namespace am {
namespace search {

constexpr int MAX_K = 32;
constexpr unsigned long long EMPTY_KEY = 0x7f800000ffffffffull;          // (+inf, no column): larger than every real key
constexpr unsigned INF_BITS = 0x7f800000u;

__host__ __device__ constexpr int kcap_for(int k) { return k <= 8 ? 8 : k <= 16 ? 16 : 32; }

// Branch-free sorted insertion of a key into an ascending list of CAP keys (list_insert of tile_engine.h on uint64:
// compare-exchange down the list, fully unrolled).  A key >= best[CAP-1] falls through.
template <int CAP>
__device__ __forceinline__ void key_insert(unsigned long long (&best)[CAP], unsigned long long x) {
#pragma unroll
    for (int i = 0; i < CAP; ++i) {
        const bool lt = x < best[i];
        const unsigned long long lo = lt ? x : best[i];
        x = lt ? best[i] : x;
        best[i] = lo;
    }
}

// ---- exclusion policies ----------------------------------------------------------------------------------------------------
// A policy names the types of what only it needs - Labels: the label array of a side, as the kernel is handed it; Label: one
// row's label in a register; SelfOffset: the shift of the excluded diagonal - and gives the other policy's the type Absent
// (row_sweep.h), which takes no room: neither in the kernel's arguments nor in the epilogue.  So the one kernel and the one
// epilogue below list every policy's arguments and members, each in ITS place: a label array beside the norms of its side, the
// offset behind nchunks, the label registers behind the norm registers.  Both orders are part of the program - the kernarg
// offsets of the parameter list, the order of the epilogue's members through the order in which the compiler promotes them to
// registers - and gathered into one struct per policy, at one place, every instruction stream of this file moved
// (profiles/exclusion_policy/isa_compare.txt).  ARRAYS: the per-column arrays a tile brings through LDS,
// [2][ARRAYS][128] - array 0 is |y_j|^2 (+inf past the end).

// Self exclusion by INDEX: column i + self_offset is skipped for row i (self_offset < 0: none; duplicates of a row stay
// its neighbours), and only the tiles the shifted diagonal crosses run the variant of the gates that tests for it.
struct ByIndex {
    static constexpr bool BY_LABEL = false;
    static constexpr int ARRAYS = 1;
    using Labels = Absent;
    using Label = Absent;
    using SelfOffset = int64_t;
};

// A whole GROUP left out, by LABEL: every row of X and of Y carries one int32 label, and row i of X skips the rows of Y
// whose label equals its own.  The embedding pipeline cuts every file into windows, so stored rows come in runs of
// near-duplicates per track; with "row i itself, by index" as the only exclusion the nearest neighbour of almost every
// window is a sibling window of its own song.
//
// Labels.  The column labels travel beside the column norms through LDS as array 1, the 32 bits of the label (the layout
// of ColumnAux of row_sweep.h, staged by hand because array 1 is not a float: a label is only moved and compared for
// equality, never computed with).  A lane keeps the labels of its two rows in two registers.  There is no diagonal:
// which columns a row skips is not tied to its index.
//
// Gates.  Both gates - the tile minimum, then __any per element - run on the plain values and do not know about the
// exclusion: they are supersets (a 32 x 32 sub-tile that holds a same-label pair closer than the row's list end always
// passes the first one), which costs time and never a result, because the exclusion is applied where a key is made:
// inside the wave-uniform insert loop, where one LDS word per candidate is read already,
//     d2 = (label[column] == label[row]) ? +inf : clamp0(u)
// and a key at +inf never displaces a finite one (the merge reports it as (+inf, -1)).  The gates stay strict: the
// list holds admissible columns only, and the lane still meets them in increasing order.
struct ByLabel {
    static constexpr bool BY_LABEL = true;
    static constexpr int ARRAYS = 2;
    using Labels = const int32_t* __restrict__;
    using Label = int32_t;
    using SelfOffset = Absent;
};

template <class Excl>
constexpr size_t LDS_BYTES = (ENGINE_LDS_FLOATS + 2 * Excl::ARRAYS * TB) * sizeof(float);   // staging slabs + [2][ARRAYS][128] column values

template <int KCAP, class Excl>
struct KnnListEpilogue {
    const float* qnorm;
    typename Excl::Labels qgroup;
    int64_t nq;
    float* aux;                          // LDS [2][ARRAYS][128] : |y_j|^2 of the tile (+inf past nq), then the labels' bits
    typename Excl::SelfOffset self_lo;   // column excluded for the first row of this row block (row r: self_lo + r); none: -2 * TB
    float xn[2];
    typename Excl::Label xg[2];          // the labels of the lane's two rows
    unsigned long long best[2][KCAP];
    float aux_reg;
    typename Excl::Label aux_grp;
    const LaneInfo& L;

    __device__ __forceinline__ KnnListEpilogue(const LaneInfo& l) : L(l) {}
    __device__ __forceinline__ void aux_issue(int, int64_t qtile) {
        if (L.tid < TB) {
            const int64_t j = qtile * TB + L.tid;
            aux_reg = j < nq ? qnorm[j] : INFINITY;
            if constexpr (Excl::BY_LABEL) aux_grp = j < nq ? qgroup[j] : 0;     // never looked at: such a pair is at +inf already
        }
    }
    __device__ __forceinline__ void aux_commit(int t) {
        if (L.tid < TB) {
            aux[(t & 1) * Excl::ARRAYS * TB + L.tid] = aux_reg;
            if constexpr (Excl::BY_LABEL) reinterpret_cast<int32_t*>(aux)[(t & 1) * 2 * TB + TB + L.tid] = aux_grp;
        }
    }
    __device__ __forceinline__ float last(int nt) const { return __uint_as_float((unsigned)(best[nt][KCAP - 1] >> 32)); }

    // The two gates run on values that are recomputed, not kept (16 more live registers cost the KCAP 16 form its second
    // workgroup per CU), and unclamped: max(., 0) commutes with min, and a NaN loses every compare.  ByIndex: on a tile the
    // shifted diagonal crosses (wave-uniform `diag`) the lane's excluded column counts as +inf.  ByLabel: the gates see ALL
    // columns, the row's own group included.  Past the gates, the registers that may improve some lane's list are visited
    // through a wave-uniform bit mask, so that the 64-bit insert is instantiated once per accumulator tile and not once per
    // register (unrolled 16 times it pushed the KCAP 16 / 32 kernels over the unroll budget and their accumulators into
    // scratch).  The mask is taken before the inserts tighten the list: a superset, and a key that no longer fits falls
    // through the insert.  Only in that loop is a column's label read and compared.
    __device__ __forceinline__ void finish(int t, int64_t qtile, f32x16 (&acc)[2][2]) {
        const float* a = aux + (t & 1) * Excl::ARRAYS * TB + L.wm * 64 + L.h * 4;
        const int32_t* g = reinterpret_cast<const int32_t*>(a + TB);          // ByLabel: the labels of the lane's columns
        const int64_t c0 = qtile * TB + L.wm * 64 + L.h * 4;       // the lane's first column of the tile
        const unsigned cbase = (unsigned)c0;
        bool diag = false;
        int srel[2] = {-1, -1};                                     // ByIndex: excluded column relative to c0 (-1: not in this tile)
        if constexpr (!Excl::BY_LABEL) {
            diag = qtile * TB < self_lo + TB && qtile * TB + TB > self_lo;
            if (diag) {
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const int64_t rel = self_lo + sweep_row(0, L, nt) - c0;
                    srel[nt] = (rel >= 0 && rel < 64) ? (int)rel : -1;
                }
            }
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            f32x4 yn[4];
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) yn[g4] = *reinterpret_cast<const f32x4*>(a + mt * 32 + g4 * 8);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                auto value = [&](int reg, bool self_test) {
                    const float u = fmaf(-2.f, acc[mt][nt][reg], xn[nt] + yn[reg >> 2][reg & 3]);
                    if constexpr (Excl::BY_LABEL) return u;
                    else return (self_test && mt * 32 + (reg & 3) + 8 * (reg >> 2) == srel[nt]) ? INFINITY : u;   // the row itself: by index
                };
                float tmin = INFINITY;
                if (diag) {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) tmin = fminf(tmin, value(reg, true));
                } else {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) tmin = fminf(tmin, value(reg, false));
                }
                tmin = fmaxf(tmin, 0.f);
                // common case after warm-up: no lane of the wave improves its list with this 32 x 32 tile
                if (__any(tmin < last(nt))) {
                    unsigned mask = 0;
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg)
                        if (__any(value(reg, true) < last(nt))) mask |= 1u << reg;
                    while (mask != 0) {                             // wave-uniform, ascending registers = ascending columns
                        const int reg = __builtin_ctz(mask);
                        mask &= mask - 1;
                        const int rel = mt * 32 + (reg & 3) + 8 * (reg >> 2);
                        float p = acc[mt][nt][0];
#pragma unroll
                        for (int q = 1; q < 16; ++q) p = (reg == q) ? acc[mt][nt][q] : p;
                        const float u = fmaf(-2.f, p, xn[nt] + a[rel]);
                        bool skipped;
                        if constexpr (Excl::BY_LABEL) skipped = g[rel] == xg[nt];      // the row's own group: by label
                        else skipped = rel == srel[nt];
                        const float d2 = skipped ? INFINITY : clamp0(u);
                        key_insert<KCAP>(best[nt], ((unsigned long long)(__float_as_uint(d2) & 0x7fffffffu) << 32) | (cbase + (unsigned)rel));
                    }
                }
            }
        }
    }
};

// partial[(chunk * N + row) * KCAP + s] = s-th smallest key of `row` inside column chunk `chunk`
template <int KCAP, bool KTAIL, class Excl>
__global__ void __launch_bounds__(ENGINE_THREADS, KCAP <= 16 ? 2 : 1)
knn_search_kernel(const float* __restrict__ X, int64_t N, int64_t ldx, const float* __restrict__ xnorm, typename Excl::Labels xgroup,
                  const float* __restrict__ Y, int64_t M, int64_t ldy, const float* __restrict__ ynorm, typename Excl::Labels ygroup,
                  int D, int nchunks, typename Excl::SelfOffset self_offset, unsigned long long* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LaneInfo L;
    const WorkItem w = work_item((M + TB - 1) / TB, nchunks);
    const int chunk = blockIdx.x % nchunks;            // the chunk work_item gave this workgroup: its slice of `partial`

    KnnListEpilogue<KCAP, Excl> epi(L);
    epi.qnorm = ynorm;
    epi.nq = M;
    epi.aux = lds + ENGINE_LDS_FLOATS;
    if constexpr (Excl::BY_LABEL) epi.qgroup = ygroup;
    else epi.self_lo = self_offset >= 0 ? w.prow0 + self_offset : -2 * TB;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        epi.xn[nt] = row_norm(xnorm, w.prow0, N, L, nt);
        if constexpr (Excl::BY_LABEL) {
            const int64_t i = sweep_row(w.prow0, L, nt);
            epi.xg[nt] = i < N ? xgroup[i] : 0;            // (a row past the end is never stored)
        }
#pragma unroll
        for (int s = 0; s < KCAP; ++s) epi.best[nt][s] = EMPTY_KEY;
    }
    dense_pipeline_early<EV_DEFAULT, KTAIL>(Y, M, ldy, LinearTiles{w.qtile0}, X, N, ldx, w.prow0, w.ntiles, D, lds, L, epi);

    // (its own slot and row arithmetic, one P tile per pass: through join_slot / joined_row of row_sweep.h the register
    // numbers of all six instantiations moved, and the 16-key form has no register to spare)
    // A P row is covered by 4 lists (2 half-waves x 2 Q-half waves): merged through LDS, the rows of one 32-row P tile
    // per wave at a time ([64][4][KCAP] keys: 64 KiB at KCAP = 32, inside the 72 KiB of staging slabs, which are free now)
    unsigned long long* mg = reinterpret_cast<unsigned long long*>(lds);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        if (nt != 0) __syncthreads();                  // the readers of the first pass are done
        unsigned long long* dst = mg + ((L.wn * 32 + L.r) * 4 + (L.wm * 2 + L.h)) * KCAP;
#pragma unroll
        for (int s = 0; s < KCAP; ++s) dst[s] = epi.best[nt][s];
        __syncthreads();
        if (L.tid < 64) {
            const int64_t i = w.prow0 + (L.tid >> 5) * 64 + nt * 32 + (L.tid & 31);
            if (i < N) {
                const unsigned long long* src = mg + L.tid * 4 * KCAP;
                unsigned long long m[KCAP];
#pragma unroll
                for (int s = 0; s < KCAP; ++s) m[s] = src[s];
                for (int s = KCAP; s < 4 * KCAP; ++s) key_insert<KCAP>(m, src[s]);
                unsigned long long* out = partial + ((int64_t)chunk * N + i) * KCAP;
#pragma unroll
                for (int s = 0; s < KCAP; ++s) out[s] = m[s];
            }
        }
    }
}

// the k smallest keys of a row over all chunks -> (distance, column); +inf distance -> column -1
template <int KCAP>
__global__ void __launch_bounds__(256) knn_search_merge_kernel(const unsigned long long* __restrict__ partial, int64_t N, int nchunks,
                                                               int k, int squared, float* __restrict__ out_dist,
                                                               int64_t* __restrict__ out_idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    unsigned long long m[KCAP];
#pragma unroll
    for (int s = 0; s < KCAP; ++s) m[s] = partial[i * KCAP + s];
    for (int c = 1; c < nchunks; ++c) {
        const unsigned long long* src = partial + ((int64_t)c * N + i) * KCAP;
        for (int s = 0; s < KCAP; ++s) key_insert<KCAP>(m, src[s]);
    }
#pragma unroll
    for (int s = 0; s < KCAP; ++s) {
        if (s < k) {
            const unsigned bits = (unsigned)(m[s] >> 32);
            const float d2 = __uint_as_float(bits);
            out_dist[i * k + s] = squared ? d2 : sqrt_rn(d2);
            out_idx[i * k + s] = bits >= INF_BITS ? (int64_t)-1 : (int64_t)(unsigned)m[s];
        }
    }
}

// ---- host side: the shapes a call takes, what its workspace holds, and one call ------------------------------------------
static inline bool shape_ok(int64_t N, int64_t M, int D, int k) { return k >= 1 && k <= MAX_K && sweep_shape_ok(N, M, D, COLUMNS_KEYED); }

struct Buffers {
    float *xn, *yn;
    unsigned long long* partial;
};
static inline void carve(Carver& c, int64_t N, int64_t M, int k, int nchunks, Buffers& b) {
    b.xn = c.take<float>((size_t)N);
    b.yn = c.take<float>((size_t)M);
    b.partial = c.take<unsigned long long>((size_t)nchunks * (size_t)N * kcap_for(k));
}

template <int KCAP, class Excl>
static int run(const float* X, int64_t N, int64_t ldx, const float* xn, typename Excl::Labels x_group, const float* Y, int64_t M,
               int64_t ldy, const float* yn, typename Excl::Labels y_group, int D, int k, int nchunks,
               typename Excl::SelfOffset self_offset, int squared, unsigned long long* partial, float* out_dist, int64_t* out_idx,
               hipStream_t st) {
    const int rc = launch_sweep(&knn_search_kernel<KCAP, false, Excl>, &knn_search_kernel<KCAP, true, Excl>, LDS_BYTES<Excl>, N, nchunks, D,
                                st, X, N, ldx, xn, x_group, Y, M, ldy, yn, y_group, D, nchunks, self_offset, partial);
    if (rc != AM_OK) return rc;
    hipLaunchKernelGGL(knn_search_merge_kernel<KCAP>, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, st, partial, N, nchunks, k, squared,
                       out_dist, out_idx);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

// validate, carve, norms, tile kernel, merge; `query` names the entry's workspace query in the error text
template <class Excl>
static int run_search(const float* X, int64_t N, int64_t ldx, typename Excl::Labels x_group, const float* Y, int64_t M, int64_t ldy,
                      typename Excl::Labels y_group, int D, int k, typename Excl::SelfOffset self_offset, int squared, float* out_dist,
                      int64_t* out_idx, void* ws, size_t ws_bytes, hipStream_t st, const char* query) {
    int rc;
    if ((rc = check_matrix(X, N, ldx, D, "X")) != AM_OK) return rc;
    if ((rc = check_matrix(Y, M, ldy, D, "Y")) != AM_OK) return rc;
    if constexpr (Excl::BY_LABEL)
        AM_REQUIRE(x_group != nullptr && y_group != nullptr, AM_ERR_BAD_ARG, "%s is null", x_group == nullptr ? "x_group" : "y_group");
    AM_REQUIRE(out_dist != nullptr && out_idx != nullptr, AM_ERR_BAD_ARG, "%s is null", out_dist == nullptr ? "out_dist" : "out_idx");
    AM_REQUIRE(k >= 1 && k <= MAX_K, AM_ERR_BAD_SHAPE, "k = %d: the search keeps 1 .. %d neighbours per row", k, MAX_K);
    AM_REQUIRE(shape_ok(N, M, D, k), AM_ERR_BAD_SHAPE, "N=%lld M=%lld: a column index takes 32 bits of a list key (M < 2^32 - 1)",
               (long long)N, (long long)M);
    const int nchunks = choose_chunks(N, M);
    Carver c(ws, ws_bytes);
    Buffers b;
    carve(c, N, M, k, nchunks, b);
    AM_REQUIRE(c.ok(), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (%s), have %zu", c.off, query, ws_bytes);
    // a column past the end excludes nothing; the kernel adds row indices to the offset
    if constexpr (!Excl::BY_LABEL)
        if (self_offset >= M) self_offset = -1;
    const float* yn;
    if ((rc = launch_norms_pair(X, N, ldx, Y, M, ldy, D, b.xn, b.yn, st, &yn)) != AM_OK) return rc;
    switch (kcap_for(k)) {
        case 8:  return run<8, Excl>(X, N, ldx, b.xn, x_group, Y, M, ldy, yn, y_group, D, k, nchunks, self_offset, squared, b.partial, out_dist, out_idx, st);
        case 16: return run<16, Excl>(X, N, ldx, b.xn, x_group, Y, M, ldy, yn, y_group, D, k, nchunks, self_offset, squared, b.partial, out_dist, out_idx, st);
        default: return run<32, Excl>(X, N, ldx, b.xn, x_group, Y, M, ldy, yn, y_group, D, k, nchunks, self_offset, squared, b.partial, out_dist, out_idx, st);
    }
}

}  // namespace search
}  // namespace am

using namespace am;

extern "C" size_t am_knn_search_workspace_bytes(int64_t N, int64_t M, int D, int k) {
    if (!search::shape_ok(N, M, D, k)) return 0;
    Carver c(nullptr, 0);
    search::Buffers b;
    search::carve(c, N, M, k, choose_chunks(N, M), b);
    return c.off;
}

// the labels are the caller's: nothing more to hold
extern "C" size_t am_knn_search_groups_workspace_bytes(int64_t N, int64_t M, int D, int k) { return am_knn_search_workspace_bytes(N, M, D, k); }

extern "C" int am_knn_search_chunks(int64_t N, int64_t M, int D, int k) {
    return search::shape_ok(N, M, D, k) ? choose_chunks(N, M) : 0;
}

extern "C" int am_knn_search_f32(const float* X, int64_t N, int64_t ldx, const float* Y, int64_t M, int64_t ldy, int D, int k,
                                 int64_t self_offset, int squared, float* out_dist, int64_t* out_idx, void* ws, size_t ws_bytes,
                                 am_stream_t stream) {
    return search::run_search<search::ByIndex>(X, N, ldx, {}, Y, M, ldy, {}, D, k, self_offset, squared, out_dist, out_idx, ws, ws_bytes,
                                               static_cast<hipStream_t>(stream), "am_knn_search_workspace_bytes");
}

extern "C" int am_knn_search_groups_f32(const float* X, int64_t N, int64_t ldx, const int32_t* x_group, const float* Y, int64_t M,
                                        int64_t ldy, const int32_t* y_group, int D, int k, int squared, float* out_dist,
                                        int64_t* out_idx, void* ws, size_t ws_bytes, am_stream_t stream) {
    return search::run_search<search::ByLabel>(X, N, ldx, x_group, Y, M, ldy, y_group, D, k, {}, squared, out_dist, out_idx, ws, ws_bytes,
                                               static_cast<hipStream_t>(stream), "am_knn_search_groups_workspace_bytes");
}
