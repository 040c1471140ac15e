// Per-sample fidelity on the PRDC manifold: for every row of X (the samples) its REALISM, the number of reference balls it
// lies in and its RARITY, against the rows of Y (the manifold set) and their k-NN radii r_j, without an N x M matrix.
//     realism_i = max_j r_j / |x_i - y_j|                 (Kynkaanniemi et al. 2019; >= 1: inside some ball)
//     count_i   = #{ j : x_i inside ball j }             (the column counts of am_prdc_counts_f32, bit for bit)
//     rarity_i  = min { r_j : x_i inside ball j }         (Han et al. 2023; 0 for a row outside every ball)
//
// A fourth epilogue on the exact f32 128 x 128 tile engine, beside the radii (pairwise.hip), the search (knn_search.hip) and
// the k-means assign (kmeans.hip): dense_pipeline_early with the production schedule, the (row block) x (column chunk) plan
// of work_item / choose_chunks, the KTAIL instantiation for D % 32 != 0, and the arithmetic of a pair
//     d2 = max(fmaf(-2, <x, y>, |x|^2 + |y|^2), 0)       NaN -> +inf (clamp0); a padded column has |y|^2 = +inf
// with the f32 norms of launch_norms: the bits of am_knn_search_f32(squared) and of the exact PRDC kernel.
//
// A column brings three floats per tile through LDS: |y_j|^2, the membership threshold and the radius.  A pre-kernel
// (scores_columns_kernel) cleans the radii - one that is not > 0 (zero, negative, NaN) becomes 0: nobody's ball, ratio 0 -
// and computes T(r_j) = threshold_of_radius (pairwise_common.h) once per column, so that
//     member  <=>  d2 < T(r_j)  <=>  sqrt_rn(d2) < r_j       the strict test of the exact PRDC kernel.
// The tile kernel tests the UNCLAMPED value u against T' = (T > 0 ? T : -inf):  max(u, 0) < T <=> u < T for T > 0 (a
// negative u clamps to 0 < T), nothing is below -inf, and a NaN loses the compare as +inf does.
//
// Ratio of a pair: q = fdiv_rn(fmul_rn(r_j, r_j), d2), correctly rounded; NaN (0 / 0, inf / inf) counts as 0; d2 == 0 with
// r_j > 0 gives +inf.  realism = sqrt_rn(max_j q).
//
// What a lane keeps per row: ONE max key, ONE min key, one int32.
//     max key = (uint64)bits(q)   << 32 | (0xffffffff - column)      q >= 0: floats order like their bits
//     min key = (uint64)bits(r_j) << 32 | column                     over the members only
// so ties - equal ratios, equal radii - go to the SMALLEST column whatever the chunking, the tile order or the lane.
// The count is one compare and one add per pair.  The min key is formed only for a 32 x 32 tile in which some lane's
// count moved.  The division runs behind a gate: with B the lane's best ratio so far,
//     q >= B  =>  r^2 / d2 >= B (1 - 2^-24)  =>  fma(-B', u, r^2) >= 0,   B' = B (1 - 2^-20) rounded  (<= B (1 - 2^-24))
// (the fma's sign is that of the exact value: rounding never crosses zero; a negative u passes; NaN fails, and its ratio
// is 0).  B = +inf takes B' = FLT_MAX so that d2 = 0 still passes (inf * 0 would be NaN); B below 2^-100, where a rounded
// ratio may be subnormal and the relative bound does not hold, takes B' = 0 - then every pair with r^2 > 0 passes.  While
// B' = 0 the test is strict (r^2 > 0): a ratio of 0 is "no reference row" and needs no key.  The gate is the maximum of
// that fma over the sixteen values of an accumulator tile, __any over the wave; past it the same test selects the lanes
// that divide.  B is frozen per tile: a superset, and the key compare decides.  The reported bits are those of the
// ungated definition.
//
// The four keys and counts of a row (2 half-waves x 2 column-half waves) meet in LDS, the chunks' partials
// ([nchunks][N] max keys, min keys, counts) in sample_scores_merge_kernel: max / min / sum, no floating-point atomics, the
// same bits on every call.
//
// Which pairs count is a POLICY (AllPairs, OtherLabels below): what the kernel is handed, what the epilogue keeps for it,
// and two places of `finish`.  Everything else - the epilogue, the tile kernel with its join, the column and merge
// kernels, the entry's validation, workspace and norms - exists once.
//
// Register budget: 64 accumulators, 64 staging registers, 32 fragment registers, 8 key registers and 2 counts, with
// OtherLabels two label registers more; __launch_bounds__(256, 2), two workgroups per CU (2 x 75 KiB of LDS, 2 x 76 KiB
// with the labels), no scratch in either policy (tests/test_sample_scores_resources_cpu.py).
#include "row_sweep.h"

namespace am {
namespace scores {

constexpr unsigned long long NO_MEMBER = 0xffffffffffffffffull;          // min key of a row outside every ball
constexpr int MERGE_THREADS = 256;
constexpr float GATE_SHRINK = 1.f - 9.5367431640625e-07f;                // 1 - 2^-20
constexpr float GATE_TINY = 7.888609052210118e-31f;                      // 2^-100
constexpr float F32_MAX = 3.4028234663852886e+38f;
constexpr float F32_MIN_NORMAL = 1.1754943508222875e-38f;

// ---- exclusion policies ----------------------------------------------------------------------------------------------------
// A policy names the types of what only it needs - Labels: the label array of a side, as the kernel is handed it; Label: one
// row's label in a register - and gives them the type Absent (row_sweep.h), which takes no room, where it needs none.  The
// kernel and the epilogue list them in their places, the label array of a side behind its float arrays, the label registers
// behind the norm registers: the kernarg offsets and the order of the epilogue's members are part of the program (the
// policies of knn_search.hip; profiles/exclusion_policy/isa_compare.txt).  ARRAYS: the per-column arrays a tile brings
// through LDS, [2][ARRAYS][128]: |y_j|^2, T'(r_j), r_j and, fourth, the label's bits.

// every pair counts
struct AllPairs {
    static constexpr bool BY_LABEL = false;
    static constexpr int ARRAYS = 3;
    using Labels = Absent;
    using Label = Absent;
};

// A whole GROUP left out: one int32 label per row of X and per row of Y, and a pair (i, j) with x_group[i] == y_group[j] is
// no pair: it is not counted, its ratio is 0, it is no candidate of the rarity.
//     realism_i = max { r_j / |x_i - y_j| : label_j != label_i }
//     count_i   = #{ j : label_j != label_i, x_i inside ball j }
//     rarity_i  = min { r_j : label_j != label_i, x_i inside ball j }
// The embedding pipeline cuts every file into windows, so a window lies inside the balls of its own song's windows whatever
// the model did; with leave-group-out radii alone (knn_search.hip, by label) those balls even grow.  Only a membership pass
// that knows the labels scores a window against the OTHER songs.
//
// Labels.  The column labels travel as a fourth [128] array beside |y_j|^2, T'(r_j) and r_j through LDS, staged by hand
// because the array is not float: a label is only moved and compared for equality, never computed with.  A lane keeps the
// labels of its two rows in two registers.
//
// Gates.  The dense loop does not know about the exclusion: cnt += u < T' over ALL columns, and the division gate's fma /
// max.  Both gates are supersets of what the labels leave, which costs time and never a result, because the exclusion is
// applied where a result is made:
//   - in the path that runs only when some lane's count moved in the 32 x 32 sub-tile, a member whose label equals the
//     row's takes 1 off the count again instead of making a min key (the count went up by exactly 1 for it: same test,
//     same bits);
//   - in the gated division path a same-label column makes no max key.  B, the lane's best ratio, is only ever raised by
//     admissible keys, so the gate's bound keeps its meaning.
struct OtherLabels {
    static constexpr bool BY_LABEL = true;
    static constexpr int ARRAYS = 4;
    using Labels = const int32_t* __restrict__;
    using Label = int32_t;
};

template <class Excl>
constexpr size_t LDS_BYTES = (ENGINE_LDS_FLOATS + 2 * Excl::ARRAYS * TB) * sizeof(float);   // staging slabs + [2][ARRAYS][128] column values
static_assert(2 * LDS_BYTES<AllPairs> <= 160 * 1024 && 2 * LDS_BYTES<OtherLabels> <= 160 * 1024, "two workgroups share the 160 KiB LDS of a CU");

// cleaned radius (0 for one that is not > 0) and the threshold the tile kernel compares the unclamped d2 with
__global__ void scores_columns_kernel(const float* __restrict__ r_y, int64_t M, float* __restrict__ rad, float* __restrict__ thr) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    const float r0 = r_y[j];
    const float r = r0 > 0.f ? r0 : 0.f;
    const float T = threshold_of_radius(r);
    rad[j] = r;
    thr[j] = T > 0.f ? T : -INFINITY;
}

template <class Excl>
struct ScoresEpilogue {
    static constexpr int K = Excl::ARRAYS;
    const float* ynorm;
    const float* ythr;
    const float* yrad;
    typename Excl::Labels ygroup;
    int64_t nc;
    float* aux;                          // LDS [2][K][128] : |y_j|^2 (+inf past nc), T'(r_j) (-inf past nc), r_j (0 past nc), label bits
    float xn[2];
    typename Excl::Label xg[2];          // the labels of the lane's two rows
    unsigned long long kmax[2], kmin[2];
    int cnt[2];
    float aux_n, aux_t, aux_r;
    typename Excl::Label aux_g;
    const LaneInfo& L;

    __device__ __forceinline__ ScoresEpilogue(const LaneInfo& l) : L(l) {}
    __device__ __forceinline__ void aux_issue(int, int64_t qtile) {
        if (L.tid < TB) {
            const int64_t j = qtile * TB + L.tid;
            aux_n = j < nc ? ynorm[j] : INFINITY;
            aux_t = j < nc ? ythr[j] : -INFINITY;
            aux_r = j < nc ? yrad[j] : 0.f;
            if constexpr (Excl::BY_LABEL) aux_g = j < nc ? ygroup[j] : 0;     // never decides: such a column is no member and its ratio is 0
        }
    }
    __device__ __forceinline__ void aux_commit(int t) {
        if (L.tid < TB) {
            float* dst = aux + (t & 1) * K * TB + L.tid;
            dst[0] = aux_n;
            dst[TB] = aux_t;
            dst[2 * TB] = aux_r;
            if constexpr (Excl::BY_LABEL) reinterpret_cast<int32_t*>(dst)[3 * TB] = aux_g;
        }
    }

    __device__ __forceinline__ void finish(int t, int64_t qtile, f32x16 (&acc)[2][2]) {
        const float* a = aux + (t & 1) * K * TB + L.wm * 64 + L.h * 4;
        const int32_t* g = reinterpret_cast<const int32_t*>(a + 3 * TB);          // OtherLabels: the labels of the lane's columns
        const unsigned cbase = (unsigned)(qtile * TB + L.wm * 64 + L.h * 4);      // the lane's first column of the tile
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            // the gate's factor -B' and its limit (t > limit passes): frozen for this accumulator tile
            float nb[2], lim[2], tmax[2];
            int c0[2];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const float best = __uint_as_float((unsigned)(kmax[nt] >> 32));
                const float bs = best < GATE_TINY ? 0.f : (best > F32_MAX ? F32_MAX : best * GATE_SHRINK);
                nb[nt] = -bs;
                lim[nt] = bs > 0.f ? -F32_MIN_NORMAL : 0.f;
                tmax[nt] = -INFINITY;
                c0[nt] = cnt[nt];
            }
            // the dense loop: all columns, under OtherLabels the row's own group included
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const f32x4 yn = *reinterpret_cast<const f32x4*>(a + mt * 32 + g4 * 8);
                const f32x4 tp = *reinterpret_cast<const f32x4*>(a + TB + mt * 32 + g4 * 8);
                const f32x4 rr = *reinterpret_cast<const f32x4*>(a + 2 * TB + mt * 32 + g4 * 8);
                f32x4 r2;
#pragma unroll
                for (int e = 0; e < 4; ++e) r2[e] = __fmul_rn(rr[e], rr[e]);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float u = fmaf(-2.f, acc[mt][nt][g4 * 4 + e], xn[nt] + yn[e]);
                        cnt[nt] += u < tp[e] ? 1 : 0;
                        tmax[nt] = fmaxf(tmax[nt], fmaf(nb[nt], u, r2[e]));      // a NaN is dropped: its ratio is 0
                    }
                }
            }
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                // common case after warm-up: no lane of the wave can raise its ratio with this 32 x 32 tile
                if (__any(tmax[nt] > lim[nt])) {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int rel = mt * 32 + (reg & 3) + 8 * (reg >> 2);
                        const float u = fmaf(-2.f, acc[mt][nt][reg], xn[nt] + a[rel]);
                        const float r = a[2 * TB + rel];
                        const float r2 = __fmul_rn(r, r);
                        bool pair = fmaf(nb[nt], u, r2) > lim[nt];
                        if constexpr (Excl::BY_LABEL) pair = pair && g[rel] != xg[nt];      // the row's own group: by label, no key
                        if (pair) {
                            const float q0 = __fdiv_rn(r2, clamp0(u));
                            const float q = q0 != q0 ? 0.f : q0;
                            const unsigned long long key =
                                ((unsigned long long)__float_as_uint(q) << 32) | (0xffffffffu - (cbase + (unsigned)rel));
                            kmax[nt] = key > kmax[nt] ? key : kmax[nt];
                        }
                    }
                }
                // rare: k N inside-pairs among N M, of the own group or not
                if (__any(cnt[nt] != c0[nt])) {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int rel = mt * 32 + (reg & 3) + 8 * (reg >> 2);
                        const float u = fmaf(-2.f, acc[mt][nt][reg], xn[nt] + a[rel]);
                        if (u < a[TB + rel]) {
                            bool own = false;
                            if constexpr (Excl::BY_LABEL) own = g[rel] == xg[nt];
                            if (own) {
                                cnt[nt] -= 1;                                    // counted by the dense loop: taken off again
                            } else {
                                const unsigned long long key =
                                    ((unsigned long long)__float_as_uint(a[2 * TB + rel]) << 32) | (cbase + (unsigned)rel);
                                kmin[nt] = key < kmin[nt] ? key : kmin[nt];
                            }
                        }
                    }
                }
            }
        }
    }
};

// pmax / pmin / pcnt [chunk * N + row] = the row's keys and count inside column chunk `chunk`
template <bool KTAIL, class Excl>
__global__ void __launch_bounds__(ENGINE_THREADS, 2)
sample_scores_kernel(const float* __restrict__ X, int64_t N, int64_t ldx, const float* __restrict__ xnorm, typename Excl::Labels xgroup,
                     const float* __restrict__ Y, int64_t M, int64_t ldy, const float* __restrict__ ynorm,
                     const float* __restrict__ ythr, const float* __restrict__ yrad, typename Excl::Labels ygroup, int D, int nchunks,
                     unsigned long long* __restrict__ pmax, unsigned long long* __restrict__ pmin, int* __restrict__ pcnt) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LaneInfo L;
    const WorkItem w = work_item((M + TB - 1) / TB, nchunks);
    const int chunk = blockIdx.x % nchunks;            // the chunk work_item gave this workgroup: its slice of the partials

    ScoresEpilogue<Excl> epi(L);
    epi.ynorm = ynorm;
    epi.ythr = ythr;
    epi.yrad = yrad;
    if constexpr (Excl::BY_LABEL) epi.ygroup = ygroup;
    epi.nc = M;
    epi.aux = lds + ENGINE_LDS_FLOATS;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        epi.xn[nt] = row_norm(xnorm, w.prow0, N, L, nt);
        if constexpr (Excl::BY_LABEL) {
            const int64_t i = sweep_row(w.prow0, L, nt);
            epi.xg[nt] = i < N ? xgroup[i] : 0;            // (a row past the end is never stored)
        }
        epi.kmax[nt] = 0ull;
        epi.kmin[nt] = NO_MEMBER;
        epi.cnt[nt] = 0;
    }
    dense_pipeline_early<EV_DEFAULT, KTAIL>(Y, M, ldy, LinearTiles{w.qtile0}, X, N, ldx, w.prow0, w.ntiles, D, lds, L, epi);

    // a row is covered by 4 lanes (2 half-waves x 2 column-half waves): [128][4] max keys, min keys and counts through the
    // staging slabs, free now
    unsigned long long* mgmax = reinterpret_cast<unsigned long long*>(lds);
    unsigned long long* mgmin = mgmax + TB * 4;
    int* mgcnt = reinterpret_cast<int*>(mgmin + TB * 4);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int slot = join_slot(L, nt);
        mgmax[slot] = epi.kmax[nt];
        mgmin[slot] = epi.kmin[nt];
        mgcnt[slot] = epi.cnt[nt];
    }
    __syncthreads();
    if (L.tid < TB) {
        const int64_t i = joined_row(w.prow0, L.tid);
        if (i < N) {
            unsigned long long hi = mgmax[L.tid * 4], lo = mgmin[L.tid * 4];
            int c = mgcnt[L.tid * 4];
#pragma unroll
            for (int s = 1; s < 4; ++s) {
                const unsigned long long a = mgmax[L.tid * 4 + s], b = mgmin[L.tid * 4 + s];
                hi = a > hi ? a : hi;
                lo = b < lo ? b : lo;
                c += mgcnt[L.tid * 4 + s];
            }
            pmax[(int64_t)chunk * N + i] = hi;
            pmin[(int64_t)chunk * N + i] = lo;
            pcnt[(int64_t)chunk * N + i] = c;
        }
    }
}

// max / min / sum of a row's partials over all chunks -> the five outputs
__global__ void __launch_bounds__(MERGE_THREADS)
sample_scores_merge_kernel(const unsigned long long* __restrict__ pmax, const unsigned long long* __restrict__ pmin,
                           const int* __restrict__ pcnt, int64_t N, int nchunks, float* __restrict__ out_realism,
                           int64_t* __restrict__ out_realism_idx, int32_t* __restrict__ out_count, float* __restrict__ out_rarity,
                           int64_t* __restrict__ out_rarity_idx) {
    const int64_t i = (int64_t)blockIdx.x * MERGE_THREADS + threadIdx.x;
    if (i >= N) return;
    unsigned long long hi = pmax[i], lo = pmin[i];
    int c = pcnt[i];
    for (int ch = 1; ch < nchunks; ++ch) {
        const unsigned long long a = pmax[(int64_t)ch * N + i], b = pmin[(int64_t)ch * N + i];
        hi = a > hi ? a : hi;
        lo = b < lo ? b : lo;
        c += pcnt[(int64_t)ch * N + i];
    }
    const unsigned qbits = (unsigned)(hi >> 32);
    out_realism[i] = sqrt_rn(__uint_as_float(qbits));
    out_realism_idx[i] = qbits == 0u ? (int64_t)-1 : (int64_t)(0xffffffffu - (unsigned)hi);
    out_count[i] = c;
    const bool member = lo != NO_MEMBER;
    out_rarity[i] = member ? __uint_as_float((unsigned)(lo >> 32)) : 0.f;
    out_rarity_idx[i] = member ? (int64_t)(unsigned)lo : (int64_t)-1;
}

// ---- host side: the shapes a call takes, what its workspace holds, and one call ------------------------------------------
static inline bool shape_ok(int64_t N, int64_t M, int D) { return sweep_shape_ok(N, M, D, COLUMNS_KEYED); }

struct Buffers {
    float *xn, *yn, *thr, *rad;
    unsigned long long *pmax, *pmin;
    int* pcnt;
};
static inline void carve(Carver& c, int64_t N, int64_t M, int nchunks, Buffers& b) {
    b.xn = c.take<float>((size_t)N);
    b.yn = c.take<float>((size_t)M);
    b.thr = c.take<float>((size_t)M);
    b.rad = c.take<float>((size_t)M);
    b.pmax = c.take<unsigned long long>((size_t)nchunks * (size_t)N);
    b.pmin = c.take<unsigned long long>((size_t)nchunks * (size_t)N);
    b.pcnt = c.take<int>((size_t)nchunks * (size_t)N);
}

static int launch_columns(const float* r_y, int64_t M, float* rad, float* thr, hipStream_t st) {
    hipLaunchKernelGGL(scores_columns_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, st, r_y, M, rad, thr);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

static int launch_merge(const unsigned long long* pmax, const unsigned long long* pmin, const int* pcnt, int64_t N, int nchunks,
                        float* out_realism, int64_t* out_realism_idx, int32_t* out_count, float* out_rarity, int64_t* out_rarity_idx,
                        hipStream_t st) {
    hipLaunchKernelGGL(sample_scores_merge_kernel, dim3((unsigned)ceil_div(N, MERGE_THREADS)), dim3(MERGE_THREADS), 0, st, pmax, pmin,
                       pcnt, N, nchunks, out_realism, out_realism_idx, out_count, out_rarity, out_rarity_idx);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

// validate, carve, norms, columns, tile kernel, merge; `query` names the entry's workspace query in the error text
template <class Excl>
static int run_scores(const float* X, int64_t N, int64_t ldx, typename Excl::Labels x_group, const float* Y, int64_t M, int64_t ldy,
                      typename Excl::Labels y_group, int D, const float* r_y, float* out_realism, int64_t* out_realism_idx,
                      int32_t* out_count, float* out_rarity, int64_t* out_rarity_idx, void* ws, size_t ws_bytes, hipStream_t st,
                      const char* query) {
    int rc;
    if ((rc = check_matrix(X, N, ldx, D, "X")) != AM_OK) return rc;
    if ((rc = check_matrix(Y, M, ldy, D, "Y")) != AM_OK) return rc;
    if constexpr (Excl::BY_LABEL)
        AM_REQUIRE(x_group != nullptr && y_group != nullptr, AM_ERR_BAD_ARG, "%s is null", x_group == nullptr ? "x_group" : "y_group");
    AM_REQUIRE(r_y != nullptr && out_realism != nullptr && out_realism_idx != nullptr && out_count != nullptr &&
                   out_rarity != nullptr && out_rarity_idx != nullptr,
               AM_ERR_BAD_ARG, "%s is null",
               r_y == nullptr ? "r_y" : out_realism == nullptr ? "out_realism" : out_realism_idx == nullptr ? "out_realism_idx"
               : out_count == nullptr ? "out_count" : out_rarity == nullptr ? "out_rarity" : "out_rarity_idx");
    AM_REQUIRE(shape_ok(N, M, D), AM_ERR_BAD_SHAPE, "N=%lld M=%lld: a column index takes 32 bits of a key (M < 2^32 - 1)",
               (long long)N, (long long)M);
    const int nchunks = choose_chunks(N, M);
    Carver c(ws, ws_bytes);
    Buffers b;
    carve(c, N, M, nchunks, b);
    AM_REQUIRE(c.ok(), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (%s), have %zu", c.off, query, ws_bytes);
    const float* yn;
    if ((rc = launch_norms_pair(X, N, ldx, Y, M, ldy, D, b.xn, b.yn, st, &yn)) != AM_OK) return rc;
    if ((rc = launch_columns(r_y, M, b.rad, b.thr, st)) != AM_OK) return rc;
    rc = launch_sweep(&sample_scores_kernel<false, Excl>, &sample_scores_kernel<true, Excl>, LDS_BYTES<Excl>, N, nchunks, D, st, X, N, ldx,
                      b.xn, x_group, Y, M, ldy, yn, b.thr, b.rad, y_group, D, nchunks, b.pmax, b.pmin, b.pcnt);
    if (rc != AM_OK) return rc;
    return launch_merge(b.pmax, b.pmin, b.pcnt, N, nchunks, out_realism, out_realism_idx, out_count, out_rarity, out_rarity_idx, st);
}

}  // namespace scores
}  // namespace am

using namespace am;

extern "C" size_t am_sample_scores_workspace_bytes(int64_t N, int64_t M, int D) {
    if (!scores::shape_ok(N, M, D)) return 0;
    Carver c(nullptr, 0);
    scores::Buffers b;
    scores::carve(c, N, M, choose_chunks(N, M), b);
    return c.off;
}

// the labels are the caller's: nothing more to hold
extern "C" size_t am_sample_scores_groups_workspace_bytes(int64_t N, int64_t M, int D) { return am_sample_scores_workspace_bytes(N, M, D); }

extern "C" int am_sample_scores_chunks(int64_t N, int64_t M, int D) {
    return scores::shape_ok(N, M, D) ? choose_chunks(N, M) : 0;
}

extern "C" int am_sample_scores_f32(const float* X, int64_t N, int64_t ldx, const float* Y, int64_t M, int64_t ldy, int D,
                                    const float* r_y, float* out_realism, int64_t* out_realism_idx, int32_t* out_count,
                                    float* out_rarity, int64_t* out_rarity_idx, void* ws, size_t ws_bytes, am_stream_t stream) {
    return scores::run_scores<scores::AllPairs>(X, N, ldx, {}, Y, M, ldy, {}, D, r_y, out_realism, out_realism_idx, out_count, out_rarity,
                                                out_rarity_idx, ws, ws_bytes, static_cast<hipStream_t>(stream),
                                                "am_sample_scores_workspace_bytes");
}

extern "C" int am_sample_scores_groups_f32(const float* X, int64_t N, int64_t ldx, const int32_t* x_group, const float* Y, int64_t M,
                                           int64_t ldy, const int32_t* y_group, int D, const float* r_y, float* out_realism,
                                           int64_t* out_realism_idx, int32_t* out_count, float* out_rarity, int64_t* out_rarity_idx,
                                           void* ws, size_t ws_bytes, am_stream_t stream) {
    return scores::run_scores<scores::OtherLabels>(X, N, ldx, x_group, Y, M, ldy, y_group, D, r_y, out_realism, out_realism_idx, out_count,
                                                   out_rarity, out_rarity_idx, ws, ws_bytes, static_cast<hipStream_t>(stream),
                                                   "am_sample_scores_groups_workspace_bytes");
}
