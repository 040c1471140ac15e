// Retrieval ranks of paired sets: at which rank does a query row find its own gallery rows among all M of them?  For every
// row of Q (the queries, N rows) against the rows of G (the gallery, M rows), without an N x M matrix: the exact rank of the
// row's best POSITIVE column, as two integer counts - what R@k, median rank, MRR and mAP@10 of the text-to-audio and
// audio-captioning tables are made of (metrics/retrieval.py).
//
// Definitions.  Inputs: Q [N, D], G [M, D] float32; a list of positive gallery rows per query row, P_i = pos_columns[
// pos_start[i] .. pos_start[i] + pos_count[i]) (distinct columns; rows with one label share a segment); the similarity,
// cosine or dot; optionally one int32 group id per row of either side (the song).
//     u_ij = fmul_rn(a_ij, w_j)                    the score of a pair
//     a_ij = <q_i, g_j> with the bits of the 128 x 128 f32 tile engine: the fmaf chain over the index order
//            8c+0, 8c+4, 8c+1, 8c+5, 8c+2, 8c+6, 8c+3, 8c+7 (tile_engine.h), from +0
//     w_j  = 1 for dot; fdiv_rn(1, sqrt_rn(|g_j|^2)) for cosine, |g_j|^2 from launch_norms; correctly rounded operations only
// The query's own norm changes no order inside its row and is not applied in the sweep.  A pair whose u is NaN HAS NO SCORE
// (a zero-norm gallery row under cosine: 0 * inf; a row with a non-finite element): it is never a positive, never counted.
// Per query row i:
//     t_i        = max { u_ij : j in P_i, u_ij scored };  positive_i = the smallest such column that reaches it
//     unranked     a row with no scored positive (or a malformed segment, below): better = tied = -1, positive = -1, score = NaN
//     negatives    the columns that are not in P_i and, with group ids, whose group differs from the row's own
//     better_i   = #{ negatives j : u_ij >  t_i }      IEEE float compares, int32
//     tied_i     = #{ negatives j : u_ij == t_i }
//     score_i    = t_i for dot; fmul_rn(t_i, w_i^Q) for cosine (w^Q from the query norms): the cosine itself
//     rank_i     = 1 + better_i: the optimistic convention, the (sims > diag).sum(1) of the public retrieval code; tied_i is
//                  reported so that nobody has to trust the convention
//     n_pos_i    = the entries of the row's segment that name a column in [0, M); n_pos_own_group_i = those of them in the
//                  row's own group (0 without groups)
// A segment that leaves pos_columns, or an entry outside [0, M), is never dereferenced: the row comes out unranked.
//
// Three steps.
//   1. retrieval_weights_kernel: w_j from the norms (all ones for dot); the same kernel makes w_i^Q.
//   2. retrieval_positives_kernel: one thread per query row evaluates its few positive pairs directly - the scalar fmaf
//      chain in the engine's index order (wave_pair_dot of pairwise_fast.h, oracle/exact_c/pairwise_exact.c), so that t_i
//      has the BITS of the tile engine: the sweep compares its accumulators with t_i for equality.  N |P| D flops; simple,
//      not fast.  It also counts the positives at the maximum that the sweep will count as tied (those whose group differs
//      from the row's, or all of them without groups).
//   3. retrieval_kernel, a ninth epilogue on the exact f32 tile engine (row_sweep.h): dense_pipeline_early with the
//      production schedule, the (row block) x (column chunk) plan of work_item / choose_chunks, the KTAIL instantiation.  A
//      lane keeps t_i and two int32 counts for each of its two rows; a tile brings w_j through LDS - NaN past the end, so
//      that a padded column has no score whatever the sign of t_i - and with groups the label bits as a second array,
//      staged by hand.  `finish` is dense - one multiply, two compares, two adds per pair, under the group policy one label
//      compare ANDed in - and knows nothing about positives: a positive can never be > t_i, and the tied positives are
//      taken off afterwards with the number from step 2.  (No "rare path": a badly ranked row has counts moving in every
//      tile.)  The four lanes of a row meet through join_slot / joined_row; partials are [nchunks][N] int32 x 2;
//      retrieval_merge_kernel adds the chunks in chunk order, subtracts the tied positives and writes the outputs.
// No atomics of any kind: two calls give the same bits, whatever the chunk plan (integer sums).
//
// Register budget: 64 accumulators, 64 staging registers, 32 fragment registers, 2 thresholds, 4 counts, with groups two
// label registers; __launch_bounds__(256, 2), two workgroups per CU, no scratch (tests/test_retrieval_resources_cpu.py).
#include "row_sweep.h"

namespace am {
namespace retrieval {

constexpr int SIDE_THREADS = 256;        // the weight, positives and merge kernels

// ---- which columns can be negatives ------------------------------------------------------------------------------------------
// As the policies of knn_search.hip and sample_scores.hip: a policy names the types of what only it needs and gives them the
// type Absent (row_sweep.h) where it needs none.  ARRAYS: the per-column arrays a tile brings through LDS, [2][ARRAYS][128]:
// w_j and, second, the group's bits.
struct AllColumns {
    static constexpr bool BY_GROUP = false;
    static constexpr int ARRAYS = 1;
    using Labels = Absent;
    using Label = Absent;
};

// the row's own group (its song: the windows next to it) is no negative
struct OtherGroups {
    static constexpr bool BY_GROUP = true;
    static constexpr int ARRAYS = 2;
    using Labels = const int32_t* __restrict__;
    using Label = int32_t;
};

template <class Excl>
constexpr size_t LDS_BYTES = (ENGINE_LDS_FLOATS + 2 * Excl::ARRAYS * TB) * sizeof(float);   // staging slabs + [2][ARRAYS][128] column values
static_assert(2 * LDS_BYTES<AllColumns> <= 160 * 1024 && 2 * LDS_BYTES<OtherGroups> <= 160 * 1024, "two workgroups share the 160 KiB LDS of a CU");

// ---- step 1: w = 1 / sqrt(|row|^2), correctly rounded; 1 for dot -----------------------------------------------------------------
__global__ void __launch_bounds__(SIDE_THREADS)
retrieval_weights_kernel(const float* __restrict__ norm, int64_t n, int cosine, float* __restrict__ w) {
    const int64_t j = (int64_t)blockIdx.x * SIDE_THREADS + threadIdx.x;
    if (j >= n) return;
    w[j] = cosine ? __fdiv_rn(1.f, sqrt_rn(norm[j])) : 1.f;
}

// <q, g> with the bits of the tile engine: the fmaf chain over 8c+0, 8c+4, 8c+1, 8c+5, ... from +0, the inner-dimension tail
// padded with zeros as the engine's slabs are
__device__ __forceinline__ float engine_dot(const float* __restrict__ q, const float* __restrict__ g, int D) {
    float acc = 0.f;
    for (int c = 0; c < D; c += 8) {
        const f32x4 q0 = load_k4(q, c, D), q1 = load_k4(q, c + 4, D);
        const f32x4 g0 = load_k4(g, c, D), g1 = load_k4(g, c + 4, D);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            acc = fmaf(g0[s], q0[s], acc);
            acc = fmaf(g1[s], q1[s], acc);
        }
    }
    if ((D % BK) != 0) acc = fmaf(0.f, 0.f, acc);          // the zero steps up to the slab's end (they only turn -0 into +0)
    return acc;
}

// ---- step 2: the positives of a row, one thread per row ---------------------------------------------------------------------------
// thr[i] = t_i (NaN: unranked), tied_pos[i] = the positives at t_i that the sweep counts; the four per-row outputs that need
// no sweep are written here
__global__ void __launch_bounds__(SIDE_THREADS)
retrieval_positives_kernel(const float* __restrict__ Q, int64_t N, int64_t ldq, const float* __restrict__ G, int64_t M, int64_t ldg,
                           int D, int cosine, const float* __restrict__ wq, const float* __restrict__ wg,
                           const int64_t* __restrict__ pos_start, const int64_t* __restrict__ pos_count,
                           const int64_t* __restrict__ pos_columns, int64_t n_pos_columns, const int32_t* __restrict__ q_group,
                           const int32_t* __restrict__ g_group, float* __restrict__ thr, int32_t* __restrict__ tied_pos,
                           float* __restrict__ out_score, int64_t* __restrict__ out_positive, int32_t* __restrict__ out_n_pos,
                           int32_t* __restrict__ out_n_pos_own_group) {
    const int64_t i = (int64_t)blockIdx.x * SIDE_THREADS + threadIdx.x;
    if (i >= N) return;
    const int64_t s = pos_start[i], c = pos_count[i];
    const bool segment_ok = s >= 0 && c >= 0 && s <= n_pos_columns && c <= n_pos_columns - s;
    const bool by_group = q_group != nullptr;
    const int32_t own = by_group ? q_group[i] : 0;
    const float* q = Q + i * ldq;
    float t = -INFINITY;
    int64_t best = -1;
    int32_t n_pos = 0, n_own = 0, n_tied = 0;
    bool valid = segment_ok;
    for (int64_t e = 0; segment_ok && e < c; ++e) {
        const int64_t j = pos_columns[s + e];
        if (j < 0 || j >= M) {               // never dereferenced: the row is unranked
            valid = false;
            continue;
        }
        n_pos += 1;
        const bool same_group = by_group && g_group[j] == own;
        n_own += same_group ? 1 : 0;
        const float u = __fmul_rn(engine_dot(q, G + j * ldg, D), wg[j]);
        if (u != u) continue;                // no score: no positive
        if (best < 0 || u > t) {
            t = u;
            best = j;
            n_tied = same_group ? 0 : 1;
        } else if (u == t) {
            best = j < best ? j : best;
            n_tied += same_group ? 0 : 1;
        }
    }
    const bool ranked = valid && best >= 0;
    thr[i] = ranked ? t : __builtin_nanf("");
    tied_pos[i] = ranked ? n_tied : 0;
    out_score[i] = ranked ? (cosine ? __fmul_rn(t, wq[i]) : t) : __builtin_nanf("");
    out_positive[i] = ranked ? best : (int64_t)-1;
    out_n_pos[i] = n_pos;
    out_n_pos_own_group[i] = n_own;
}

// ---- step 3: the sweep --------------------------------------------------------------------------------------------------------------
template <class Excl>
struct RanksEpilogue {
    static constexpr int K = Excl::ARRAYS;
    const float* gw;
    typename Excl::Labels ggroup;
    int64_t nc;
    float* aux;                          // LDS [2][K][128] : w_j (NaN past nc: such a pair has no score), group bits
    float thr[2];                        // t_i of the lane's two rows (NaN: nothing counts)
    typename Excl::Label qg[2];          // their groups
    int better[2], tied[2];
    float aux_w;
    typename Excl::Label aux_g;
    const LaneInfo& L;

    __device__ __forceinline__ RanksEpilogue(const LaneInfo& l) : L(l) {}
    __device__ __forceinline__ void aux_issue(int, int64_t qtile) {
        if (L.tid < TB) {
            const int64_t j = qtile * TB + L.tid;
            aux_w = j < nc ? gw[j] : __builtin_nanf("");
            if constexpr (Excl::BY_GROUP) aux_g = j < nc ? ggroup[j] : 0;     // never decides: such a pair has no score
        }
    }
    __device__ __forceinline__ void aux_commit(int t) {
        if (L.tid < TB) {
            float* dst = aux + (t & 1) * K * TB + L.tid;
            dst[0] = aux_w;
            if constexpr (Excl::BY_GROUP) reinterpret_cast<int32_t*>(dst)[TB] = aux_g;
        }
    }

    __device__ __forceinline__ void finish(int t, int64_t, f32x16 (&acc)[2][2]) {
        const float* a = aux + (t & 1) * K * TB + L.wm * 64 + L.h * 4;
        typedef int i32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(a + mt * 32 + g4 * 8);
                i32x4 g = {0, 0, 0, 0};
                if constexpr (Excl::BY_GROUP) g = *reinterpret_cast<const i32x4*>(a + TB + mt * 32 + g4 * 8);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float u = __fmul_rn(acc[mt][nt][g4 * 4 + e], w[e]);
                        bool gt = u > thr[nt], eq = u == thr[nt];
                        if constexpr (Excl::BY_GROUP) {
                            const bool other = g[e] != qg[nt];
                            gt = gt && other;
                            eq = eq && other;
                        }
                        better[nt] += gt ? 1 : 0;
                        tied[nt] += eq ? 1 : 0;
                    }
                }
            }
        }
    }
};

// pbetter / ptied [chunk * N + row] = the row's counts inside column chunk `chunk` (positives at t_i included in ptied)
template <bool KTAIL, class Excl>
__global__ void __launch_bounds__(ENGINE_THREADS, 2)
retrieval_kernel(const float* __restrict__ Q, int64_t N, int64_t ldq, const float* __restrict__ thr, typename Excl::Labels qgroup,
                 const float* __restrict__ G, int64_t M, int64_t ldg, const float* __restrict__ gw, typename Excl::Labels ggroup, int D,
                 int nchunks, int* __restrict__ pbetter, int* __restrict__ ptied) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LaneInfo L;
    const WorkItem w = work_item((M + TB - 1) / TB, nchunks);
    const int chunk = blockIdx.x % nchunks;            // the chunk work_item gave this workgroup: its slice of the partials

    RanksEpilogue<Excl> epi(L);
    epi.gw = gw;
    if constexpr (Excl::BY_GROUP) epi.ggroup = ggroup;
    epi.nc = M;
    epi.aux = lds + ENGINE_LDS_FLOATS;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int64_t i = sweep_row(w.prow0, L, nt);
        epi.thr[nt] = i < N ? thr[i] : __builtin_nanf("");        // (a row past the end is never stored)
        if constexpr (Excl::BY_GROUP) epi.qg[nt] = i < N ? qgroup[i] : 0;
        epi.better[nt] = 0;
        epi.tied[nt] = 0;
    }
    // the gallery rows are the engine's Q operand (the register axis), the query rows its P operand (the lane axis)
    dense_pipeline_early<EV_DEFAULT, KTAIL>(G, M, ldg, LinearTiles{w.qtile0}, Q, N, ldq, w.prow0, w.ntiles, D, lds, L, epi);

    // a row is covered by 4 lanes (2 half-waves x 2 column-half waves): [128][4] counts twice through the staging slabs,
    // free now
    int* mgb = reinterpret_cast<int*>(lds);
    int* mgt = mgb + TB * 4;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int slot = join_slot(L, nt);
        mgb[slot] = epi.better[nt];
        mgt[slot] = epi.tied[nt];
    }
    __syncthreads();
    if (L.tid < TB) {
        const int64_t i = joined_row(w.prow0, L.tid);
        if (i < N) {
            int b = mgb[L.tid * 4], e = mgt[L.tid * 4];
#pragma unroll
            for (int s = 1; s < 4; ++s) {
                b += mgb[L.tid * 4 + s];
                e += mgt[L.tid * 4 + s];
            }
            pbetter[(int64_t)chunk * N + i] = b;
            ptied[(int64_t)chunk * N + i] = e;
        }
    }
}

// the chunks' partials of a row in chunk order, the tied positives taken off again; -1, -1 for an unranked row
__global__ void __launch_bounds__(SIDE_THREADS)
retrieval_merge_kernel(const int* __restrict__ pbetter, const int* __restrict__ ptied, int64_t N, int nchunks,
                       const int32_t* __restrict__ tied_pos, const int64_t* __restrict__ positive, int32_t* __restrict__ out_better,
                       int32_t* __restrict__ out_tied) {
    const int64_t i = (int64_t)blockIdx.x * SIDE_THREADS + threadIdx.x;
    if (i >= N) return;
    int b = pbetter[i], e = ptied[i];
    for (int ch = 1; ch < nchunks; ++ch) {
        b += pbetter[(int64_t)ch * N + i];
        e += ptied[(int64_t)ch * N + i];
    }
    const bool ranked = positive[i] >= 0;
    out_better[i] = ranked ? b : -1;
    out_tied[i] = ranked ? e - tied_pos[i] : -1;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// the counts are int32: M <= 2^31 - 1
static bool shape_ok(int64_t N, int64_t M, int D) { return sweep_shape_ok(N, M, D, COLUMNS_ANY) && M <= (int64_t)0x7fffffff; }

struct Buffers {
    float *qn, *gn, *wq, *wg, *thr;
    int32_t* tied_pos;
    int *pbetter, *ptied;
};
static void carve(Carver& c, int64_t N, int64_t M, int nchunks, Buffers& b) {
    b.qn = c.take<float>((size_t)N);
    b.gn = c.take<float>((size_t)M);
    b.wq = c.take<float>((size_t)N);
    b.wg = c.take<float>((size_t)M);
    b.thr = c.take<float>((size_t)N);
    b.tied_pos = c.take<int32_t>((size_t)N);
    b.pbetter = c.take<int>((size_t)nchunks * (size_t)N);
    b.ptied = c.take<int>((size_t)nchunks * (size_t)N);
}

static int launch_weights(const float* norm, int64_t n, int cosine, float* w, hipStream_t st) {
    hipLaunchKernelGGL(retrieval_weights_kernel, dim3((unsigned)ceil_div(n, SIDE_THREADS)), dim3(SIDE_THREADS), 0, st, norm, n, cosine, w);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

template <class Excl>
static int launch_tiles(const float* Q, int64_t N, int64_t ldq, const float* thr, typename Excl::Labels q_group, const float* G, int64_t M,
                        int64_t ldg, const float* wg, typename Excl::Labels g_group, int D, int nchunks, int* pbetter, int* ptied,
                        hipStream_t st) {
    return launch_sweep(&retrieval_kernel<false, Excl>, &retrieval_kernel<true, Excl>, LDS_BYTES<Excl>, N, nchunks, D, st, Q, N, ldq, thr,
                        q_group, G, M, ldg, wg, g_group, D, nchunks, pbetter, ptied);
}

}  // namespace retrieval
}  // namespace am

using namespace am;

extern "C" size_t am_retrieval_workspace_bytes(int64_t N, int64_t M, int D) {
    if (!retrieval::shape_ok(N, M, D)) return 0;
    Carver c(nullptr, 0);
    retrieval::Buffers b;
    retrieval::carve(c, N, M, choose_chunks(N, M), b);
    return c.off;
}

extern "C" int am_retrieval_chunks(int64_t N, int64_t M, int D) { return retrieval::shape_ok(N, M, D) ? choose_chunks(N, M) : 0; }

extern "C" int am_retrieval_ranks_f32(const float* Q, int64_t N, int64_t ldq, const float* G, int64_t M, int64_t ldg, int D, int cosine,
                                      const int64_t* pos_start, const int64_t* pos_count, const int64_t* pos_columns,
                                      int64_t n_pos_columns, const int32_t* q_group, const int32_t* g_group, int32_t* out_better,
                                      int32_t* out_tied, float* out_score, int64_t* out_positive, int32_t* out_n_pos,
                                      int32_t* out_n_pos_own_group, void* ws, size_t ws_bytes, am_stream_t stream) {
    int rc;
    if ((rc = check_matrix(Q, N, ldq, D, "Q")) != AM_OK) return rc;
    if ((rc = check_matrix(G, M, ldg, D, "G")) != AM_OK) return rc;
    AM_REQUIRE(pos_start != nullptr && pos_count != nullptr, AM_ERR_BAD_ARG, "%s is null", pos_start == nullptr ? "pos_start" : "pos_count");
    AM_REQUIRE(n_pos_columns >= 0, AM_ERR_BAD_ARG, "n_pos_columns=%lld is negative", (long long)n_pos_columns);
    AM_REQUIRE(pos_columns != nullptr || n_pos_columns == 0, AM_ERR_BAD_ARG, "pos_columns is null");
    AM_REQUIRE((q_group == nullptr) == (g_group == nullptr), AM_ERR_BAD_ARG, "%s is null and %s is not: group ids go with both sides or neither",
               q_group == nullptr ? "q_group" : "g_group", q_group == nullptr ? "g_group" : "q_group");
    AM_REQUIRE(out_better != nullptr && out_tied != nullptr && out_score != nullptr && out_positive != nullptr && out_n_pos != nullptr &&
                   out_n_pos_own_group != nullptr,
               AM_ERR_BAD_ARG, "%s is null",
               out_better == nullptr ? "out_better" : out_tied == nullptr ? "out_tied" : out_score == nullptr ? "out_score"
               : out_positive == nullptr ? "out_positive" : out_n_pos == nullptr ? "out_n_pos" : "out_n_pos_own_group");
    AM_REQUIRE(retrieval::shape_ok(N, M, D), AM_ERR_BAD_SHAPE, "N=%lld M=%lld: too large for one launch (the counts are int32: M < 2^31)",
               (long long)N, (long long)M);
    const int nchunks = choose_chunks(N, M);
    Carver c(ws, ws_bytes);
    retrieval::Buffers b;
    retrieval::carve(c, N, M, nchunks, b);
    AM_REQUIRE(c.ok(), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (am_retrieval_workspace_bytes), have %zu", c.off, ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int cos = cosine != 0 ? 1 : 0;
    const float* gn;
    if ((rc = launch_norms_pair(Q, N, ldq, G, M, ldg, D, b.qn, b.gn, st, &gn)) != AM_OK) return rc;
    if ((rc = retrieval::launch_weights(b.qn, N, cos, b.wq, st)) != AM_OK) return rc;
    if ((rc = retrieval::launch_weights(gn, M, cos, b.wg, st)) != AM_OK) return rc;
    hipLaunchKernelGGL(retrieval::retrieval_positives_kernel, dim3((unsigned)ceil_div(N, retrieval::SIDE_THREADS)),
                       dim3(retrieval::SIDE_THREADS), 0, st, Q, N, ldq, G, M, ldg, D, cos, (const float*)b.wq, (const float*)b.wg, pos_start,
                       pos_count, pos_columns, n_pos_columns, q_group, g_group, b.thr, b.tied_pos, out_score, out_positive, out_n_pos,
                       out_n_pos_own_group);
    AM_LAUNCH_CHECK();
    if (q_group != nullptr)
        rc = retrieval::launch_tiles<retrieval::OtherGroups>(Q, N, ldq, b.thr, q_group, G, M, ldg, b.wg, g_group, D, nchunks, b.pbetter,
                                                             b.ptied, st);
    else
        rc = retrieval::launch_tiles<retrieval::AllColumns>(Q, N, ldq, b.thr, {}, G, M, ldg, b.wg, {}, D, nchunks, b.pbetter, b.ptied, st);
    if (rc != AM_OK) return rc;
    hipLaunchKernelGGL(retrieval::retrieval_merge_kernel, dim3((unsigned)ceil_div(N, retrieval::SIDE_THREADS)),
                       dim3(retrieval::SIDE_THREADS), 0, st, (const int*)b.pbetter, (const int*)b.ptied, N, nchunks,
                       (const int32_t*)b.tied_pos, (const int64_t*)out_positive, out_better, out_tied);
    AM_LAUNCH_CHECK();
    return AM_OK;
}
