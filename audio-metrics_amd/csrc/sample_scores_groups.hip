// Per-sample fidelity on the PRDC manifold that leaves a whole GROUP out: am_sample_scores_f32 (sample_scores.hip) with one
// int32 label per row of X and per row of Y.  A pair (i, j) with x_group[i] == y_group[j] is no pair: it is not counted,
// its ratio is 0, it is no candidate of the rarity.
//     realism_i = max { r_j / |x_i - y_j| : label_j != label_i }
//     count_i   = #{ j : label_j != label_i, x_i inside ball j }
//     rarity_i  = min { r_j : label_j != label_i, x_i inside ball j }
// The embedding pipeline cuts every file into windows, so a window lies inside the balls of its own song's windows whatever
// the model did; with leave-group-out radii alone (knn_groups.hip) those balls even grow.  Only a membership pass that knows
// the labels scores a window against the OTHER songs.
//
// Everything but the exclusion is the contract of sample_scores.hip, to the bit: the arithmetic of a pair
//     d2 = max(fmaf(-2, <x, y>, |x|^2 + |y|^2), 0)       NaN -> +inf (clamp0); a padded column has |y|^2 = +inf
// on the exact f32 128 x 128 tile engine with the f32 norms of launch_norms, scores_columns_kernel's cleaned radii and
// thresholds T'(r_j), the strict test u < T', q = fdiv_rn(fmul_rn(r, r), d2) with NaN -> 0, the two 64-bit keys of
// sample_scores_keys.h (ties to the smallest column), the (row block) x (column chunk) plan, the [nchunks][N] partials and
// ONE merge kernel, sample_scores_merge_kernel, reached through scores::launch_merge.
//
// Labels.  The column labels travel as a fourth [128] array beside |y_j|^2, T'(r_j) and r_j through LDS, [2][4][128], staged
// by hand because the array is not float: a label is only moved and compared for equality, never computed with.  A lane
// keeps the labels of its two rows in two registers.
//
// Gates.  The dense loop is that of sample_scores.hip and does not know about the exclusion: cnt += u < T' over ALL columns,
// and the division gate's fma / max.  Both gates are supersets of what the labels leave, which costs time and never a result,
// because the exclusion is applied where a result is made:
//   - in the path that runs only when some lane's count moved in the 32 x 32 sub-tile, a member whose label equals the
//     row's takes 1 off the count again instead of making a min key (the count went up by exactly 1 for it: same test,
//     same bits);
//   - in the gated division path a same-label column makes no max key.  B, the lane's best ratio, is only ever raised by
//     admissible keys, so the gate's bound keeps its meaning.
//
// Register budget: that of sample_scores.hip with two label registers more; __launch_bounds__(256, 2), two workgroups per
// CU (2 x 76 KiB of LDS), no scratch (tests/test_sample_scores_groups_resources_cpu.py).
#include "sample_scores_keys.h"

namespace am {
namespace scores {

constexpr size_t GROUPS_LDS_BYTES = (ENGINE_LDS_FLOATS + 2 * 4 * TB) * sizeof(float);   // staging slabs + [2][4][128] column values

struct ScoresGroupEpilogue {
    const float* ynorm;
    const float* ythr;
    const float* yrad;
    const int32_t* ygroup;
    int64_t nc;
    float* aux;                          // LDS [2][4][128] : |y_j|^2 (+inf past nc), T'(r_j) (-inf past nc), r_j (0 past nc), label bits
    float xn[2];
    int32_t xg[2];                       // the labels of the lane's two rows
    unsigned long long kmax[2], kmin[2];
    int cnt[2];
    float aux_n, aux_t, aux_r;
    int32_t aux_g;
    const LaneInfo& L;

    __device__ __forceinline__ ScoresGroupEpilogue(const LaneInfo& l) : L(l) {}
    __device__ __forceinline__ void aux_issue(int, int64_t qtile) {
        if (L.tid < TB) {
            const int64_t j = qtile * TB + L.tid;
            aux_n = j < nc ? ynorm[j] : INFINITY;
            aux_t = j < nc ? ythr[j] : -INFINITY;
            aux_r = j < nc ? yrad[j] : 0.f;
            aux_g = j < nc ? ygroup[j] : 0;              // never decides: such a column is no member and its ratio is 0
        }
    }
    __device__ __forceinline__ void aux_commit(int t) {
        if (L.tid < TB) {
            float* dst = aux + (t & 1) * 4 * TB + L.tid;
            dst[0] = aux_n;
            dst[TB] = aux_t;
            dst[2 * TB] = aux_r;
            reinterpret_cast<int32_t*>(dst)[3 * TB] = aux_g;
        }
    }

    __device__ __forceinline__ void finish(int t, int64_t qtile, f32x16 (&acc)[2][2]) {
        const float* a = aux + (t & 1) * 4 * TB + L.wm * 64 + L.h * 4;
        const int32_t* g = reinterpret_cast<const int32_t*>(a + 3 * TB);
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
            // the dense loop of sample_scores.hip: all columns, the row's own group included
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
                        if (fmaf(nb[nt], u, r2) > lim[nt] && g[rel] != xg[nt]) {      // the row's own group: by label, no key
                            const float q0 = __fdiv_rn(r2, clamp0(u));
                            const float q = q0 != q0 ? 0.f : q0;
                            const unsigned long long key =
                                ((unsigned long long)__float_as_uint(q) << 32) | (0xffffffffu - (cbase + (unsigned)rel));
                            kmax[nt] = key > kmax[nt] ? key : kmax[nt];
                        }
                    }
                }
                // rare: the inside-pairs, of the own group or not
                if (__any(cnt[nt] != c0[nt])) {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int rel = mt * 32 + (reg & 3) + 8 * (reg >> 2);
                        const float u = fmaf(-2.f, acc[mt][nt][reg], xn[nt] + a[rel]);
                        if (u < a[TB + rel]) {
                            if (g[rel] == xg[nt]) {
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
template <bool KTAIL>
__global__ void __launch_bounds__(ENGINE_THREADS, 2)
sample_scores_groups_kernel(const float* __restrict__ X, int64_t N, int64_t ldx, const float* __restrict__ xnorm,
                            const int32_t* __restrict__ xgroup, const float* __restrict__ Y, int64_t M, int64_t ldy,
                            const float* __restrict__ ynorm, const float* __restrict__ ythr, const float* __restrict__ yrad,
                            const int32_t* __restrict__ ygroup, int D, int nchunks, unsigned long long* __restrict__ pmax,
                            unsigned long long* __restrict__ pmin, int* __restrict__ pcnt) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LaneInfo L;
    const WorkItem w = work_item((M + TB - 1) / TB, nchunks);
    const int chunk = blockIdx.x % nchunks;            // the chunk work_item gave this workgroup: its slice of the partials

    ScoresGroupEpilogue epi(L);
    epi.ynorm = ynorm;
    epi.ythr = ythr;
    epi.yrad = yrad;
    epi.ygroup = ygroup;
    epi.nc = M;
    epi.aux = lds + ENGINE_LDS_FLOATS;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        epi.xn[nt] = row_norm(xnorm, w.prow0, N, L, nt);
        const int64_t i = sweep_row(w.prow0, L, nt);
        epi.xg[nt] = i < N ? xgroup[i] : 0;            // (a row past the end is never stored)
        epi.kmax[nt] = 0ull;
        epi.kmin[nt] = NO_MEMBER;
        epi.cnt[nt] = 0;
    }
    dense_pipeline_early<EV_DEFAULT, KTAIL>(Y, M, ldy, LinearTiles{w.qtile0}, X, N, ldx, w.prow0, w.ntiles, D, lds, L, epi);

    // the join of sample_scores_kernel: a row is covered by 4 lanes (2 half-waves x 2 column-half waves): [128][4] max keys,
    // min keys and counts through the staging slabs, free now
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

}  // namespace scores
}  // namespace am

using namespace am;

extern "C" size_t am_sample_scores_groups_workspace_bytes(int64_t N, int64_t M, int D) {
    if (!scores::shape_ok(N, M, D)) return 0;
    Carver c(nullptr, 0);
    scores::Buffers b;
    scores::carve(c, N, M, choose_chunks(N, M), b);
    return c.off;
}

extern "C" int am_sample_scores_groups_f32(const float* X, int64_t N, int64_t ldx, const int32_t* x_group, const float* Y, int64_t M,
                                           int64_t ldy, const int32_t* y_group, int D, const float* r_y, float* out_realism,
                                           int64_t* out_realism_idx, int32_t* out_count, float* out_rarity, int64_t* out_rarity_idx,
                                           void* ws, size_t ws_bytes, am_stream_t stream) {
    int rc;
    if ((rc = check_matrix(X, N, ldx, D, "X")) != AM_OK) return rc;
    if ((rc = check_matrix(Y, M, ldy, D, "Y")) != AM_OK) return rc;
    AM_REQUIRE(x_group != nullptr && y_group != nullptr, AM_ERR_BAD_ARG, "%s is null", x_group == nullptr ? "x_group" : "y_group");
    AM_REQUIRE(r_y != nullptr && out_realism != nullptr && out_realism_idx != nullptr && out_count != nullptr &&
                   out_rarity != nullptr && out_rarity_idx != nullptr,
               AM_ERR_BAD_ARG, "%s is null",
               r_y == nullptr ? "r_y" : out_realism == nullptr ? "out_realism" : out_realism_idx == nullptr ? "out_realism_idx"
               : out_count == nullptr ? "out_count" : out_rarity == nullptr ? "out_rarity" : "out_rarity_idx");
    AM_REQUIRE(scores::shape_ok(N, M, D), AM_ERR_BAD_SHAPE, "N=%lld M=%lld: a column index takes 32 bits of a key (M < 2^32 - 1)",
               (long long)N, (long long)M);
    const int nchunks = choose_chunks(N, M);
    Carver c(ws, ws_bytes);
    scores::Buffers b;
    scores::carve(c, N, M, nchunks, b);
    AM_REQUIRE(c.ok(), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (am_sample_scores_groups_workspace_bytes), have %zu",
               c.off, ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float* yn;
    if ((rc = launch_norms_pair(X, N, ldx, Y, M, ldy, D, b.xn, b.yn, st, &yn)) != AM_OK) return rc;
    if ((rc = scores::launch_columns(r_y, M, b.rad, b.thr, st)) != AM_OK) return rc;
    rc = launch_sweep(&scores::sample_scores_groups_kernel<false>, &scores::sample_scores_groups_kernel<true>, scores::GROUPS_LDS_BYTES, N,
                      nchunks, D, st, X, N, ldx, b.xn, x_group, Y, M, ldy, yn, b.thr, b.rad, y_group, D, nchunks, b.pmax, b.pmin, b.pcnt);
    if (rc != AM_OK) return rc;
    return scores::launch_merge(b.pmax, b.pmin, b.pcnt, N, nchunks, out_realism, out_realism_idx, out_count, out_rarity, out_rarity_idx,
                                st);
}
