// Exact k-nearest-neighbour search that leaves a whole GROUP out: every row of X and of Y carries one int32 label, and
// row i of X gets its k nearest rows of Y whose label differs from its own.  The embedding pipeline cuts every file into
// windows, so stored rows come in runs of near-duplicates per track; with "row i itself, by index" as the only exclusion
// (knn_search.hip) the nearest neighbour of almost every window is a sibling window of its own song.
//
// Everything but the exclusion is the contract of knn_search.hip: the arithmetic of a pair
//     d2 = max(fmaf(-2, <x, y>, |x|^2 + |y|^2), 0)       NaN -> +inf (clamp0); a padded column has |y|^2 = +inf
// on the exact f32 128 x 128 tile engine with the f32 row norms of launch_norms, the 64-bit keys of knn_keys.h (ties go to
// the smallest column whatever the chunking, the tile order or the lane that saw the value), the (row block) x (column
// chunk) plan, the partial lists uint64 [nchunks][N][KCAP] and ONE merge kernel - knn_search_merge_kernel of knn_search.hip,
// reached through search::launch_merge.
//
// Labels.  The column labels travel beside the column norms through LDS, [2][2][128]: array 0 is |y_j|^2 (+inf past the
// end), array 1 the 32 bits of the label (the layout of ColumnAux of row_sweep.h, staged by hand because array 1 is not a
// float: a label is only moved and compared for equality, never computed with).  A lane keeps the labels of its two rows
// in two registers.  There is no diagonal: which columns a row skips is not tied to its index.
//
// Gates.  Both gates of knn_search.hip - the tile minimum, then __any per element - run on the plain values and do not know
// about the exclusion: they are supersets (a 32 x 32 sub-tile that holds a same-label pair closer than the row's list end
// always passes the first one), which costs time and never a result, because the exclusion is applied where a key is made:
// inside the wave-uniform insert loop, where one LDS word per candidate is read already,
//     d2 = (label[column] == label[row]) ? +inf : clamp0(u)
// and a key at +inf never displaces a finite one (the merge reports it as (+inf, -1)).  The gates are strict (d2 < last)
// for the reason given in knn_search.hip: a lane meets the columns of its chunk in increasing order and its list holds
// admissible columns only, so a value equal to the list's last distance always has the larger column and loses the tie
// anyway; the insert itself compares whole keys.
//
// Register budget: the lists of knn_search.hip (2 rows x KCAP keys x 2 registers per lane) with two label registers in
// place of the diagonal's bookkeeping; no instantiation uses scratch, two workgroups per CU for the lists of 8 and 16
// keys, one for the 32-key lists (tests/test_knn_groups_cpu.py).
#include "knn_keys.h"

namespace am {
namespace search {

constexpr size_t GROUPS_LDS_BYTES = (ENGINE_LDS_FLOATS + 2 * 2 * TB) * sizeof(float);   // staging slabs + [2][2][128] norms, labels

template <int KCAP>
struct KnnGroupEpilogue {
    const float* qnorm;
    const int32_t* qgroup;
    int64_t nq;
    float* aux;                          // LDS [2][2][128] : |y_j|^2 of the tile (+inf past nq), then the labels' bits
    float xn[2];
    int32_t xg[2];                       // the labels of the lane's two rows
    unsigned long long best[2][KCAP];
    float aux_reg;
    int32_t aux_grp;
    const LaneInfo& L;

    __device__ __forceinline__ KnnGroupEpilogue(const LaneInfo& l) : L(l) {}
    __device__ __forceinline__ void aux_issue(int, int64_t qtile) {
        if (L.tid < TB) {
            const int64_t j = qtile * TB + L.tid;
            aux_reg = j < nq ? qnorm[j] : INFINITY;
            aux_grp = j < nq ? qgroup[j] : 0;            // never looked at: such a pair is at +inf already
        }
    }
    __device__ __forceinline__ void aux_commit(int t) {
        if (L.tid < TB) {
            aux[(t & 1) * 2 * TB + L.tid] = aux_reg;
            reinterpret_cast<int32_t*>(aux)[(t & 1) * 2 * TB + TB + L.tid] = aux_grp;
        }
    }
    __device__ __forceinline__ float last(int nt) const { return __uint_as_float((unsigned)(best[nt][KCAP - 1] >> 32)); }

    // The gates run on values that are recomputed, not kept, and unclamped (knn_search.hip: KnnIndexEpilogue::finish), and on
    // ALL columns, the row's own group included.  Past them the registers that may improve some lane's list are visited
    // through a wave-uniform bit mask, and only there the label of the column is read and compared.
    __device__ __forceinline__ void finish(int t, int64_t qtile, f32x16 (&acc)[2][2]) {
        const float* a = aux + (t & 1) * 2 * TB + L.wm * 64 + L.h * 4;
        const int32_t* g = reinterpret_cast<const int32_t*>(a + TB);
        const unsigned cbase = (unsigned)(qtile * TB + L.wm * 64 + L.h * 4);       // the lane's first column of the tile
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            f32x4 yn[4];
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) yn[g4] = *reinterpret_cast<const f32x4*>(a + mt * 32 + g4 * 8);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                auto value = [&](int reg) { return fmaf(-2.f, acc[mt][nt][reg], xn[nt] + yn[reg >> 2][reg & 3]); };
                float tmin = INFINITY;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) tmin = fminf(tmin, value(reg));
                tmin = fmaxf(tmin, 0.f);
                // common case after warm-up: no lane of the wave improves its list with this 32 x 32 tile
                if (__any(tmin < last(nt))) {
                    unsigned mask = 0;
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg)
                        if (__any(value(reg) < last(nt))) mask |= 1u << reg;
                    while (mask != 0) {                             // wave-uniform, ascending registers = ascending columns
                        const int reg = __builtin_ctz(mask);
                        mask &= mask - 1;
                        const int rel = mt * 32 + (reg & 3) + 8 * (reg >> 2);
                        float p = acc[mt][nt][0];
#pragma unroll
                        for (int q = 1; q < 16; ++q) p = (reg == q) ? acc[mt][nt][q] : p;
                        const float u = fmaf(-2.f, p, xn[nt] + a[rel]);
                        const float d2 = g[rel] == xg[nt] ? INFINITY : clamp0(u);      // the row's own group: by label
                        key_insert<KCAP>(best[nt], ((unsigned long long)(__float_as_uint(d2) & 0x7fffffffu) << 32) | (cbase + (unsigned)rel));
                    }
                }
            }
        }
    }
};

// partial[(chunk * N + row) * KCAP + s] = s-th smallest key of `row` inside column chunk `chunk`
template <int KCAP, bool KTAIL>
__global__ void __launch_bounds__(ENGINE_THREADS, KCAP <= 16 ? 2 : 1)
knn_groups_kernel(const float* __restrict__ X, int64_t N, int64_t ldx, const float* __restrict__ xnorm,
                  const int32_t* __restrict__ xgroup, const float* __restrict__ Y, int64_t M, int64_t ldy,
                  const float* __restrict__ ynorm, const int32_t* __restrict__ ygroup, int D, int nchunks,
                  unsigned long long* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LaneInfo L;
    const WorkItem w = work_item((M + TB - 1) / TB, nchunks);
    const int chunk = blockIdx.x % nchunks;            // the chunk work_item gave this workgroup: its slice of `partial`

    KnnGroupEpilogue<KCAP> epi(L);
    epi.qnorm = ynorm;
    epi.qgroup = ygroup;
    epi.nq = M;
    epi.aux = lds + ENGINE_LDS_FLOATS;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        epi.xn[nt] = row_norm(xnorm, w.prow0, N, L, nt);
        const int64_t i = sweep_row(w.prow0, L, nt);
        epi.xg[nt] = i < N ? xgroup[i] : 0;            // (a row past the end is never stored)
#pragma unroll
        for (int s = 0; s < KCAP; ++s) epi.best[nt][s] = EMPTY_KEY;
    }
    dense_pipeline_early<EV_DEFAULT, KTAIL>(Y, M, ldy, LinearTiles{w.qtile0}, X, N, ldx, w.prow0, w.ntiles, D, lds, L, epi);

    // The join of knn_search_kernel, on the same slot and row arithmetic: a P row is covered by 4 lists (2 half-waves x 2
    // Q-half waves), merged through LDS, the rows of one 32-row P tile per wave at a time ([64][4][KCAP] keys: 64 KiB at
    // KCAP = 32, inside the 72 KiB of staging slabs, which are free now)
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

template <int KCAP>
static int run_groups(const float* X, int64_t N, int64_t ldx, const float* xn, const int32_t* xg, const float* Y, int64_t M, int64_t ldy,
                      const float* yn, const int32_t* yg, int D, int k, int nchunks, int squared, unsigned long long* partial,
                      float* out_dist, int64_t* out_idx, hipStream_t st) {
    const int rc = launch_sweep(&knn_groups_kernel<KCAP, false>, &knn_groups_kernel<KCAP, true>, GROUPS_LDS_BYTES, N, nchunks, D, st, X,
                                N, ldx, xn, xg, Y, M, ldy, yn, yg, D, nchunks, partial);
    if (rc != AM_OK) return rc;
    return launch_merge(KCAP, partial, N, nchunks, k, squared, out_dist, out_idx, st);
}

}  // namespace search
}  // namespace am

using namespace am;

extern "C" size_t am_knn_search_groups_workspace_bytes(int64_t N, int64_t M, int D, int k) {
    if (!search::shape_ok(N, M, D, k)) return 0;
    Carver c(nullptr, 0);
    search::Buffers b;
    search::carve(c, N, M, k, choose_chunks(N, M), b);
    return c.off;
}

extern "C" int am_knn_search_groups_f32(const float* X, int64_t N, int64_t ldx, const int32_t* x_group, const float* Y, int64_t M,
                                        int64_t ldy, const int32_t* y_group, int D, int k, int squared, float* out_dist,
                                        int64_t* out_idx, void* ws, size_t ws_bytes, am_stream_t stream) {
    int rc;
    if ((rc = check_matrix(X, N, ldx, D, "X")) != AM_OK) return rc;
    if ((rc = check_matrix(Y, M, ldy, D, "Y")) != AM_OK) return rc;
    AM_REQUIRE(x_group != nullptr && y_group != nullptr, AM_ERR_BAD_ARG, "%s is null", x_group == nullptr ? "x_group" : "y_group");
    AM_REQUIRE(out_dist != nullptr && out_idx != nullptr, AM_ERR_BAD_ARG, "%s is null", out_dist == nullptr ? "out_dist" : "out_idx");
    AM_REQUIRE(k >= 1 && k <= search::MAX_K, AM_ERR_BAD_SHAPE, "k = %d: the search keeps 1 .. %d neighbours per row", k, search::MAX_K);
    AM_REQUIRE(search::shape_ok(N, M, D, k), AM_ERR_BAD_SHAPE,
               "N=%lld M=%lld: a column index takes 32 bits of a list key (M < 2^32 - 1)", (long long)N, (long long)M);
    const int nchunks = choose_chunks(N, M);
    Carver c(ws, ws_bytes);
    search::Buffers b;
    search::carve(c, N, M, k, nchunks, b);
    AM_REQUIRE(c.ok(), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (am_knn_search_groups_workspace_bytes), have %zu", c.off,
               ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float* yn;
    if ((rc = launch_norms_pair(X, N, ldx, Y, M, ldy, D, b.xn, b.yn, st, &yn)) != AM_OK) return rc;
    switch (search::kcap_for(k)) {
        case 8:  return search::run_groups<8>(X, N, ldx, b.xn, x_group, Y, M, ldy, yn, y_group, D, k, nchunks, squared, b.partial, out_dist, out_idx, st);
        case 16: return search::run_groups<16>(X, N, ldx, b.xn, x_group, Y, M, ldy, yn, y_group, D, k, nchunks, squared, b.partial, out_dist, out_idx, st);
        default: return search::run_groups<32>(X, N, ldx, b.xn, x_group, Y, M, ldy, yn, y_group, D, k, nchunks, squared, b.partial, out_dist, out_idx, st);
    }
}
