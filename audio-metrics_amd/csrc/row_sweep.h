// The row sweep: every row of one set against all rows of another on the exact f32 128 x 128 tile engine, without an
// N x M matrix.  The search (knn_search.hip), the k-means assign (kmeans.hip), the per-sample scores (sample_scores.hip),
// the soft-min (softmin.hip), the scoring rule (psr.hip) and both sweeps of fld.hip are one plan with seven epilogues:
//   * dense_pipeline_early with the production schedule, the KTAIL instantiation for D % 32 != 0;
//   * the (row block) x (column chunk) plan of work_item / choose_chunks, one workgroup per (block, chunk);
//   * K f32 values per column staged through LDS beside the operand slabs (ColumnAux; the search, the scores and the
//     soft-min stage the same [2][K][128] layout by hand - through ColumnAux their instruction streams moved);
//   * a lane keeps a few values for each of its two rows; the four lanes of a row (2 half-waves x 2 column-half waves)
//     meet in LDS in a fixed slot order (join_slot / joined_row; the search merges lists, one P tile per pass, on its
//     own arithmetic) and leave one partial per (chunk, row) for a merge kernel.
// What differs between the files is the arithmetic of `finish`, what a lane keeps, and the merge kernel's output.
// This header holds everything else once: the index arithmetic of the plan, the block reductions and the online
// log-sum-exp of the merge kernels, and the host side of a launch.  swd.hip and rff.hip, whose epilogues store tiles and
// join nothing, share the launcher.
#pragma once
#include "pairwise_common.h"

namespace am {

// ---- geometry of a lane inside its workgroup's 128 rows -----------------------------------------------------------------
// (each is written as one sum from the left, base first: the tile kernels are register-tight and a re-associated index
// moves their register allocation)
// row that lane L holds in its P tile nt; base = the row block's first row, or 0 for the row inside the block
template <class B>
__device__ __forceinline__ B sweep_row(B base, const LaneInfo& L, int nt) { return base + L.wn * 64 + nt * 32 + L.r; }
// where that lane's values of the row go for the join: [2][64][4], the four lanes of a row side by side
__device__ __forceinline__ int join_slot(const LaneInfo& L, int nt) { return (nt * 64 + L.wn * 32 + L.r) * 4 + (L.wm * 2 + L.h); }
// row that thread tid < 128 joins: its four slots start at tid * 4
__device__ __forceinline__ int64_t joined_row(int64_t base, int tid) {
    const int nt = tid >> 6, q = tid & 63;
    return base + (q >> 5) * 64 + nt * 32 + (q & 31);
}

// The join itself stays in each kernel - LDS arrays of its own value types at [join_slot], one barrier, thread tid < 128
// folds slots tid * 4 .. tid * 4 + 3 in slot order and stores part[chunk * N + joined_row]: a variadic template for it
// moved the instruction streams of the kernels that join more than one value per row.

// |x_i|^2 of the lane's row in P tile nt; 0 past the end (such a row is never stored)
__device__ __forceinline__ float row_norm(const float* xnorm, int64_t prow0, int64_t N, const LaneInfo& L, int nt) {
    const int64_t i = sweep_row(prow0, L, nt);
    return i < N ? xnorm[i] : 0.f;
}

// ---- K per-column f32 arrays of a Q tile through LDS: [2][K][128], array k of buffer t & 1 at (t & 1) * K * TB + k * TB ----
// What a column past the end reads is part of the type, one value per array: +inf for a norm (such a pair is at distance
// +inf), else whatever makes the epilogue's arithmetic on that pair harmless.  (A pad kept in a member moves the register
// allocation of the tile kernels.)
enum ColumnPad { PAD_ZERO, PAD_ONE, PAD_INF, PAD_NEG_INF };
__device__ constexpr float pad_value(ColumnPad p) {
    return p == PAD_INF ? __builtin_inff() : p == PAD_NEG_INF ? -__builtin_inff() : p == PAD_ONE ? 1.f : 0.f;
}

// The base of an epilogue: aux_issue / aux_commit are what the pipeline calls, tile(t) is what finish(t) reads - the
// lane's first column of array 0; array k is TB floats further, the columns of accumulator register reg of tile mt are at
// mt * 32 + 8 * (reg >> 2) + (reg & 3).
template <ColumnPad... P>
struct ColumnAux {
    static constexpr int K = sizeof...(P);
    const float* src[K];                 // the arrays, nc values each
    int64_t nc;
    float* lds;
    float staged[K];
    const LaneInfo& L;

    __device__ __forceinline__ ColumnAux(const LaneInfo& l) : L(l) {}
    static __device__ constexpr float pad(int k) {
        float v = 0.f;
        int i = 0;
        ((v = i++ == k ? pad_value(P) : v), ...);
        return v;
    }
    __device__ __forceinline__ void aux_issue(int, int64_t qtile) {
        if (L.tid < TB) {
            const int64_t j = qtile * TB + L.tid;
#pragma unroll
            for (int k = 0; k < K; ++k) staged[k] = j < nc ? src[k][j] : pad(k);
        }
    }
    __device__ __forceinline__ void aux_commit(int t) {
        if (L.tid < TB) {
#pragma unroll
            for (int k = 0; k < K; ++k) lds[(t & 1) * K * TB + k * TB + L.tid] = staged[k];
        }
    }
    __device__ __forceinline__ const float* tile(int t) const { return lds + (t & 1) * K * TB + L.wm * 64 + L.h * 4; }
};

// ---- what one variant of a kernel has and another has not ------------------------------------------------------------------
// The type of a kernel parameter or an epilogue member in the instantiations that do not have it (the exclusion policies
// of knn_search.hip and sample_scores.hip).  Its size is 0: as a kernel parameter it takes no room in the kernel
// arguments (every other parameter keeps its offset), as a member no room in the struct.  It is only ever default-
// constructed and passed on.
struct Absent {
    int none[0];
};
static_assert(sizeof(Absent) == 0, "Absent must take no room: it holds a place in kernel parameter lists and epilogues");

// ---- reductions of a 256-thread merge kernel ----------------------------------------------------------------------------
struct SumOp {
    template <class T>
    __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};

// op over the workgroup's 256 values in a fixed tree: the same order on every call.  s[256] is free to reuse once every
// thread has its result: a caller that reduces twice through the same array puts a barrier between the two.
template <class Op, class T>
__device__ __forceinline__ T block_reduce_256(T v, T* s, Op op = Op()) {
    s[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const T o = s[threadIdx.x + w];
            s[threadIdx.x] = op(s[threadIdx.x], o);
        }
        __syncthreads();
    }
    return s[0];
}

// ---- online log-sum-exp: a running f32 maximum mx and the f64 sum s of exp(z - mx) ---------------------------------------
// (mx, s) <- (mx, s) + (mx2, s2).  The side that holds the maximum keeps its sum as it is; an empty side (-inf, 0) adds 0.
__device__ __forceinline__ void lse_join(float& mx, double& s, float mx2, double s2) {
    const float m = fmaxf(mx, mx2);
    const double a = mx == m ? s : s * exp((double)mx - (double)m);
    const double b = mx2 == m ? s2 : s2 * exp((double)mx2 - (double)m);
    mx = m;
    s = a + b;
}

// One accumulator tile's step of the running pair is two loops over the sixteen z a lane holds of it, which stay with the
// epilogue (z is evaluated twice, not kept; as a functor handed to a shared loop it moved the kernels' schedules), around
// this: tmax = the tile's maximum -> the sum is rescaled by exp(mx_old - mx_new) when the maximum rises in some lane, at
// most one more exp per tile -> the reference ref of the second loop, s += exp(z - ref).
__device__ __forceinline__ double lse_raise(float& mx, double& s, float tmax) {
    const float mnew = fmaxf(mx, tmax);
    if (__any(mnew != mx)) {                                   // the maximum rose in some lane: rescale its sum
        if (mnew != mx) s *= exp((double)mx - (double)mnew);   // from -inf: 0 * exp(-inf) = 0
        mx = mnew;
    }
    return mnew == -INFINITY ? 0.0 : (double)mnew;             // nothing finite yet: every term is 0
}

// ---- host side -----------------------------------------------------------------------------------------------------------
enum ColumnLimit {
    COLUMNS_ANY,                         // nothing beyond cols >= 1
    COLUMNS_KEYED,                       // a column is the low 32 bits of a key (0xffffffff = none): cols < 2^32 - 1
    COLUMNS_TILED                        // the column tiles are counted in an int
};
// the shapes one launch takes: one grid dimension holds row blocks x chunks (at most 64 chunks)
static inline bool sweep_shape_ok(int64_t rows, int64_t cols, int D, ColumnLimit limit) {
    if (!(rows >= 1 && cols >= 1 && D >= 1 && ceil_div(rows, TB) * 64 < (int64_t)0x7fffffff)) return false;
    return limit == COLUMNS_KEYED ? cols < (int64_t)0xffffffffll : limit == COLUMNS_TILED ? ceil_div(cols, TB) < (int64_t)0x7fffffff : true;
}

// |x|^2 of the rows of X into xn and of Y into yn - unless Y is X, a set against itself, which has one set of norms.
// *yn_used = the norms of Y.
static inline int launch_norms_pair(const float* X, int64_t N, int64_t ldx, const float* Y, int64_t M, int64_t ldy, int D, float* xn,
                                    float* yn, hipStream_t st, const float** yn_used) {
    const bool same = X == Y && N == M && ldx == ldy;
    int rc;
    if ((rc = launch_norms(X, N, ldx, D, xn, st)) != AM_OK) return rc;
    if (!same && (rc = launch_norms(Y, M, ldy, D, yn, st)) != AM_OK) return rc;
    *yn_used = same ? xn : yn;
    return AM_OK;
}

// One tile kernel over `rows` rows: grid = row blocks x chunks, lds_bytes of dynamic LDS.  The inner-dimension tail
// (D % 32 != 0) is a separate instantiation so the common kernel carries no tail code.
template <class... P, class... A>
static inline int launch_sweep(void (*plain)(P...), void (*tail)(P...), size_t lds_bytes, int64_t rows, int nchunks, int D,
                               hipStream_t st, A... args) {
    void (*kernel)(P...) = (D % BK) != 0 ? tail : plain;
    AM_HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), (int)lds_bytes));
    hipLaunchKernelGGL(kernel, dim3((unsigned)(ceil_div(rows, TB) * nchunks)), dim3(ENGINE_THREADS), lds_bytes, st,
                       static_cast<P>(args)...);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

}  // namespace am
