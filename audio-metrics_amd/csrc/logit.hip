// One fused pass of K linear logistic probes over the stored rows of ONE set, so one class (am_logit_pass_f32 / _f64): the
// hot path of the classifier two-sample test (metrics/c2st.py).  Per row i, model k and class sign s (+1: label 1, -1: label 0)
//     z_ik = b_k + sum_d a_kd x_id,   t = s z,   loss = max(-t, 0) + log1p(exp(-|t|)),   r = -s / (1 + exp(t))    (= p - y)
// and per model, over the rows that TRAIN it (fold[i] in 0..K and != k, every element finite),
//     sums[k] = { sum_i r x_id (d = 0..D-1), sum_i r, sum_i loss }.
// z_out[i] is z under the model of the row's own fold (held out of it), NaN where the row has none.
//
//   logit_rows_kernel   one workgroup owns 64 rows at a time and walks its row blocks g, g + grid, ... in order.
//                       Forward: Z[64][16] = X coef^T on v_mfma_f64_16x16x4_f64 (wave w the rows 16 w .. 16 w + 15, the models
//                       padded to 16 columns of zeros), 32-deep slabs of the inner dimension ascending through a double-buffered
//                       LDS ring; float32 rows are converted on load (exact), so both row types share every later bit.  Then r
//                       goes into LDS and the block's sums of r and of the loss are folded by shuffles in a fixed order.
//                       Backward: G[16][D] += R^T X on the same instruction - the block's rows go through the same ring a second
//                       time (they come from L2), rows with a non-finite element staged as zeros; wave w forms the 16-column tile
//                       (w & 1) over the row half (w >> 1), the two halves are added lower + upper, and the tile is added into
//                       the workgroup's partial (every element of it is owned by one lane for the whole launch).
//   logit_sums_kernel   adds the workgroups' partials in workgroup order, one thread per output element.
// No floating-point atomics and no data-dependent order: the grid is min(ceil(N / 64), 256), a function of N alone, so two calls
// return the same bits.  A column of an MFMA result depends on its own column of the operand only, so a model's sums and a row's
// z do not depend on the other models of the call or on K, and a row's z depends on that row and its model alone.
#include "am_common.h"

namespace am {

constexpr int LG_TILE = 64, LG_KT = 32, LG_LDT = 46, LG_MODELS = 16, LG_GRID = 256;
// LG_LDT: row stride of the staged slab in f64.  2 * 46 = 28 (mod 64) dwords: the forward read (16 rows x 2 k per 32-lane group)
// is free of bank conflicts, the backward read (2 rows x 16 columns) has 2 lanes of 32 two-way; 46 * 8 bytes is a multiple of 16.

typedef double lg_f64x4 __attribute__((ext_vector_type(4)));
typedef float lg_f32x4 __attribute__((ext_vector_type(4)));

// the 8 elements of one row's slab that one thread stages.  Thread (row = tid >> 2, q = tid & 3): float32 rows take two 16-byte
// loads at k = 16 j + 4 q (four lanes read 64 consecutive bytes; rows are 16-byte aligned with ld % 4 == 0, so a load at a
// multiple of 4 below D stays inside the row's ld), float64 rows eight loads at k = 4 j + q.  Every load is unconditional: an
// index past the end is clamped into the row and its value masked when the slab is staged.
template <class T> struct LgRaw;
template <> struct LgRaw<float> { lg_f32x4 v[2]; };
template <> struct LgRaw<double> { double v[8]; };

__device__ __forceinline__ int lg_k(float, int q, int e) { return (e >> 2) * 16 + q * 4 + (e & 3); }
__device__ __forceinline__ int lg_k(double, int q, int e) { return e * 4 + q; }

__device__ __forceinline__ void lg_load(const float* __restrict__ row, int k0, int q, int D, LgRaw<float>& r) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int k = k0 + j * 16 + q * 4;
        r.v[j] = *reinterpret_cast<const lg_f32x4*>(row + (k < D ? k : 0));
    }
}

__device__ __forceinline__ void lg_load(const double* __restrict__ row, int k0, int q, int D, LgRaw<double>& r) {
#pragma unroll
    for (int e = 0; e < 8; ++e) r.v[e] = row[min(k0 + e * 4 + q, D - 1)];
}

__device__ __forceinline__ double lg_get(const LgRaw<float>& r, int e) { return (double)r.v[e >> 2][e & 3]; }
__device__ __forceinline__ double lg_get(const LgRaw<double>& r, int e) { return r.v[e]; }

template <class T>
__global__ void __launch_bounds__(256) logit_rows_kernel(const T* __restrict__ X, int64_t N, int64_t ld, int D, const int32_t* __restrict__ fold,
                                                         int label, const double* __restrict__ coef, int K, double* __restrict__ z_out,
                                                         double* __restrict__ partials) {
    __shared__ double As[2][LG_TILE * LG_LDT];            // [row][k] of the slab
    __shared__ double CR[2 * LG_KT * LG_MODELS];          // forward: Cs[2][k][model]; backward: Rs[row][model]
    __shared__ double Gx[2][2 * 64 * 4];                  // the upper row half's tile, by step parity
    __shared__ double red[2][4][LG_MODELS];               // per wave: sum r, sum loss of its 16 rows
    __shared__ int fl[LG_TILE], rowbad[LG_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int srow = tid >> 2, sq = tid & 3;              // staging of X
    const int ck = tid >> 3, cm = (tid & 7) * 2;          // staging of coef: two models of one k
    const int ct = wave & 1, rh = wave >> 1;              // backward: column tile, row half
    const int nslab = (D + LG_KT - 1) / LG_KT, steps = 2 * nslab;
    const int64_t nblocks = (N + LG_TILE - 1) / LG_TILE;
    const int64_t stride = (int64_t)K * (D + 2) + 2;
    double* __restrict__ part = partials + (int64_t)blockIdx.x * stride;
    const double sgn = label ? 1.0 : -1.0;
    const double bias = l15 < K ? coef[(int64_t)l15 * (D + 1) + D] : 0.0;

    double r_acc = 0.0, loss_acc = 0.0;                   // threads 0..15: model tid, over this workgroup's blocks
    double n_part = 0.0, n_bad = 0.0;                     // thread 0
    bool first = true;

    for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x, first = false) {
        const int64_t row0 = blk * LG_TILE;
        const bool srow_ok = row0 + srow < N;
        const T* prow = X + (srow_ok ? row0 + srow : 0) * ld;

        LgRaw<T> raw;
        double cv[2];
        int k0_next = 0;
        auto fetch = [&](int step) {
            k0_next = (step % nslab) * LG_KT;
            lg_load(prow, k0_next, sq, D, raw);
            if (step < nslab) {
                const int k = min(k0_next + ck, D - 1);
#pragma unroll
                for (int e = 0; e < 2; ++e) cv[e] = coef[(int64_t)min(cm + e, K - 1) * (D + 1) + k];
            }
        };
        auto stage = [&](int step) {
            const int buf = step & 1;
            if (step < nslab) {                           // forward: the values as they are; a non-finite one marks its row
                bool bad = false;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int k = lg_k(T(), sq, e);
                    const double v = (srow_ok && k0_next + k < D) ? lg_get(raw, e) : 0.0;
                    bad |= !(v - v == 0.0);
                    As[buf][srow * LG_LDT + k] = v;
                }
                if (bad) rowbad[srow] = 1;
#pragma unroll
                for (int e = 0; e < 2; ++e)
                    CR[(buf * LG_KT + ck) * LG_MODELS + cm + e] = (cm + e < K && k0_next + ck < D) ? cv[e] : 0.0;
            } else {                                      // backward: a row with a non-finite element is staged as zeros
                const bool keep = srow_ok && !rowbad[srow];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int k = lg_k(T(), sq, e);
                    As[buf][srow * LG_LDT + k] = (keep && k0_next + k < D) ? lg_get(raw, e) : 0.0;
                }
            }
        };
        // lower row half: add the upper half's tile of slab `slab` and fold the sum into the workgroup's partial
        lg_f64x4 held = lg_f64x4{0.0, 0.0, 0.0, 0.0};
        auto flush = [&](int slab, int buf) {
            const int col = slab * LG_KT + ct * 16 + l15;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int model = l4 + 4 * r;
                if (model < K && col < D) {
                    const double v = held[r] + Gx[buf][(ct * 64 + lane) * 4 + r];
                    double* p = part + (int64_t)model * (D + 2) + col;
                    *p = first ? v : *p + v;
                }
            }
        };

        fetch(0);
        __syncthreads();                                  // the previous block is done with the LDS
        if (tid < LG_TILE) {
            fl[tid] = row0 + tid < N ? fold[row0 + tid] : -1;
            rowbad[tid] = 0;
        }
        __syncthreads();
        stage(0);
        __syncthreads();

        lg_f64x4 acc = lg_f64x4{0.0, 0.0, 0.0, 0.0};
        for (int step = 0; step < steps; ++step) {
            const int buf = step & 1;
            if (step + 1 < steps) fetch(step + 1);
            if (step < nslab) {
#pragma unroll
                for (int ks = 0; ks < LG_KT / 4; ++ks) {
                    const double a = As[buf][(wave * 16 + l15) * LG_LDT + ks * 4 + l4];
                    const double b = CR[(buf * LG_KT + ks * 4 + l4) * LG_MODELS + l15];
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
                }
                if (step == nslab - 1) {                  // Z is complete: r, the loss, z_out, the counts
                    __syncthreads();                      // every wave is done with Cs: Rs takes its place
                    double rs = 0.0, ls = 0.0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int rl = wave * 16 + l4 + 4 * r;
                        const int64_t row = row0 + rl;
                        const int f = fl[rl];
                        const bool ok = row < N && !rowbad[rl] && f >= 0 && f <= K;
                        const bool trains = ok && l15 < K && l15 != f;
                        const double z = acc[r] + bias;
                        const double t = sgn * z;
                        const double rv = trains ? -sgn / (1.0 + exp(t)) : 0.0;
                        const double lv = trains ? fmax(-t, 0.0) + log1p(exp(-fabs(t))) : 0.0;
                        CR[rl * LG_MODELS + l15] = rv;
                        rs += rv;
                        ls += lv;
                        if (z_out && row < N) {
                            if (ok && f < K) {
                                if (l15 == f) z_out[row] = z;
                            } else if (l15 == 0) {
                                z_out[row] = __builtin_nan("");
                            }
                        }
                    }
                    rs += __shfl_xor(rs, 16);
                    ls += __shfl_xor(ls, 16);
                    rs += __shfl_xor(rs, 32);
                    ls += __shfl_xor(ls, 32);
                    if (lane < LG_MODELS) {
                        red[0][wave][lane] = rs;
                        red[1][wave][lane] = ls;
                    }
                    if (wave == 0) {
                        const bool valid = row0 + lane < N;
                        const bool bad = rowbad[lane] != 0;
                        double np = (valid && !bad && fl[lane] >= 0 && fl[lane] <= K) ? 1.0 : 0.0;
                        double nb = (valid && bad) ? 1.0 : 0.0;
#pragma unroll
                        for (int off = 32; off >= 1; off >>= 1) {
                            np += __shfl_xor(np, off);
                            nb += __shfl_xor(nb, off);
                        }
                        n_part += np;
                        n_bad += nb;
                    }
                    acc = lg_f64x4{0.0, 0.0, 0.0, 0.0};
                }
            } else {
                if (step > nslab && rh == 0) flush(step - 1 - nslab, buf ^ 1);
                lg_f64x4 g = lg_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) {
                    const int rl = rh * 32 + kk * 4 + l4;
                    const double a = CR[rl * LG_MODELS + l15];
                    const double b = As[buf][rl * LG_LDT + ct * 16 + l15];
                    g = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, g, 0, 0, 0);
                }
                if (rh == 0) {
                    held = g;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) Gx[buf][(ct * 64 + lane) * 4 + r] = g[r];
                }
            }
            if (step + 1 < steps) stage(step + 1);        // its last readers passed the barrier of the previous step
            __syncthreads();
        }
        if (rh == 0) flush(nslab - 1, (steps - 1) & 1);
        if (tid < LG_MODELS) {                            // the four waves' rows, ascending
            r_acc += (red[0][0][tid] + red[0][1][tid]) + (red[0][2][tid] + red[0][3][tid]);
            loss_acc += (red[1][0][tid] + red[1][1][tid]) + (red[1][2][tid] + red[1][3][tid]);
        }
    }
    if (tid < K) {
        part[(int64_t)tid * (D + 2) + D] = r_acc;
        part[(int64_t)tid * (D + 2) + D + 1] = loss_acc;
    }
    if (tid == 0) {
        part[stride - 2] = n_part;
        part[stride - 1] = n_bad;
    }
}

// out[e] = sum over the workgroups' partials in workgroup order; the last two elements go to counts
__global__ void __launch_bounds__(256) logit_sums_kernel(const double* __restrict__ partials, int nwg, int64_t stride, double* __restrict__ sums,
                                                         double* __restrict__ counts) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= stride) return;
    double s = 0.0;
    for (int w = 0; w < nwg; ++w) s += partials[(int64_t)w * stride + e];
    if (e < stride - 2)
        sums[e] = s;
    else
        counts[e - (stride - 2)] = s;
}

static int logit_grid(int64_t N) {
    const int64_t blocks = ceil_div(N, (int64_t)LG_TILE);
    return blocks < LG_GRID ? (int)blocks : LG_GRID;
}

template <class T>
static int logit_pass(const T* X, int64_t N, int64_t ld, int D, const int32_t* fold, int label, const double* coef, int K, double* sums,
                      double* z_out, double* counts, void* ws, size_t ws_bytes, hipStream_t st) {
    AM_REQUIRE(X && fold && coef && sums && counts, AM_ERR_BAD_ARG, "null pointer");
    AM_REQUIRE(label == 0 || label == 1, AM_ERR_BAD_ARG, "label=%d (the class of every row of X: 1 or 0)", label);
    AM_REQUIRE(N >= 1 && D >= 1 && D <= 8192 && ld >= D, AM_ERR_BAD_SHAPE, "X has shape %lld x %d, ld=%lld (N >= 1, 1 <= D <= 8192, ld >= D)",
               (long long)N, D, (long long)ld);
    AM_REQUIRE(K >= 1 && K <= LG_MODELS, AM_ERR_BAD_SHAPE, "K=%d models (1 <= K <= 16)", K);
    if (sizeof(T) == 4)
        AM_REQUIRE(aligned16(X) && ld % 4 == 0, AM_ERR_BAD_SHAPE, "float32 rows must be 16-byte aligned with ld %% 4 == 0 (ld=%lld)",
                   (long long)ld);
    const int nwg = logit_grid(N);
    const int64_t stride = (int64_t)K * (D + 2) + 2;
    Carver c(ws, ws_bytes);
    double* partials = c.take<double>((size_t)nwg * stride);
    AM_REQUIRE(c.ok(), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (am_logit_pass_workspace_bytes), have %zu", c.off, ws_bytes);
    hipLaunchKernelGGL(logit_rows_kernel<T>, dim3((unsigned)nwg), dim3(256), 0, st, X, N, ld, D, fold, label, coef, K, z_out, partials);
    AM_LAUNCH_CHECK();
    hipLaunchKernelGGL(logit_sums_kernel, dim3((unsigned)ceil_div(stride, (int64_t)256)), dim3(256), 0, st, (const double*)partials, nwg, stride,
                       sums, counts);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

}  // namespace am

using namespace am;

extern "C" size_t am_logit_pass_workspace_bytes(int64_t N, int D, int K) {
    if (N < 1 || D < 1 || D > 8192 || K < 1 || K > LG_MODELS) return 0;
    Carver c(nullptr, 0);
    c.take<double>((size_t)logit_grid(N) * ((size_t)K * (D + 2) + 2));
    return c.off;
}

extern "C" int am_logit_pass_f32(const float* X, int64_t N, int64_t ld, int D, const int32_t* fold, int label, const double* coef, int K,
                                 double* sums, double* z_out, double* counts, void* ws, size_t ws_bytes, am_stream_t stream) {
    return logit_pass<float>(X, N, ld, D, fold, label, coef, K, sums, z_out, counts, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int am_logit_pass_f64(const double* X, int64_t N, int64_t ld, int D, const int32_t* fold, int label, const double* coef, int K,
                                 double* sums, double* z_out, double* counts, void* ws, size_t ws_bytes, am_stream_t stream) {
    return logit_pass<double>(X, N, ld, D, fold, label, coef, K, sums, z_out, counts, ws, ws_bytes, static_cast<hipStream_t>(stream));
}
