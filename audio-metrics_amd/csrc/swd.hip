// Sliced Wasserstein distance: projections, a segmented key-only sort and the 1-D transport cost, each one entry point.
//
// PROJECT (am_sliced_project_f32): Z[l][i] = <theta_l, x_i> without norms and without a distance - the seventh epilogue of
// the exact f32 tile engine.  The plan is kmeans.hip's assign (dense_pipeline_early with the production schedule, the
// (row block) x (column chunk) plan of work_item / choose_chunks, the KTAIL instantiation for D % 32 != 0) with the
// directions on the Q side, where the centroids go, and the rows of X on the P side.  finish() stores the accumulators as
// they are: the lane index r runs along rows of X, so the store of one accumulator register is two runs of 32 consecutive
// floats of Z (one per half-wave, in two directions).  The k order of a dot product is the engine's and does not depend on
// the tile position: a projection has the same bits alone and among any other directions.
//
// SORT (am_sort_rows_f32): every row of an [L, N] matrix ascending, keys only.  LSD radix sort over the order-preserving
// transform of the bits, 8 bits per pass, 4 passes: in -> tmp -> out -> tmp -> out.  ONE workgroup of 16 waves owns a row
// from start to end; wave w owns the contiguous segment [w S, (w + 1) S) of whatever buffer a pass reads, S = ceil(N / 16)
// rounded up to 64.  A pass is
//   A  every wave counts the digits of its segment into its own 256 counters (integer LDS atomics: order-free)
//   -  the counters become start offsets by an exclusive scan in (digit, wave) order
//   B  every wave walks its segment again, 64 keys at a time: the lanes that share a digit find each other with eight
//      ballots, take consecutive slots from the wave's counter of that digit in lane order, and the lowest of them advances
//      the counter
// so keys of one digit keep their (wave, step, lane) order = their order in the source: the scatter is stable.  No wave
// waits for another inside a phase, there is no communication between workgroups, every trip count is a function of N and
// every __syncthreads sits in uniform control flow.  NaNs (either sign, any payload) get the largest key and come out as the
// canonical quiet NaN behind +inf; -0.0 sorts before +0.0.
//
// W (am_sliced_w_f32): the quantile coupling of two sorted rows on the merged grid {i / n} u {j / m}.  One thread per atom i
// of the LARGER side: it overlaps atoms floor(i nb / na) .. ceil((i + 1) nb / na) - 1 of the smaller one (at most two) with
// integer weights min((i + 1) nb, (j + 1) na) - max(i nb, j na), exact in int64 and in a double.  Terms, block sums and the
// row sum are f64 in a fixed order, divided by na nb once.  No floating-point atomics: two calls return the same bits.
#include "row_sweep.h"

namespace am {
namespace swd {

constexpr size_t PROJECT_LDS_BYTES = ENGINE_LDS_FLOATS * sizeof(float);

struct ProjectEpilogue {
    float* Z;
    int64_t ldz, n, nl, prow0;
    const LaneInfo& L;

    __device__ __forceinline__ ProjectEpilogue(const LaneInfo& l) : L(l) {}
    __device__ __forceinline__ void aux_issue(int, int64_t) {}
    __device__ __forceinline__ void aux_commit(int) {}
    // register 4 g + e of acc[mt][nt] <-> direction qtile * 128 + wm * 64 + mt * 32 + 8 g + 4 h + e, row prow0 + wn * 64 + nt * 32 + r
    __device__ __forceinline__ void finish(int, int64_t qtile, f32x16 (&acc)[2][2]) {
        const int64_t cbase = qtile * TB + L.wm * 64 + L.h * 4;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int64_t i = prow0 + L.wn * 64 + nt * 32 + L.r;
            if (i >= n) continue;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int64_t c = cbase + mt * 32 + (reg & 3) + 8 * (reg >> 2);
                    if (c < nl) Z[c * ldz + i] = acc[mt][nt][reg];
                }
            }
        }
    }
};

template <bool KTAIL>
__global__ void __launch_bounds__(ENGINE_THREADS, 2)
sliced_project_kernel(const float* __restrict__ X, int64_t N, int64_t ldx, const float* __restrict__ T, int64_t NL, int64_t ldt,
                      int D, int nchunks, float* __restrict__ Z, int64_t ldz) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LaneInfo L;
    const WorkItem w = work_item((NL + TB - 1) / TB, nchunks);
    ProjectEpilogue epi(L);
    epi.Z = Z;
    epi.ldz = ldz;
    epi.n = N;
    epi.nl = NL;
    epi.prow0 = w.prow0;
    dense_pipeline_early<EV_DEFAULT, KTAIL>(T, NL, ldt, LinearTiles{w.qtile0}, X, N, ldx, w.prow0, w.ntiles, D, lds, L, epi);
}

// ---- sort ----------------------------------------------------------------------------------------------------------------
constexpr int SORT_THREADS = 1024;
constexpr int SORT_WAVES = SORT_THREADS / 64;
constexpr int RADIX = 256;
constexpr unsigned NAN_KEY = 0xffffffffu;               // no number maps here: ~b needs b = +0 (no sign), b ^ 2^31 needs b = 0x7fffffff (a NaN)
constexpr unsigned NAN_BITS = 0x7fc00000u;

__device__ __forceinline__ unsigned key_of_bits(unsigned b) {
    if ((b & 0x7fffffffu) > 0x7f800000u) return NAN_KEY;
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ unsigned bits_of_key(unsigned u) {
    if (u == NAN_KEY) return NAN_BITS;
    return (u >> 31) ? (u ^ 0x80000000u) : ~u;
}

// `in` may be `out` (pass 0 has read all of it before pass 1 writes); tmp is a third buffer
__global__ void __launch_bounds__(SORT_THREADS)
sort_rows_kernel(const unsigned* in, int64_t ld_in, unsigned* out, int64_t ld_out, unsigned* __restrict__ tmp, int64_t ld_tmp,
                 int64_t N, int64_t seg) {
    __shared__ unsigned hist[SORT_WAVES * RADIX];       // [wave][digit]: counts, then the next free slot
    __shared__ unsigned tot[RADIX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = blockIdx.x;
    const unsigned* src0 = in + row * ld_in;
    unsigned* a = tmp + row * ld_tmp;
    unsigned* b = out + row * ld_out;
    const int64_t seg0 = (int64_t)wave * seg;
    const int64_t steps = seg / 64;                      // the same for every wave: a function of N
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned* mine = hist + wave * RADIX;

#pragma unroll 1
    for (int pass = 0; pass < 4; ++pass) {
        const unsigned* s = pass == 0 ? src0 : ((pass & 1) ? a : b);
        unsigned* d = (pass & 1) ? b : a;
        const int shift = pass * 8;
        for (int i = tid; i < SORT_WAVES * RADIX; i += SORT_THREADS) hist[i] = 0u;
        __syncthreads();
        // A: digit counts of the wave's segment
#pragma unroll 4
        for (int64_t it = 0; it < steps; ++it) {
            const int64_t idx = seg0 + it * 64 + lane;
            if (idx < N) {
                const unsigned v = s[idx];
                const unsigned u = pass == 0 ? key_of_bits(v) : v;
                atomicAdd(mine + ((u >> shift) & 255u), 1u);
            }
        }
        __syncthreads();
        // counts -> start offsets, exclusive in (digit, wave) order
        if (tid < RADIX) {
            unsigned run = 0u;
#pragma unroll
            for (int w = 0; w < SORT_WAVES; ++w) {
                const unsigned c = hist[w * RADIX + tid];
                hist[w * RADIX + tid] = run;
                run += c;
            }
            tot[tid] = run;
        }
        __syncthreads();
        if (wave == 0) {                                 // one wave scans the 256 totals, four per lane
            unsigned t[4], sum = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                t[e] = tot[lane * 4 + e];
                sum += t[e];
            }
            unsigned incl = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned up = __shfl_up(incl, o);
                if (lane >= o) incl += up;
            }
            unsigned run = incl - sum;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                tot[lane * 4 + e] = run;
                run += t[e];
            }
        }
        __syncthreads();
        for (int i = tid; i < SORT_WAVES * RADIX; i += SORT_THREADS) hist[i] += tot[i & (RADIX - 1)];
        __syncthreads();
        // B: stable scatter of the wave's segment
        int64_t idx = seg0 + lane;
        unsigned v = idx < N ? s[idx] : 0u;
#pragma unroll 1
        for (int64_t it = 0; it < steps; ++it) {
            const int64_t nidx = idx + 64;
            const unsigned nv = (it + 1 < steps && nidx < N) ? s[nidx] : 0u;      // the next step's key, in flight under this one
            const bool active = idx < N;
            const unsigned u = pass == 0 ? key_of_bits(v) : v;
            const unsigned digit = (u >> shift) & 255u;
            unsigned long long same = __builtin_amdgcn_ballot_w64(active);
#pragma unroll
            for (int bit = 0; bit < 8; ++bit) {
                const bool one = (digit >> bit) & 1u;
                const unsigned long long m = __builtin_amdgcn_ballot_w64(one);
                same &= one ? m : ~m;
            }
            const unsigned rank = (unsigned)__popcll(same & below);
            const unsigned start = mine[digit];
            __builtin_amdgcn_wave_barrier();              // every lane has read the counter before its first lane advances it
            if (active) {
                if (rank == 0u) mine[digit] = start + (unsigned)__popcll(same);
                const unsigned pos = start + rank;
                if (pos < (unsigned long long)N) d[pos] = pass == 3 ? bits_of_key(u) : u;     // (always true: the counts add up to N)
            }
            __builtin_amdgcn_wave_barrier();
            v = nv;
            idx = nidx;
        }
        __syncthreads();                                 // the pass's stores are visible to the workgroup's next pass
    }
}

// ---- W -------------------------------------------------------------------------------------------------------------------
constexpr int W_THREADS = 256;

__device__ __forceinline__ bool finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// fixed-shape trees over the workgroup's values: the same order of additions on every call
__device__ __forceinline__ void block_sums_256(double& v, int& c, double* sv, int* sc) {
    sv[threadIdx.x] = v;
    sc[threadIdx.x] = c;
    __syncthreads();
#pragma unroll
    for (int w = W_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            sv[threadIdx.x] += sv[threadIdx.x + w];
            sc[threadIdx.x] += sc[threadIdx.x + w];
        }
        __syncthreads();
    }
    v = sv[0];
    c = sc[0];
}

// A: the larger side (na atoms per row), B: the other one (nb <= na); part[row * nblk + block] = sum of weight * |a - b|^p
template <int P>
__global__ void __launch_bounds__(W_THREADS)
sliced_w_kernel(const float* __restrict__ A, int64_t lda, int64_t na, const float* __restrict__ B, int64_t ldb, int64_t nb,
                int64_t nblk, double* __restrict__ part, int* __restrict__ cpart) {
    __shared__ double sv[W_THREADS];
    __shared__ int sc[W_THREADS];
    const int64_t row = blockIdx.x / nblk, blk = blockIdx.x - row * nblk;
    const int64_t i = blk * W_THREADS + threadIdx.x;
    const float* a = A + row * lda;
    const float* b = B + row * ldb;
    double v = 0.0;
    int bad = 0;
    if (i < na) {
        const float ai = a[i];
        bad += finite_f32(ai) ? 0 : 1;
        if (i < nb) bad += finite_f32(b[i]) ? 0 : 1;
        const int64_t lo_i = i * nb, hi_i = lo_i + nb;                     // the atom's interval, in units of 1 / (na nb)
        const int64_t j0 = lo_i / na, j1 = (hi_i + na - 1) / na - 1;       // j1 - j0 <= 1 because nb <= na
        for (int64_t j = j0; j <= j1 && j < nb; ++j) {
            const int64_t lo_j = j * na, hi_j = lo_j + na;
            const int64_t wgt = (hi_i < hi_j ? hi_i : hi_j) - (lo_i > lo_j ? lo_i : lo_j);
            const double diff = fabs((double)ai - (double)b[j]);
            v += (double)wgt * (P == 1 ? diff : diff * diff);
        }
    }
    block_sums_256(v, bad, sv, sc);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = v;
        cpart[blockIdx.x] = bad;
    }
}

// one workgroup per row: its block sums in a fixed tree, the division, NaN for a row that holds a non-finite value
__global__ void __launch_bounds__(W_THREADS)
sliced_w_finish_kernel(const double* __restrict__ part, const int* __restrict__ cpart, int64_t nblk, double scale,
                       double* __restrict__ out, int32_t* __restrict__ nonfinite) {
    __shared__ double sv[W_THREADS];
    __shared__ int sc[W_THREADS];
    const int64_t row = blockIdx.x;
    double v = 0.0;
    int bad = 0;
    for (int64_t j = threadIdx.x; j < nblk; j += W_THREADS) {
        v += part[row * nblk + j];
        bad += cpart[row * nblk + j];
    }
    block_sums_256(v, bad, sv, sc);
    if (threadIdx.x == 0) {
        out[row] = bad > 0 ? __longlong_as_double(0x7ff8000000000000ll) : v / scale;
        nonfinite[row] = bad;
    }
}

static bool project_shape_ok(int64_t N, int64_t L, int D) {
    return sweep_shape_ok(N, L, D, COLUMNS_ANY);
}
static int64_t sort_tmp_ld(int64_t N) { return ceil_div(N, 4) * 4; }
static bool sort_shape_ok(int64_t L, int64_t N) {                                       // one workgroup per row; tmp of < 2^42 bytes
    return L >= 1 && L <= (int64_t)0x7fffffff && N >= 1 && N <= (int64_t)0x7fffffff && L <= ((int64_t)1 << 40) / sort_tmp_ld(N);
}
static bool w_shape_ok(int64_t L, int64_t n, int64_t m) {
    if (!(L >= 1 && n >= 1 && m >= 1 && n <= (int64_t)0x7fffffff && m <= (int64_t)0x7fffffff)) return false;
    if (n > (((int64_t)1 << 53) - 1) / m) return false;                                // the weights are exact while n m < 2^53
    return L <= (int64_t)0x7fffffff / ceil_div(n > m ? n : m, W_THREADS);
}

}  // namespace swd
}  // namespace am

using namespace am;

extern "C" int am_sliced_project_f32(const float* X, int64_t N, int64_t ldx, const float* Theta, int64_t L, int64_t ldt, int D,
                                     float* Z, int64_t ldz, am_stream_t stream) {
    int rc;
    if ((rc = check_matrix(X, N, ldx, D, "X")) != AM_OK) return rc;
    if ((rc = check_matrix(Theta, L, ldt, D, "Theta")) != AM_OK) return rc;
    AM_REQUIRE(Z != nullptr, AM_ERR_BAD_ARG, "Z is null");
    AM_REQUIRE(ldz >= N, AM_ERR_BAD_ARG, "ldz=%lld is smaller than N=%lld", (long long)ldz, (long long)N);
    AM_REQUIRE(swd::project_shape_ok(N, L, D), AM_ERR_BAD_SHAPE, "N=%lld L=%lld: too large for one launch", (long long)N,
               (long long)L);
    const int nchunks = choose_chunks(N, L);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return launch_sweep(&swd::sliced_project_kernel<false>, &swd::sliced_project_kernel<true>, swd::PROJECT_LDS_BYTES, N, nchunks, D, st, X,
                        N, ldx, Theta, L, ldt, D, nchunks, Z, ldz);
}

extern "C" size_t am_sort_rows_workspace_bytes(int64_t L, int64_t N) {
    if (!swd::sort_shape_ok(L, N)) return 0;
    Carver c(nullptr, 0);
    c.take<unsigned>((size_t)L * (size_t)swd::sort_tmp_ld(N));
    return c.off;
}

extern "C" int am_sort_rows_f32(const float* in, int64_t L, int64_t N, int64_t ld_in, float* out, int64_t ld_out, void* ws,
                                size_t ws_bytes, am_stream_t stream) {
    AM_REQUIRE(in != nullptr && out != nullptr, AM_ERR_BAD_ARG, "%s is null", in == nullptr ? "in" : "out");
    AM_REQUIRE(swd::sort_shape_ok(L, N), AM_ERR_BAD_SHAPE, "L=%lld N=%lld: rows of 1 .. 2^31 - 1 keys", (long long)L, (long long)N);
    AM_REQUIRE(ld_in >= N && ld_out >= N, AM_ERR_BAD_ARG, "row strides %lld and %lld must be at least N=%lld", (long long)ld_in,
               (long long)ld_out, (long long)N);
    const int64_t ld_tmp = swd::sort_tmp_ld(N);
    Carver c(ws, ws_bytes);
    unsigned* tmp = c.take<unsigned>((size_t)L * (size_t)ld_tmp);
    AM_REQUIRE(c.ok(), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (am_sort_rows_workspace_bytes), have %zu", c.off,
               ws_bytes);
    const int64_t seg = ceil_div(ceil_div(N, swd::SORT_WAVES), 64) * 64;
    hipLaunchKernelGGL(swd::sort_rows_kernel, dim3((unsigned)L), dim3(swd::SORT_THREADS), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const unsigned*>(in), ld_in, reinterpret_cast<unsigned*>(out), ld_out, tmp, ld_tmp, N, seg);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

extern "C" size_t am_sliced_w_workspace_bytes(int64_t L, int64_t n, int64_t m) {
    if (!swd::w_shape_ok(L, n, m)) return 0;
    const size_t cells = (size_t)L * (size_t)ceil_div(n > m ? n : m, swd::W_THREADS);
    Carver c(nullptr, 0);
    c.take<double>(cells);
    c.take<int>(cells);
    return c.off;
}

extern "C" int am_sliced_w_f32(const float* Zx, int64_t n, int64_t ldzx, const float* Zy, int64_t m, int64_t ldzy, int64_t L, int p,
                               double* out, int32_t* nonfinite, void* ws, size_t ws_bytes, am_stream_t stream) {
    AM_REQUIRE(Zx != nullptr && Zy != nullptr && out != nullptr && nonfinite != nullptr, AM_ERR_BAD_ARG, "%s is null",
               Zx == nullptr ? "Zx" : Zy == nullptr ? "Zy" : out == nullptr ? "out" : "nonfinite");
    AM_REQUIRE(p == 1 || p == 2, AM_ERR_BAD_ARG, "p=%d must be 1 or 2", p);
    AM_REQUIRE(swd::w_shape_ok(L, n, m), AM_ERR_BAD_SHAPE, "L=%lld n=%lld m=%lld: rows of 1 .. 2^31 - 1 atoms with n m < 2^53",
               (long long)L, (long long)n, (long long)m);
    AM_REQUIRE(ldzx >= n && ldzy >= m, AM_ERR_BAD_ARG, "row strides %lld and %lld must be at least n=%lld and m=%lld",
               (long long)ldzx, (long long)ldzy, (long long)n, (long long)m);
    // the larger side gets the threads; equal sizes keep the argument order (the coupling is then atom i with atom i)
    const bool swap = m > n;
    const float* A = swap ? Zy : Zx;
    const float* B = swap ? Zx : Zy;
    const int64_t na = swap ? m : n, nb = swap ? n : m, lda = swap ? ldzy : ldzx, ldb = swap ? ldzx : ldzy;
    const int64_t nblk = ceil_div(na, swd::W_THREADS);
    Carver c(ws, ws_bytes);
    double* part = c.take<double>((size_t)L * (size_t)nblk);
    int* cpart = c.take<int>((size_t)L * (size_t)nblk);
    AM_REQUIRE(c.ok(), AM_ERR_WORKSPACE, "workspace too small: need %zu bytes (am_sliced_w_workspace_bytes), have %zu", c.off,
               ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (p == 1)
        hipLaunchKernelGGL(swd::sliced_w_kernel<1>, dim3((unsigned)(L * nblk)), dim3(swd::W_THREADS), 0, st, A, lda, na, B, ldb, nb, nblk,
                           part, cpart);
    else
        hipLaunchKernelGGL(swd::sliced_w_kernel<2>, dim3((unsigned)(L * nblk)), dim3(swd::W_THREADS), 0, st, A, lda, na, B, ldb, nb, nblk,
                           part, cpart);
    AM_LAUNCH_CHECK();
    hipLaunchKernelGGL(swd::sliced_w_finish_kernel, dim3((unsigned)L), dim3(swd::W_THREADS), 0, st, (const double*)part,
                       (const int*)cpart, nblk, (double)na * (double)nb, out, nonfinite);
    AM_LAUNCH_CHECK();
    return AM_OK;
}
