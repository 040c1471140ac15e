// The two 256-row f16 FILTER kernels of the PRDC path on the OPERAND-STATIONARY engine (pstat_engine.h): the bodies of
// wide_kernels.h - membership filter, symmetric k-NN sweep - with the workgroup's P block held in registers for the whole
// work item and only Q slabs streaming through LDS.  Rows of up to 512 f16 (D <= 512); wider sets keep wide_engine.h
// (pairwise_wide.hip).  Same queue protocol, same results (the 16x16x32 body: other accumulator values); its own translation unit so
// that the three PRDC objects compile in parallel.
#include "wide_kernels.h"
#include "pstat_engine.h"
#include <type_traits>

namespace am {

// S16: the 16x16x32 body of the engine (Pstat16Body) instead of the 32x32x16 one.  Which instantiations take it is decided
// here, per kernel: a body switches where it stays inside the register file and was measured faster at its width
// (profiles/mfma_shape/).  The membership filter at KSLABS = 8 without row minima does (255 registers).  The k-NN sweep at
// KSLABS = 8 does not fit: two 16-row P tiles per lane double its lane-local lists and per-row state, and the KCAP = 6 body
// came out at 256 registers plus 60 bytes of scratch (KCAP = 11 used every register before).  Everything else keeps the 32-shape
// until it is measured.
template <int KSLABS, bool S16 = false>
struct PstatEng {
    using Lane = std::conditional_t<S16, P16Lane, PLane>;
    static constexpr int LDS_WORDS = pstat_lds_words(KSLABS);
    static constexpr bool cross16(bool want_min) { return KSLABS == 8 && !want_min; }
    static constexpr bool knn16(int) { return false; }
    template <class TileMap, class Epi>
    static __device__ __forceinline__ void run(const float* Q, int64_t nq, int64_t ldq, const TileMap& tm, const float* P, int64_t np,
                                               int64_t ldp, int64_t prow0, int ntiles, int, float* lds, Lane& L, Epi& epi) {
        pstat_pipeline<std::conditional_t<S16, Pstat16Body<KSLABS>, Pstat32Body<KSLABS>>>(Q, nq, ldq, tm, P, np, ldp, prow0, ntiles, lds, L, epi);
    }
};
template <int KSLABS, bool WANT_MIN> using CrossPstatEng = PstatEng<KSLABS, PstatEng<KSLABS>::cross16(WANT_MIN)>;
template <int KSLABS, int KCAP> using KnnPstatEng = PstatEng<KSLABS, PstatEng<KSLABS>::knn16(KCAP)>;

// rows of up to P64_MAX_SLABS slabs (D <= 128): 256 threads, two workgroups per CU, a wave = 64 P rows x 64-row Q units
template <int KSLABS>
struct Pstat64Eng {
    using Lane = P64Lane;
    static constexpr int LDS_WORDS = pstat64_lds_words();
    template <class TileMap, class Epi>
    static __device__ __forceinline__ void run(const float* Q, int64_t nq, int64_t ldq, const TileMap& tm, const float* P, int64_t np,
                                               int64_t ldp, int64_t prow0, int ntiles, int, float* lds, Lane& L, Epi& epi) {
        pstat_pipeline<Pstat64Body<KSLABS>>(Q, nq, ldq, tm, P, np, ldp, prow0, ntiles, lds, L, epi);
    }
};

template <int KSLABS, bool WANT_MIN>
__global__ void __launch_bounds__(PTHREADS, 1)
cross_pstat_kernel(const float* __restrict__ Rb, int64_t Nr, int64_t ldr, const float* __restrict__ rnorm,
                   const float* __restrict__ rthr, const float* __restrict__ Cb, int64_t Nc, int64_t ldc,
                   const float* __restrict__ cnorm, const float* __restrict__ cthr, int Dh, int nchunks, int grp_rows,
                   const unsigned* __restrict__ maxn, unsigned* __restrict__ rmin_approx, unsigned* __restrict__ row_any,
                   unsigned* __restrict__ row_cover, int32_t* __restrict__ col_count, uint2* __restrict__ wgq, int qcap,
                   int* __restrict__ wgq_count, uint2* __restrict__ items, uint2* __restrict__ ovq, int* __restrict__ ov_count,
                   int ovcap, int* __restrict__ fail, float fc) {
    cross_wide_body<CrossPstatEng<KSLABS, WANT_MIN>, WANT_MIN>(Rb, Nr, ldr, rnorm, rthr, Cb, Nc, ldc, cnorm, cthr, Dh, nchunks, grp_rows, maxn, rmin_approx,
                                                row_any, row_cover, col_count, wgq, qcap, wgq_count, items, ovq, ov_count, ovcap, fail, fc);
}

template <int KSLABS, int KCAP>
__global__ void __launch_bounds__(PTHREADS, 1)
knn_pstat_kernel(const float* __restrict__ Xb, int64_t N, int64_t ldh, const float* __restrict__ xnorm, float* thr, int Dh,
                 int win_tiles, int nwin, int per_win, int k1, const unsigned* __restrict__ maxn, float* __restrict__ partial,
                 int* __restrict__ cnt, int cap, uint2* __restrict__ wgq, float* __restrict__ wgv, int qcap,
                 int* __restrict__ wgq_count, int part, int nparts, float fc, uint2* __restrict__ ovq, float* __restrict__ ovv,
                 unsigned long long* __restrict__ ovn, int ovcap, const int* __restrict__ skip, int* __restrict__ region_counter) {
    knn_wide_body<KnnPstatEng<KSLABS, KCAP>, KCAP>(Xb, N, ldh, xnorm, thr, Dh, win_tiles, nwin, per_win, k1, maxn, partial, cnt, cap, wgq, wgv, qcap,
                                          wgq_count, part, nparts, fc, ovq, ovv, ovn, ovcap, skip, region_counter);
}

template <int KSLABS, bool WANT_MIN>
__global__ void __launch_bounds__(P64_THREADS, 2)
cross_pstat64_kernel(const float* __restrict__ Rb, int64_t Nr, int64_t ldr, const float* __restrict__ rnorm,
                     const float* __restrict__ rthr, const float* __restrict__ Cb, int64_t Nc, int64_t ldc,
                     const float* __restrict__ cnorm, const float* __restrict__ cthr, int Dh, int nchunks, int grp_rows,
                     const unsigned* __restrict__ maxn, unsigned* __restrict__ rmin_approx, unsigned* __restrict__ row_any,
                     unsigned* __restrict__ row_cover, int32_t* __restrict__ col_count, uint2* __restrict__ wgq, int qcap,
                     int* __restrict__ wgq_count, uint2* __restrict__ items, uint2* __restrict__ ovq, int* __restrict__ ov_count,
                     int ovcap, int* __restrict__ fail, float fc) {
    cross_wide_body<Pstat64Eng<KSLABS>, WANT_MIN>(Rb, Nr, ldr, rnorm, rthr, Cb, Nc, ldc, cnorm, cthr, Dh, nchunks, grp_rows, maxn, rmin_approx,
                                                  row_any, row_cover, col_count, wgq, qcap, wgq_count, items, ovq, ov_count, ovcap, fail, fc);
}

template <int KSLABS, int KCAP>
__global__ void __launch_bounds__(P64_THREADS, 2)
knn_pstat64_kernel(const float* __restrict__ Xb, int64_t N, int64_t ldh, const float* __restrict__ xnorm, float* thr, int Dh,
                   int win_tiles, int nwin, int per_win, int k1, const unsigned* __restrict__ maxn, float* __restrict__ partial,
                   int* __restrict__ cnt, int cap, uint2* __restrict__ wgq, float* __restrict__ wgv, int qcap,
                   int* __restrict__ wgq_count, int part, int nparts, float fc, uint2* __restrict__ ovq, float* __restrict__ ovv,
                   unsigned long long* __restrict__ ovn, int ovcap, const int* __restrict__ skip, int* __restrict__ region_counter) {
    knn_wide_body<Pstat64Eng<KSLABS>, KCAP>(Xb, N, ldh, xnorm, thr, Dh, win_tiles, nwin, per_win, k1, maxn, partial, cnt, cap, wgq, wgv, qcap,
                                            wgq_count, part, nparts, fc, ovq, ovv, ovn, ovcap, skip, region_counter);
}

// which of the two stationary forms a row length takes: a pure function of the width (AM_PSTAT64=0 in the A/B build: the
// 512-thread form for every width)
static bool pstat64_takes(int kslabs) {
    static const int on = env_int("AM_PSTAT64", 1);
    return on != 0 && kslabs <= P64_MAX_SLABS;
}

#ifdef AM_DEV_KNOBS
// AM_WIDE_DBG -> this translation unit's copy of g_wide_dbg (1: every Q tile read from the first 2 MB, 2: epilogues skipped)
static hipError_t set_pstat_dev_symbols(hipStream_t st) {
    const int wdbg = env_int("AM_WIDE_DBG", 0);
    return hipMemcpyToSymbolAsync(HIP_SYMBOL(g_wide_dbg), &wdbg, sizeof(int), 0, hipMemcpyHostToDevice, st);
}
#endif

// rows of Dh words (Dh % 32 == 0): the stationary form holds KSLABS = Dh / 32 slabs of a row in registers
bool pstat_supported(int Dh) { return Dh % WROW == 0 && Dh / WROW >= 1 && Dh / WROW <= 8; }
bool pstat64_supported(int Dh) { return pstat_supported(Dh) && pstat64_takes(Dh / WROW); }

// the one launch of this file: `kernel` on `blocks` workgroups of `threads` with `lds_bytes` of dynamic LDS
template <class... Params, class... Args>
static int launch_pstat(void (*kernel)(Params...), unsigned blocks, int threads, size_t lds_bytes, hipStream_t st, Args... args) {
    AM_HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), (int)lds_bytes));
#ifdef AM_DEV_KNOBS
    AM_HIP_TRY(set_pstat_dev_symbols(st));
#endif
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds_bytes, st, args...);
    AM_LAUNCH_CHECK();
    return AM_OK;
}

int launch_cross_pstat(bool want_min, unsigned blocks, const float* Rb, int64_t Nr, int64_t ldr, const float* rnorm, const float* rthr,
                       const float* Cb, int64_t Nc, int64_t ldc, const float* cnorm, const float* cthr, int Dh, int nchunks,
                       int grp_rows, const unsigned* maxn, unsigned* rmin_approx, unsigned* row_any, unsigned* row_cover,
                       int32_t* col_count, uint2* wgq, int qcap, int* wgq_count, uint2* items, uint2* ovq, int* ov_count, int ovcap,
                       int* fail, float fc, hipStream_t st) {
    const auto launch = [&](auto* kernel, int threads, size_t lds_bytes) {
        return launch_pstat(kernel, blocks, threads, lds_bytes, st, Rb, Nr, ldr, rnorm, rthr, Cb, Nc, ldc, cnorm, cthr, Dh, nchunks, grp_rows,
                            maxn, rmin_approx, row_any, row_cover, col_count, wgq, qcap, wgq_count, items, ovq, ov_count, ovcap, fail, fc);
    };
    // (the LDS of a kernel is a function of its engine's form and KSLABS alone)
#define AM_PSTAT_CROSS(KERNEL, ENG, THREADS, KS)                                                                       \
    case KS:                                                                                                          \
        return want_min ? launch(&KERNEL<KS, true>, THREADS, wide_cross_lds_bytes<ENG<KS>>())                          \
                        : launch(&KERNEL<KS, false>, THREADS, wide_cross_lds_bytes<ENG<KS>>());
    if (pstat64_takes(Dh / WROW)) {
        switch (Dh / WROW) { AM_PSTAT_CROSS(cross_pstat64_kernel, Pstat64Eng, P64_THREADS, 1) AM_PSTAT_CROSS(cross_pstat64_kernel, Pstat64Eng, P64_THREADS, 2) }
    }
#define AM_PSTAT512_CROSS(KS) AM_PSTAT_CROSS(cross_pstat_kernel, PstatEng, PTHREADS, KS)
    switch (Dh / WROW) {
        AM_PSTAT512_CROSS(1) AM_PSTAT512_CROSS(2) AM_PSTAT512_CROSS(3) AM_PSTAT512_CROSS(4)
        AM_PSTAT512_CROSS(5) AM_PSTAT512_CROSS(6) AM_PSTAT512_CROSS(7) AM_PSTAT512_CROSS(8)
    }
#undef AM_PSTAT512_CROSS
#undef AM_PSTAT_CROSS
    set_error("the operand-stationary membership filter holds rows of up to 512 f16 (got %d words)", Dh);
    return AM_ERR_BAD_SHAPE;
}

int launch_knn_pstat(int kcap, unsigned nwg, const float* Xb, int64_t N, int64_t ldh, const float* xnorm, float* thr, int Dh,
                     int win_tiles, int nwin, int per_win, int k1, const unsigned* maxn, float* partial, int* cnt, int cap,
                     uint2* wgq, float* wgv, int qcap, int* wgq_count, int part, int nparts, float fc, uint2* ovq, float* ovv,
                     unsigned long long* ovn, int ovcap, const int* skip, int* region_counter, hipStream_t st) {
    AM_REQUIRE(kcap == 6 || kcap == 11, AM_ERR_UNSUPPORTED_K, "the 256-row k-NN sweep holds lists of 6 or 11 entries (got %d)", kcap);
    const auto launch = [&](auto* kernel, int threads, size_t lds_bytes) {
        return launch_pstat(kernel, nwg, threads, lds_bytes, st, Xb, N, ldh, xnorm, thr, Dh, win_tiles, nwin, per_win, k1, maxn, partial, cnt, cap,
                            wgq, wgv, qcap, wgq_count, part, nparts, fc, ovq, ovv, ovn, ovcap, skip, region_counter);
    };
#define AM_PSTAT_KNN(KERNEL, ENG, THREADS, KS)                                                                         \
    case KS:                                                                                                          \
        return kcap == 6 ? launch(&KERNEL<KS, 6>, THREADS, knn_wide_lds_bytes<ENG<KS>>())                              \
                         : launch(&KERNEL<KS, 11>, THREADS, knn_wide_lds_bytes<ENG<KS>>());
    if (pstat64_takes(Dh / WROW)) {
        switch (Dh / WROW) { AM_PSTAT_KNN(knn_pstat64_kernel, Pstat64Eng, P64_THREADS, 1) AM_PSTAT_KNN(knn_pstat64_kernel, Pstat64Eng, P64_THREADS, 2) }
    }
#define AM_PSTAT512_KNN(KS) AM_PSTAT_KNN(knn_pstat_kernel, PstatEng, PTHREADS, KS)
    switch (Dh / WROW) {
        AM_PSTAT512_KNN(1) AM_PSTAT512_KNN(2) AM_PSTAT512_KNN(3) AM_PSTAT512_KNN(4)
        AM_PSTAT512_KNN(5) AM_PSTAT512_KNN(6) AM_PSTAT512_KNN(7) AM_PSTAT512_KNN(8)
    }
#undef AM_PSTAT512_KNN
#undef AM_PSTAT_KNN
    set_error("the operand-stationary k-NN sweep holds rows of up to 512 f16 (got %d words)", Dh);
    return AM_ERR_BAD_SHAPE;
}

}  // namespace am
