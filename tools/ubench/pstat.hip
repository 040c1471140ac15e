// Microbenchmark of an OPERAND-STATIONARY stage for the f16 filter kernels: a workgroup's P block
// (256 rows x D = 512 f16) is loaded ONCE into registers as MFMA B fragments and never moves again; only 128-row Q slabs
// (128 rows x 64 f16 = 16 KB per stage) stream through an LDS ring by LDS-DMA.  Per 8.4 MFLOP of a CU (what one stage of
// csrc/wide_engine.h multiplies) the load path moves 32 KB instead of 64 KB and a wave reads Q fragments only.
//   NW = 4: four waves (one per SIMD, 512 registers), each 64 P rows (256 fragment registers) x 128 Q rows (128 accumulators)
//   NW = 8: eight waves (two per SIMD, 256 registers), each 32 P rows (128 fragment registers) x 128 Q rows (64 accumulators)
//   LAG = 1: the barrier at the end of stage g publishes stage g+1 (first fragment reads of a stage wait behind the barrier)
//   LAG = 2: it publishes stage g+2, so the first fragments of stage g+1 are read under the last MFMAs of stage g
// Data are meaningless; only the instruction mix, the LDS traffic and the fill traffic count.  Same source patterns and the
// same unit (us per 8.4 MFLOP per CU) as stage_sched.hip, so the numbers compare directly (adopted schedule there:
// 1.73-1.85 us L2-resident, 2.00-2.17 us from a 200 MB source).
// `pstat shape [reps]` runs the MFMA-shape A/B instead (32x32x16 against 16x16x32, see pstat16 below).
// Build: hipcc --offload-arch=gfx950 -O3 pstat.hip -o pstat
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int WROW = 32;                 // LDS row: 32 words = 128 B = 64 f16
constexpr int QROWS = 128;               // Q rows per stage
constexpr int STAGE_WORDS = QROWS * WROW;   // 16 KB
constexpr int KSTEPS = 32;               // D = 512 f16 = 32 MFMA k-steps of 16

template <int N>
__device__ __forceinline__ void wait_vm() {
    static_assert(N < 64, "vmcnt");
    __builtin_amdgcn_s_waitcnt(0x0F70 | (N & 15) | ((N >> 4) << 14));
}

// ABL (ablation bits, timing only - results are meaningless with any of 1 / 2 / 4 set): 1 no LDS-DMA, 2 no fragment reads behind
// the first, 4 no barrier, 8 waves 4-7 issue their pieces one k-step behind waves 0-3, 16 s_setprio 1 around the MFMAs,
// 32 a barrier every SECOND stage only
template <int NW, int LAG, int ROT, int ABL = 0>
__global__ void __launch_bounds__(NW * 64, 1) pstat(const float* __restrict__ src, int64_t src_rows, int ld_words, int tiles,
                                                      float* __restrict__ out, unsigned long long* __restrict__ clk = nullptr) {
    constexpr int NP = 8 / NW;                        // 32-row P tiles per wave: 2 (four waves) or 1 (eight waves)
    constexpr int PIECES = 16 / NW;                   // 1 KB LDS-DMA pieces per wave and stage
    constexpr int DEPTH = LAG + 1;                    // stages in flight ahead of the one being multiplied
    constexpr int RING = 4;
    static_assert(DEPTH < RING, "ring");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int64_t nblk = src_rows / 512;

    // ---- the stationary operand: NP x 32 fragments of 16 B per lane
    f32x4 pf[NP][KSTEPS];
    {
        const int64_t pblk = ((int64_t)blockIdx.x * 5 + 3) % nblk;
        const float* prow = src + (pblk * 512 + wave * (32 * NP) + r) * (int64_t)ld_words + h * 4;
#pragma unroll
        for (int n = 0; n < NP; ++n)
#pragma unroll
            for (int s = 0; s < KSTEPS; ++s) pf[n][s] = *reinterpret_cast<const f32x4*>(prow + (int64_t)n * 32 * ld_words + s * 8);
    }

    // ---- Q slabs by LDS-DMA: piece p = 8 rows x 128 B; this wave's pieces are p = wave * PIECES + i
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, (int)0x7fffffff, 0x00020000);
    const int lr = lane >> 3, slot = lane & 7;
    unsigned vo[2];                                    // even / odd piece (the swizzle of a row depends on (row >> 1) & 7)
#pragma unroll
    for (int par = 0; par < 2; ++par) {
        const int row = par * 8 + lr;
        vo[par] = (unsigned)((row * ld_words + (slot ^ ((row >> 1) & 7)) * 4) * 4);
    }
    // the 512-row source block a Q tile reads: a 32-bit walk (a 64-bit modulo per stage would cost more SALU than the stage)
    const unsigned nb = (unsigned)nblk, blk_bytes = (unsigned)(512 * ld_words * 4);
    unsigned blk_cur = (unsigned)(((int64_t)blockIdx.x * 7) % nblk), blk_next = blk_cur;
    auto piece = [&](int ring_slot, bool next_tile, int kslab, int i) {
        if (ABL & 1) return;
        const int p = wave * PIECES + i;
        float* dst = lds + ring_slot * STAGE_WORDS + p * 8 * WROW;
        const unsigned so = (next_tile ? blk_next : blk_cur) * blk_bytes + (unsigned)(kslab * 128) + (unsigned)((p & ~1) * 8 * ld_words * 4);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)dst, 16, (int)vo[p & 1], (int)so, 0, 0);
    };

    const int sw = (r >> 1) & 7;
    int coff[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) coff[c] = ((2 * c + h) ^ sw) * 4;
    const int qrow = r * WROW;
    auto qfrags = [&](f32x4 (&q)[4], int ring_slot, int c) {
        const float* st = lds + ring_slot * STAGE_WORDS;
#pragma unroll
        for (int m = 0; m < 4; ++m) q[m] = *reinterpret_cast<const f32x4*>(st + qrow + m * 32 * WROW + coff[c]);
    };

    f32x16 acc[4][NP];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < NP; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

    const int G = tiles * 8;
    // prologue: DEPTH stages in flight, the first LAG of them landed and published
#pragma unroll
    for (int g = 0; g < DEPTH; ++g)
#pragma unroll
        for (int i = 0; i < PIECES; ++i) piece(g % RING, false, g, i);
    wait_vm<(DEPTH - LAG) * PIECES>();
    __builtin_amdgcn_s_barrier();

    f32x4 qa[4], qb[4];
    qfrags(qa, 0, 0);
    auto qfrag1 = [&](int ring_slot, int c, int m) -> f32x4 {
        return *reinterpret_cast<const f32x4*>(lds + ring_slot * STAGE_WORDS + qrow + m * 32 * WROW + coff[c]);
    };
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), w0 = __builtin_amdgcn_s_memrealtime();
    for (int t = 0; t < tiles; ++t) {
        blk_cur = blk_next;
        blk_next = blk_cur + 13 >= nb ? blk_cur + 13 - nb : blk_cur + 13;
#pragma unroll
        for (int s8 = 0; s8 < 8; ++s8) {
            if (ABL & 16) __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (ROT) {
                    // ONE fragment set: the fragment of row tile m for the next k-step is read right behind the MFMAs that used it
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
#pragma unroll
                        for (int n = 0; n < NP; ++n)
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, qa[m]),
                                                                                 __builtin_bit_cast(f16x8, pf[n][s8 * 4 + c]), acc[m][n], 0, 0, 0);
                        if (!(ABL & 2)) {
                            if (c < 3) qa[m] = qfrag1(s8 % RING, c + 1, m);
                            else if (LAG == 2) qa[m] = qfrag1((s8 + 1) % RING, 0, m);
                        }
                        if (PIECES == 4 && m == 1) piece((s8 + DEPTH) % RING, s8 + DEPTH >= 8, (s8 + DEPTH) & 7, c);
                        if (PIECES == 2 && !(ABL & 8) && m == 1 && (c & 1) == 0) piece((s8 + DEPTH) % RING, s8 + DEPTH >= 8, (s8 + DEPTH) & 7, c >> 1);
                        if (PIECES == 2 && (ABL & 8) && m == 1) {
                            if (wave < 4 ? (c & 1) == 0 : (c & 1) == 1) piece((s8 + DEPTH) % RING, s8 + DEPTH >= 8, (s8 + DEPTH) & 7, c >> 1);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    continue;
                }
                f32x4 (&cur)[4] = (c & 1) ? qb : qa;
                f32x4 (&nxt)[4] = (c & 1) ? qa : qb;
                if (c < 3) qfrags(nxt, s8 % RING, c + 1);
                else if (LAG == 2) qfrags(nxt, (s8 + 1) % RING, 0);          // published by the barrier of stage g - 1
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
#pragma unroll
                    for (int n = 0; n < NP; ++n)
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, cur[m]),
                                                                             __builtin_bit_cast(f16x8, pf[n][s8 * 4 + c]), acc[m][n], 0, 0, 0);
                    if (PIECES == 4 && m == 1) piece((s8 + DEPTH) % RING, s8 + DEPTH >= 8, (s8 + DEPTH) & 7, c);
                    if (PIECES == 2 && m == 1 && (c & 1) == 0) piece((s8 + DEPTH) % RING, s8 + DEPTH >= 8, (s8 + DEPTH) & 7, c >> 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (ABL & 16) __builtin_amdgcn_s_setprio(0);
            // stage g + LAG has landed (this wave's pieces); the barrier publishes it
            wait_vm<(DEPTH - LAG) * PIECES>();
            if (!(ABL & 4) && (!(ABL & 32) || (s8 & 1))) __builtin_amdgcn_s_barrier();
            if (LAG == 1) {
                qfrags(qa, (s8 + 1) % RING, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (G < 0) break;
    }
    if (clk != nullptr && tid == 0) {                 // the shape A/B below: cycles and 100-MHz ticks of the main loop
        clk[blockIdx.x * 2] = __builtin_amdgcn_s_memtime() - t0;
        clk[blockIdx.x * 2 + 1] = __builtin_amdgcn_s_memrealtime() - w0;
    }
    float sink = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < NP; ++b) sink += acc[a][b][5];
    sink += qa[0].x;
    if (!ROT) sink += qb[0].x;
    if (sink == 12345.678f) out[0] = sink;
}

// ---- MFMA shape A/B (NW = 8, LAG = 2, ROT = 1 only): the same stage on v_mfma_f32_16x16x32_f16 against the kernel above.
// SHAPE 16: wave w owns the same 32 P rows as TWO 16-row tiles; lane = (r = lane & 15, g = lane >> 4); the B fragment of the
// k-step of 32 elements is the 16 B at element offset 8 g (16 fragments of 16 B per row tile: 128 registers, as above).  The
// stage's 128 Q rows are EIGHT 16-row tiles and two k-steps: 16 ds_read_b128 per wave and stage, as above, each feeding two
// MFMAs; the lane reads chunk (4 c + g) ^ ((r >> 1) & 7) of row 16 mt + r.  Every ds_read_b128 lane group of the wave lands on
// sixteen distinct 16-B columns of the swizzled image: the column is 8 (r & 1) + ((4 c + g) ^ s) with s = (r >> 1) & 7, a group
// holds every s twice (r even and odd) with g = g0 for s in {0, 1, 6, 7} and g0 ^ 1 for s in {2 .. 5} (g0 = 0 or 1 in the low
// half of the wave, 2 or 3 in the high half), and s -> (g(s) ^ s) is a bijection of 0 .. 7 for either g0.
// 32 MFMAs of 16 cycles per wave and stage; a ring of FOUR fragment registers: the fragment of tile mt + 4 is read right behind
// the MFMAs of tile mt, the same three-MFMA-gaps (96 cycles) lead as the one-behind rotation above; the two LDS-DMA pieces go
// behind tile 1 of either k-step, 64 and 320 cycles into the stage as above.
// Both kernels stamp s_memtime / s_memrealtime around the main loop (thread 0 of every workgroup, into a buffer of their own).
template <int ABL = 0>
__global__ void __launch_bounds__(512, 1) pstat16(const float* __restrict__ src, int64_t src_rows, int ld_words, int tiles,
                                                  float* __restrict__ out, unsigned long long* __restrict__ clk) {
    constexpr int PIECES = 2, DEPTH = 3, RING = 4, KS16 = 16;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int64_t nblk = src_rows / 512;

    f32x4 pf[2][KS16];
    {
        const int64_t pblk = ((int64_t)blockIdx.x * 5 + 3) % nblk;
        const float* prow = src + (pblk * 512 + wave * 32 + r) * (int64_t)ld_words + g * 4;
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int s = 0; s < KS16; ++s) pf[n][s] = *reinterpret_cast<const f32x4*>(prow + (int64_t)n * 16 * ld_words + s * 16);
    }

    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, (int)0x7fffffff, 0x00020000);
    const int lr = lane >> 3, slot = lane & 7;
    unsigned vo[2];
#pragma unroll
    for (int par = 0; par < 2; ++par) {
        const int row = par * 8 + lr;
        vo[par] = (unsigned)((row * ld_words + (slot ^ ((row >> 1) & 7)) * 4) * 4);
    }
    const unsigned nb = (unsigned)nblk, blk_bytes = (unsigned)(512 * ld_words * 4);
    unsigned blk_cur = (unsigned)(((int64_t)blockIdx.x * 7) % nblk), blk_next = blk_cur;
    auto piece = [&](int ring_slot, bool next_tile, int kslab, int i) {
        if (ABL & 1) return;
        const int p = wave * PIECES + i;
        float* dst = lds + ring_slot * STAGE_WORDS + p * 8 * WROW;
        const unsigned so = (next_tile ? blk_next : blk_cur) * blk_bytes + (unsigned)(kslab * 128) + (unsigned)((p & ~1) * 8 * ld_words * 4);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)dst, 16, (int)vo[p & 1], (int)so, 0, 0);
    };

    const int sw = (r >> 1) & 7;
    int coff[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) coff[c] = r * WROW + ((4 * c + g) ^ sw) * 4;
    auto qfrag = [&](int ring_slot, int c, int mt) -> f32x4 {
        return *reinterpret_cast<const f32x4*>(lds + ring_slot * STAGE_WORDS + mt * 16 * WROW + coff[c]);
    };

    f32x4 acc[8][2];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[a][b][i] = 0.f;

#pragma unroll
    for (int s = 0; s < DEPTH; ++s)
#pragma unroll
        for (int i = 0; i < PIECES; ++i) piece(s % RING, false, s, i);
    wait_vm<PIECES>();
    __builtin_amdgcn_s_barrier();

    f32x4 q[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) q[m] = qfrag(0, 0, m);
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), w0 = __builtin_amdgcn_s_memrealtime();
    for (int t = 0; t < tiles; ++t) {
        blk_cur = blk_next;
        blk_next = blk_cur + 13 >= nb ? blk_cur + 13 - nb : blk_cur + 13;
#pragma unroll
        for (int s8 = 0; s8 < 8; ++s8) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
#pragma unroll
                for (int mt = 0; mt < 8; ++mt) {
#pragma unroll
                    for (int n = 0; n < 2; ++n)
                        acc[mt][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, q[mt & 3]),
                                                                             __builtin_bit_cast(f16x8, pf[n][s8 * 2 + c]), acc[mt][n], 0, 0, 0);
                    if (!(ABL & 2)) {
                        if (mt < 4) q[mt & 3] = qfrag(s8 % RING, c, mt + 4);
                        else if (c == 0) q[mt & 3] = qfrag(s8 % RING, 1, mt - 4);
                        else q[mt & 3] = qfrag((s8 + 1) % RING, 0, mt - 4);       // published by the barrier of the stage before
                    }
                    if (mt == 1) piece((s8 + DEPTH) % RING, s8 + DEPTH >= 8, (s8 + DEPTH) & 7, c);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            wait_vm<PIECES>();
            if (!(ABL & 4)) __builtin_amdgcn_s_barrier();
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), w1 = __builtin_amdgcn_s_memrealtime();
    if (tid == 0) {
        clk[blockIdx.x * 2] = t1 - t0;
        clk[blockIdx.x * 2 + 1] = w1 - w0;
    }
    float sink = 0.f;
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) sink += acc[a][b][1];
    sink += q[0].x;
    if (sink == 12345.678f) out[0] = sink;
}

static int cmp_double(const void* a, const void* b) {
    const double x = *(const double*)a, y = *(const double*)b;
    return x < y ? -1 : x > y ? 1 : 0;
}

// One arm of the shape A/B: LAUNCHES back-to-back launches timed as one (the clock settles over milliseconds), stamps of the last.
template <class K>
static double run_shape(K k, const char* name, int abl, int rep, const float* src, int64_t rows, float* out, unsigned long long* clk) {
    const int tiles = 1024, launches = 64;
    const size_t lds_bytes = 4 * STAGE_WORDS * 4;
    hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL(k, dim3(256), dim3(512), lds_bytes, 0, src, rows, 256, 16, out, clk);
    hipEventRecord(e0);
    for (int i = 0; i < launches; ++i) hipLaunchKernelGGL(k, dim3(256), dim3(512), lds_bytes, 0, src, rows, 256, tiles, out, clk);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms = 0; hipEventElapsedTime(&ms, e0, e1);
    static unsigned long long h[512];
    static double ghz[256], cyc[256];
    (void)hipMemcpy(h, clk, sizeof h, hipMemcpyDeviceToHost);
    for (int b = 0; b < 256; ++b) {
        ghz[b] = (double)h[2 * b] / ((double)h[2 * b + 1] * 10.0);               // s_memrealtime ticks at 100 MHz
        cyc[b] = (double)h[2 * b] / (tiles * 4);
    }
    qsort(ghz, 256, sizeof(double), cmp_double);
    qsort(cyc, 256, sizeof(double), cmp_double);
    const double us = ms * 1e3 / ((double)launches * tiles * 4);
    printf("rep %d  shape %-8s abl %d: %.3f us per 8.4 MFLOP/CU -> %.0f TFLOP/s | %.0f cycles per 8.4 MFLOP, %.3f GHz in-kernel (medians of 256 workgroups)   [%s]\n",
           rep, name, abl, us, 2.0 * 256 * 256 * 64 * 256 / us * 1e-6, cyc[128], ghz[128], hipGetErrorString(hipGetLastError()));
    fflush(stdout);
    hipEventDestroy(e0); hipEventDestroy(e1);
    return us;
}

static void summary(const char* what, double* a32, double* a16, int reps) {
    qsort(a32, reps, sizeof(double), cmp_double);
    qsort(a16, reps, sizeof(double), cmp_double);
    const double m32 = a32[reps / 2], m16 = a16[reps / 2], s32 = a32[reps - 1] - a32[0], s16 = a16[reps - 1] - a16[0];
    const double spread = s32 > s16 ? s32 : s16;
    printf("%-12s 32x32x16 median %.3f us (max - min %.3f) | 16x16x32 median %.3f us (max - min %.3f) | 32/16 = %.3f | difference of medians %.3f us = %.1f x the larger spread\n",
           what, m32, s32, m16, s16, m32 / m16, m32 - m16, spread > 0 ? (m32 - m16) / spread : 0.0);
}

// `pstat shape [reps]`: both shapes alternately, full stage and MFMAs alone (ablation 1|2|4), 200 MB source.
static int shape_ab(int reps) {
    const int src_mb = 200;
    const int64_t rows = (int64_t)src_mb * 1024;
    float *src, *out;
    unsigned long long* clk;
    (void)hipMalloc(&src, rows * 1024);
    (void)hipMalloc(&out, 4);
    (void)hipMalloc(&clk, sizeof(unsigned long long) * 512);
    uint16_t* hsrc = (uint16_t*)malloc(rows * 1024);
    uint32_t x = 12345u;
    for (int64_t i = 0; i < rows * 512; ++i) {
        x = x * 1664525u + 1013904223u;
        hsrc[i] = (uint16_t)(((x >> 16) & 0x83ffu) | 0x3400u | ((x >> 8) & 0x0400u));
    }
    (void)hipMemcpy(src, hsrc, rows * 1024, hipMemcpyHostToDevice);
    free(hsrc);
    if (reps > 32) reps = 32;
    double full32[32], full16[32], bare32[32], bare16[32];
    for (int rep = 0; rep < reps; ++rep) {
        full32[rep] = run_shape(pstat<8, 2, 1, 0>, "32x32x16", 0, rep, src, rows, out, clk);
        full16[rep] = run_shape(pstat16<0>, "16x16x32", 0, rep, src, rows, out, clk);
        bare32[rep] = run_shape(pstat<8, 2, 1, 7>, "32x32x16", 7, rep, src, rows, out, clk);
        bare16[rep] = run_shape(pstat16<7>, "16x16x32", 7, rep, src, rows, out, clk);
    }
    summary("full stage", full32, full16, reps);
    summary("MFMAs alone", bare32, bare16, reps);
    (void)hipFree(src); (void)hipFree(out); (void)hipFree(clk);
    return 0;
}

template <int NW, int LAG, int ROT, int ABL = 0>
static void run(const float* src, int64_t rows, int ld_words, float* out, int src_mb) {
    const int tiles = 1024;                          // 8192 stages of 16 KB = 4096 units of 8.4 MFLOP per CU
    const size_t lds_bytes = 4 * STAGE_WORDS * 4;
    hipFuncSetAttribute((const void*)pstat<NW, LAG, ROT, ABL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL((pstat<NW, LAG, ROT, ABL>), dim3(256), dim3(NW * 64), lds_bytes, 0, src, rows, ld_words, 16, out);
    hipEventRecord(e0);
    hipLaunchKernelGGL((pstat<NW, LAG, ROT, ABL>), dim3(256), dim3(NW * 64), lds_bytes, 0, src, rows, ld_words, tiles, out);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms = 0; hipEventElapsedTime(&ms, e0, e1);
    const double us = ms * 1e3 / (tiles * 4);        // per 8.4 MFLOP per CU (two 16-KB stages)
    printf("src %3d MB  waves %d lag %d rot %d abl %2d: %.3f us per 8.4 MFLOP/CU -> %.0f TFLOP/s of 2500 (%.2f)   [%s]\n", src_mb, NW, LAG, ROT, ABL, us,
           2.0 * 256 * 256 * 64 * 256 / us * 1e-6, 2.0 * 256 * 256 * 64 * 256 / us * 1e-6 / 2500.0, hipGetErrorString(hipGetLastError()));
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "shape")) return shape_ab(argc > 2 ? atoi(argv[2]) : 7);
    for (int src_mb : {16, 200}) {
        const int ld_words = 256;
        const int64_t rows = (int64_t)src_mb * 1024;
        float *src, *out;
        (void)hipMalloc(&src, rows * 1024);
        (void)hipMalloc(&out, 4);
        // random f16 bit patterns in a sane exponent range (the clock follows the operand bits: never bench on constants)
        {
            uint16_t* hsrc = (uint16_t*)malloc(rows * 1024);
            uint32_t x = 12345u;
            for (int64_t i = 0; i < rows * 512; ++i) {
                x = x * 1664525u + 1013904223u;
                hsrc[i] = (uint16_t)(((x >> 16) & 0x83ffu) | 0x3400u | ((x >> 8) & 0x0400u));
            }
            (void)hipMemcpy(src, hsrc, rows * 1024, hipMemcpyHostToDevice);
            free(hsrc);
        }
        run<4, 2, 1>(src, rows, ld_words, out, src_mb);
        run<8, 1, 0>(src, rows, ld_words, out, src_mb);
        run<8, 2, 0>(src, rows, ld_words, out, src_mb);
        run<8, 2, 1>(src, rows, ld_words, out, src_mb);
        run<8, 2, 1, 1>(src, rows, ld_words, out, src_mb);
        run<8, 2, 1, 2>(src, rows, ld_words, out, src_mb);
        run<8, 2, 1, 3>(src, rows, ld_words, out, src_mb);
        run<8, 2, 1, 4>(src, rows, ld_words, out, src_mb);
        run<8, 2, 1, 7>(src, rows, ld_words, out, src_mb);
        run<8, 2, 1, 8>(src, rows, ld_words, out, src_mb);
        run<8, 2, 1, 16>(src, rows, ld_words, out, src_mb);
        run<8, 2, 1, 24>(src, rows, ld_words, out, src_mb);
        run<8, 2, 1, 32>(src, rows, ld_words, out, src_mb);
        (void)hipFree(src); (void)hipFree(out);
    }
    return 0;
}
