// Operand-stationary form of the 256-row f16 filter engine (round 5): the workgroup's P block never moves again.
//
// wide_engine.h streams BOTH operands of a 256 x 256 tile through LDS: 64 KB of LDS-DMA and 24 fragment reads per wave for
// every 8.4 MFLOP of a CU, and its stage takes 2.18 us (L2-missing operands, the real kernels' regime) for 1.0 us of MFMA
// time - the fill path, not the instruction order, bounds it (rounds 2-4).  A filter kernel's work item pairs ONE
// 256-row P block with MANY Q tiles, so here the P block is read once, straight into registers, as MFMA B fragments:
//   * 512 threads = 8 wave64; wave w owns P rows 32 w .. 32 w + 31 for the whole inner dimension: KSLABS * 4 fragments of
//     16 B per lane (128 registers at D = 512), loaded with buffer loads at the start of the work item and never re-read;
//   * a stage is a 64-element slab of 128 Q rows (half a 256-row tile) = 16 KB, eight of them make a unit (half tile x D = 512);
//     a wave multiplies its 32 P rows with all 128 Q rows: 4 x 1 MFMA tiles, 64 accumulator registers, 16 MFMAs and 16
//     fragment reads per stage (Q only);
//   * the Q slabs travel through a ring of four 16-KB LDS slots by LDS-DMA, three stages ahead, two pieces per wave and
//     stage, with COUNTED vmcnt and raw s_barrier: the barrier at the end of stage g publishes stage g + 2, so the first
//     fragments of stage g + 1 are read under the last MFMAs of stage g and no DMA is ever drained inside a unit;
//   * one set of four Q fragments per wave: fragment m of the next k-step is read right behind the MFMA that used fragment m.
// Per 8.4 MFLOP the load path moves 32 KB instead of 64 KB, and the L2 of an XCD only has to hold the Q window its 32
// workgroups walk in lockstep - the 32 P blocks (8 MB against 4 MB of L2) that thrashed it are gone.
// tools/ubench/pstat.hip (random f16 operands, same unit): 1.55-1.60 us per 8.4 MFLOP against 1.73 (L2-resident source) /
// 2.19 (200 MB source) for wide_engine.h's adopted schedule on the same box (profiles/r5/ubench_pstat.txt).
//
// That is the first of three shapes (Pstat32Body, Pstat16Body, Pstat64Body below).  All three run through pstat_pipeline at the
// end of this file: the ring, the unit loop and everything the hazards below depend on exist once; a shape supplies its
// Lane, its geometry and the MFMA loop of one stage.
//
// LDS image of a slot: rows of 128 B, 16-B chunks XOR-swizzled by (row >> 1) & 7 (wide_engine.h).  MFMA roles, k order and
// therefore every accumulator value are those of wide_engine.h: P rows lane-local (MFMA column = lane & 31), Q rows in the
// registers, logical chunk 2c + h of slab kt in k-step 4 kt + c.  (Pstat16Body, the 16x16x32 body, accumulates in
// another order: its accumulator values differ in the last bits, the results behind the exact re-evaluation do not.)
//
// Hazards (MI355X_MICROARCH.md, "LDS-DMA requests stay in flight across s_barrier"):
//   RAW  stage g + 2 is read (first: the pre-read at the end of stage g + 1) only after the barrier that ends stage g, before
//        which every wave has waited for its own pieces of that stage (vmcnt(PIECES): only the pieces of stage g + 3, issued
//        during stage g, may still be in flight);
//   WAR  the pieces of stage g + 3 are issued during stage g into the slot stage g - 1 was read from; every wave's reads of
//        stage g - 1 had returned (they fed its MFMAs) before it arrived at the barrier that ends stage g - 1.
#pragma once
#include "wide_engine.h"

namespace am {

constexpr int PQ_ROWS = 128;                          // Q rows of a stage: half a 256-row tile
constexpr int PRING = 4;
constexpr int PTHREADS = 512;
// Of a P row's KSLABS 64-element slabs the first PREG_SLABS live in registers (16 per slab); slabs 7 and 8 would leave
// the epilogues 48 registers beside 64 accumulators and the compiler spills P fragments into the main loop - they stay in LDS
// instead (32 KB per slab, each wave reading only its own 32 rows: no barrier involved), one extra ds_read_b128 per k-step.
constexpr int PREG_SLABS = 6;
constexpr int pstat_lds_slabs(int kslabs) { return kslabs > PREG_SLABS ? kslabs - PREG_SLABS : 0; }
constexpr int pstat_lds_words(int kslabs) { return PRING * PQ_ROWS * WROW + pstat_lds_slabs(kslabs) * WTB * WROW; }   // 64 KB + 32 KB per LDS slab

template <int N>
__device__ __forceinline__ void pstat_wait() {        // vmcnt(N) and lgkmcnt(0): the stage's own LDS writes (side data) are out too
    static_assert(N >= 0 && N < 64, "vmcnt");
    __builtin_amdgcn_s_waitcnt(0x0070 | (N & 15) | ((N >> 4) << 14));
}

// Lane geometry the epilogues see.  `wm` = which unit of the Q tile the accumulators of the CURRENT finish() call belong
// to (the engine sets it; in wide_engine.h it is a property of the wave), NT = 32-row P tiles per wave.
struct PLane {
    static constexpr int NT = 1;
    static constexpr int MT = 4;                      // 32-row Q tiles of a unit (accumulator tiles per P tile)
    static constexpr int WAVES = 8;
    static constexpr int LISTS = 2;                   // partial per-row lists after the sweep: the two lane halves
    // The accumulators of a unit do not start at zero but at a per-COLUMN value the epilogue supplies (acc_init): the k-NN
    // sweep and the membership filter start them at -|y_j|^2 / 2 in the units of the scaled dot product, so that what comes out
    // is <x, y_j> - |y_j|^2 / 2 and the epilogue's fast path needs no fma per element to add the column norm.  The vector ALU
    // and the matrix pipe of a SIMD do not overlap here (profiles/r5/wide_bench_nomargin.txt: one vector pass per accumulator
    // element = 0.15 ms per sweep at 100 000 rows, at D = 128 and at D = 512 alike), and the start values are the same LDS
    // reads the epilogue did anyway.
    static constexpr bool ACC_INIT = true;
    // accumulator geometry (32x32x16 MFMA): register 4 g4 + e of a tile <-> Q row g4 * GSTRIDE + 4 * (lane group) + e of its QT rows
    static constexpr int GSTRIDE = 8, GROUPS = 2, QT = 32;
    int tid, lane, wave, wm, r, h;
    __device__ __forceinline__ PLane() {
        tid = threadIdx.x;
        lane = tid & 63;
        wave = tid >> 6;
        wm = 0;
        r = lane & 31;
        h = lane >> 5;
    }
    __device__ __forceinline__ int prow(int) const { return wave * 32 + r; }          // row of the P block this lane owns
    __device__ __forceinline__ int list_slot() const { return h; }
};

// ---- the same engine on the 16x16x32 MFMA -------------------------------------------------------------------------------------
//
// The f16 matrix pipe is power-limited here, and the clock the chip holds depends on the MFMA shape: the same stage on
// v_mfma_f32_16x16x32_f16 takes the same cycles at a 1.11 x higher clock (tools/ubench/pstat.hip shape,
// profiles/mfma_shape/ubench_pstat_shape.txt: 1.50 -> 1.35 us per 8.4 MFLOP of a CU).  Same 512 threads, same LDS
// image of the Q slots and the P slabs, but another accumulation order inside the matrix core: the accumulator VALUES differ
// from Pstat32Body's in the last bits (fast_c(D) prices D + 1 terms in any order), the RESULTS behind the exact re-evaluation
// do not.
//   * P (MFMA B): wave w owns P rows 32 w .. 32 w + 31 as TWO 16-row tiles; lane = (r = lane & 15, g = lane >> 4); the fragment
//     of the k-step of 32 elements is the 16 B at element offset 8 g: 16 registers per slab and wave, as above;
//   * Q (MFMA A): eight 16-row tiles per stage, two k-steps per slab: 16 ds_read_b128 per wave and stage, as above, each feeding
//     two MFMAs; the lane reads chunk (4 c + g) ^ ((r >> 1) & 7) of row 16 mt + r.  Every lane group of a ds_read_b128 lands on
//     sixteen distinct 16-B columns (column = 8 (r & 1) + ((4 c + g) ^ s), s = (r >> 1) & 7; a group holds every s twice with
//     g = g0 for s in {0, 1, 6, 7} and g0 ^ 1 for s in {2 .. 5}, and s -> g(s) ^ s is a bijection of 0 .. 7);
//   * 32 MFMAs of 16 cycles per wave and stage; a ring of four fragment registers: the fragment of tile mt + 4 is read right
//     behind the MFMAs of tile mt (three MFMA gaps = 96 cycles ahead, as above); the two DMA pieces behind tile 1 of either k-step;
//   * 64 accumulator registers as acc[2][2] composites of four 16 x 16 outputs: register 4 t + v of acc[m][nt] holds Q row
//     64 m + 16 t + 4 g + v of the unit, P row 16 nt + r of the wave.
struct P16Lane {
    static constexpr int NT = 2;                      // 16-row P tiles per wave
    static constexpr int MT = 2;                      // 64-row accumulator tiles of a unit
    static constexpr int WAVES = 8;
    static constexpr int LISTS = 4;                   // partial per-row lists after the sweep: the four lane groups
    static constexpr bool ACC_INIT = true;
    static constexpr int GSTRIDE = 16, GROUPS = 4, QT = 64;
    int tid, lane, wave, wm, r, h;                    // h = lane group
    __device__ __forceinline__ P16Lane() {
        tid = threadIdx.x;
        lane = tid & 63;
        wave = tid >> 6;
        wm = 0;
        r = lane & 15;
        h = lane >> 4;
    }
    __device__ __forceinline__ int prow(int nt) const { return wave * 32 + nt * 16 + r; }
    __device__ __forceinline__ int list_slot() const { return h; }
};

// ---- the stationary engine for NARROW rows (round 6): KSLABS <= P64_MAX_SLABS, i.e. D <= 128 (VGGish, n_pca = 64 ...) -------------
//
// At D = 128 a unit of the engine above is two stages long and its epilogue (vector ALU, matrix pipe idle) is 55 % of the k-NN
// sweep.  VERDICT r5 asked for the epilogue of one wave to run under the MFMAs of its SIMD partner.  What the
// microbenchmark found (tools/ubench/pskew.hip, profiles/r6/ubench_pskew_v*.txt):
//   * beside an OLDER wave that issues MFMAs a wave's vector instructions get about half their issue slots (s_setprio changes
//     nothing; with the vector wave the older one both run at their own pace), and the chip sits at its power limit while the
//     matrix pipe runs (1.5-1.65 GHz against 2.3 GHz in a vector-only phase): overlap buys cycles, the clock gives part back;
//   * skewing waves 0-3 against 4-7 on ONE Q stream with ONE barrier per stage is slower than lockstep (the wave in its
//     epilogue is alone on the vector ALU at ~5 cycles per instruction and every other wave waits for it at the barrier);
//     LDS-flag synchronisation instead of s_barrier costs more than it frees;
//   * what does pay where the registers allow it: TWO INDEPENDENT 256-thread workgroups per CU (own ring, own barriers - the two
//     waves of a SIMD drift apart by themselves) whose waves own 64 P rows = TWO row tiles each, against 64-row Q units:
//     every Q fragment read from LDS feeds two MFMAs (half the LDS reads per flop), the LDS-DMA bytes per flop stay those of
//     the 512-thread form, 64 accumulator registers, and the P fragments of two row tiles (32 registers per slab) fit beside
//     them up to two slabs.  Synthetic epilogue, us per 256 MFMAs of a CU: D = 128 3.17 -> 2.43 (epilogue of 4 passes), 3.75 ->
//     2.98 (6 passes); D = 64 5.15 -> 4.49.
// Same pipeline, same LDS image and swizzle, same k order: the accumulator values are those of Pstat32Body, bit for bit.  A
// stage is 64 Q rows x 64 elements = 8 KB (two pieces per wave, as above); a 256-row Q tile is four units (L.wm = 0 .. 3).
constexpr int P64_THREADS = 256;
constexpr int P64_QROWS = 64;
constexpr int P64_MAX_SLABS = 2;
constexpr int pstat64_lds_words() { return PRING * P64_QROWS * WROW; }    // four slots of 8 KB

struct P64Lane {
    static constexpr int NT = 2;                      // 32-row P tiles per wave
    static constexpr int MT = 2;                      // 32-row Q tiles of a unit
    static constexpr int WAVES = 4;
    static constexpr int LISTS = 2;
    static constexpr bool ACC_INIT = true;
    // accumulator geometry (32x32x16 MFMA): register 4 g4 + e of a tile <-> Q row g4 * GSTRIDE + 4 * (lane group) + e of its QT rows
    static constexpr int GSTRIDE = 8, GROUPS = 2, QT = 32;
    int tid, lane, wave, wm, r, h;
    __device__ __forceinline__ P64Lane() {
        tid = threadIdx.x;
        lane = tid & 63;
        wave = tid >> 6;
        wm = 0;
        r = lane & 31;
        h = lane >> 5;
    }
    __device__ __forceinline__ int prow(int nt) const { return wave * 64 + nt * 32 + r; }
    __device__ __forceinline__ int list_slot() const { return h; }
};

// ---- the three shapes ------------------------------------------------------------------------------------------------------------
//
// What pstat_pipeline needs to know of a shape: its Lane (threads, P tiles per wave, accumulator tiles), the Q rows of a stage
// (= of a unit: 256 / QROWS units make a Q tile), the elements of a k-step (16: v_mfma_f32_32x32x16_f16, 32: 16x16x32) and how
// many slabs a P row may have.  The MFMA loop of a stage is chosen by (KELEMS, Lane::NT) inside the pipeline.
template <class Lane_, int KSLABS_, int QROWS_, int KELEMS_, int MAX_SLABS, int REG_SLABS>
struct PstatShape {
    static_assert(KSLABS_ >= 1 && KSLABS_ <= MAX_SLABS, "the P fragments of a row (two row tiles: of at most 128 f16) fit the register file");
    using Lane = Lane_;
    static constexpr int KSLABS = KSLABS_, QROWS = QROWS_, KELEMS = KELEMS_;
    static constexpr int UNITS = WTB / QROWS;                           // units of a 256-row Q tile
    static constexpr int KREG = KSLABS < REG_SLABS ? KSLABS : REG_SLABS;  // slabs of the P rows held in registers, the others in LDS
    static constexpr bool LDS_SLABS = REG_SLABS < MAX_SLABS;            // does the shape have widths with slabs in LDS at all
    static constexpr int CSTEPS = 64 / KELEMS;                          // k-steps of a slab
    static constexpr int QTILE = KELEMS == 16 ? 32 : 16;                // Q rows of an MFMA
    static constexpr int NQ = KELEMS == 16 ? QROWS / QTILE : 4;         // Q fragment registers (16x16x32: a ring of four for eight tiles)
    static constexpr int PROWS = WTB / Lane::WAVES, PTILE = PROWS / Lane::NT;   // P rows of a wave, of one of its tiles
};
template <int KSLABS> using Pstat32Body = PstatShape<PLane, KSLABS, PQ_ROWS, 16, 8, PREG_SLABS>;
template <int KSLABS> using Pstat16Body = PstatShape<P16Lane, KSLABS, PQ_ROWS, 32, 8, PREG_SLABS>;
template <int KSLABS> using Pstat64Body = PstatShape<P64Lane, KSLABS, P64_QROWS, 16, P64_MAX_SLABS, P64_MAX_SLABS>;

// Q, P: f16 matrices viewed as f32 words (ld in words), rows of KSLABS * 32 words.  tmap(t) = index of the 256-row Q tile that
// local tile t multiplies; P block = rows prow0 .. prow0 + 255.  Epi:
//   aux_issue(t, qtile) / aux_commit(t)   per-TILE side data through LDS (as in wide_engine.h)
//   finish(t, qtile, acc[MT][NT])         once per UNIT, L.wm telling which of the tile's
//   acc_init(t, m)                        start value of accumulator tile m (Lane::QT Q rows) of unit L.wm of local tile t
// The MFMA loops of the shapes stand in this one function, under `if constexpr`, and not behind functions of the shape: the
// compiler simplifies a function before it inlines it, and with the stage (or only the P load, or the fragment addresses) in a
// function of its own every kernel came out with other address arithmetic and hundreds of reordered lines.  For the same
// reason the unit index keeps the arithmetic of a two-unit and of a four-unit tile apart, and the LDS fill of the P slabs is
// absent - not merely empty - in a shape that never has one.  As it stands all 40 kernels are instruction for instruction
// those of the three separate pipelines this function replaced (profiles/pstat_refactor/isa_compare.txt, tools/isa_compare.py).
template <class Body, class TileMap, class Epi>
__device__ __forceinline__ void pstat_pipeline(const float* __restrict__ Q, int64_t nq, int64_t ldq, const TileMap& tmap,
                                               const float* __restrict__ P, int64_t np, int64_t ldp, int64_t prow0, int ntiles,
                                               float* __restrict__ lds, typename Body::Lane& L, Epi& epi) {
    using Lane = typename Body::Lane;
    static_assert(Epi::ACC_INIT, "the epilogues of this engine start their accumulators at the column norm");
    constexpr int KSLABS = Body::KSLABS, KREG = Body::KREG, KLDS = KSLABS - KREG;   // slabs of a P row: in registers, in LDS
    constexpr int CSTEPS = Body::CSTEPS, KSTEPS = KREG * CSTEPS;                    // k-steps of a slab, of the register slabs
    constexpr int UNITS = Body::UNITS, ULOG = UNITS == 2 ? 1 : 2, STAGE_WORDS = Body::QROWS * WROW, NQ = Body::NQ;
    static_assert((1 << ULOG) == UNITS && (!Body::LDS_SLABS || Body::PROWS == 32), "two or four units; LDS slabs: 32 P rows per wave");
    constexpr int PIECES = 2;                         // 1-KB LDS-DMA pieces per wave and stage
    constexpr int DEPTH = 3;                          // stages in flight ahead of the one being multiplied
    const int wave = __builtin_amdgcn_readfirstlane(L.wave);

    // ---- the stationary operand: per P tile of the wave and k-step one fragment, the 16 B at element offset 8 h of the step
    f32x4 pf[Lane::NT][KSTEPS];
    {
        const TileRsrc prs = make_wide_rsrc(P, ldp, np, prow0, 0);
#pragma unroll
        for (int nt = 0; nt < Lane::NT; ++nt) {
            const unsigned vop = (unsigned)(((int64_t)(wave * Body::PROWS + nt * Body::PTILE + L.r) * ldp + L.h * 4) * 4);
#pragma unroll
            for (int s = 0; s < KSTEPS; ++s)
                pf[nt][s] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(prs.rsrc, (int)vop, s * Body::KELEMS * 2, 0));
        }
        // the slabs kept in LDS: [slab][256 rows][128 B], swizzled like a Q slot; this wave's 32 rows = 4 pieces per slab
        if constexpr (Body::LDS_SLABS) {
            const int lr8 = L.lane >> 3, s8 = L.lane & 7;
#pragma unroll
            for (int sl = 0; sl < KLDS; ++sl)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = wave * 32 + i * 8 + lr8;
                    const unsigned vo = (unsigned)(((int64_t)row * ldp + (s8 ^ ((row >> 1) & 7)) * 4) * 4);
                    lds_direct_b128(prs, lds + PRING * STAGE_WORDS + sl * WTB * WROW + (wave * 32 + i * 8) * WROW, vo, (unsigned)((KREG + sl) * 128));
                }
        }
    }
    const float* plds = lds + PRING * STAGE_WORDS + wave * 32 * WROW;      // this wave's rows of LDS slab 0

    // ---- Q slabs: piece p = 8 rows x 128 B; wave w fetches pieces 2 w, 2 w + 1 (rows 16 w .. 16 w + 15 of the unit)
    const int lr = L.lane >> 3, slot8 = L.lane & 7;
    // even piece (rows lr of the wave's sixteen); the odd piece's rows lie 8 further down and their swizzle (row >> 1) & 7
    // differs in bit 2 of the chunk index = bit 6 of the byte offset (rows are multiples of 128 B): one register, one XOR
    const unsigned voq0 = (unsigned)(((int64_t)lr * ldq + (slot8 ^ ((lr >> 1) & 7)) * 4) * 4);
    const unsigned odd_soff = (unsigned)((int64_t)8 * ldq * 4);
    const unsigned wave_soff = (unsigned)((int64_t)wave * 16 * ldq * 4), unit_soff = (unsigned)((int64_t)Body::QROWS * ldq * 4);
    const int64_t q_tiles_total = (nq + WTB - 1) / WTB;
    auto qtile_of = [&](int t) -> int64_t { return t < ntiles ? tmap(t) : q_tiles_total; };   // past the end: empty descriptor
    int ft = 0, fu = 0, fk = 0, fslot = 0;            // (tile, unit, slab, ring slot) of the stage being fetched
    TileRsrc qrs = make_wide_rsrc(Q, ldq, nq, qtile_of(0) * WTB);
    auto fetch_stage = [&](int i) {                   // piece i of the stage under the fetch cursor
        float* dst = lds + fslot * STAGE_WORDS + (wave * 2 + i) * 8 * WROW;
        lds_direct_b128(qrs, dst, i == 0 ? voq0 : (voq0 ^ 64u),
                        (unsigned)(fk * 128) + (UNITS == 2 ? (fu ? unit_soff : 0u) : (unsigned)fu * unit_soff) + wave_soff + (i == 0 ? 0u : odd_soff));
    };
    auto next_tile = [&]() {
        ++ft;
        qrs = make_wide_rsrc(Q, ldq, nq, qtile_of(ft) * WTB);
    };
    auto advance_fetch = [&]() {
        fslot = (fslot + 1) & (PRING - 1);
        if (++fk == KSLABS) {
            fk = 0;
            if constexpr (UNITS == 2) {
                fu ^= 1;
                if (fu == 0) next_tile();
            } else if (++fu == UNITS) {
                fu = 0;
                next_tile();
            }
        }
    };

    // fragment addresses: logical 16-B chunk (KELEMS / 8) c + h of row r sits in slot (that chunk) ^ ((r >> 1) & 7); row tiles
    // lie QTILE rows apart
    const int sw = (L.r >> 1) & 7;
    int coff[CSTEPS];
#pragma unroll
    for (int c = 0; c < CSTEPS; ++c) coff[c] = L.r * WROW + ((Body::KELEMS / 8 * c + L.h) ^ sw) * 4;
    auto qfrag = [&](int ring_slot, int c, int m) -> f32x4 {
        return *reinterpret_cast<const f32x4*>(lds + ring_slot * STAGE_WORDS + m * Body::QTILE * WROW + coff[c]);
    };
    auto pfrag_lds = [&](int step, int nt) -> f32x4 {     // P tile nt in the LDS slabs (16x16x32)
        return *reinterpret_cast<const f32x4*>(plds + (step / 2 - KREG) * WTB * WROW + nt * 16 * WROW + coff[step & 1]);
    };

    f32x16 acc[Lane::MT][Lane::NT];
    // a unit's accumulators start at acc_init's per-column value (PLane), the same for every P tile of the wave
    auto start_unit = [&](int t, int wm) {
        L.wm = wm;
#pragma unroll
        for (int m = 0; m < Lane::MT; ++m) {
            const f32x16 c0 = epi.acc_init(t, m);
#pragma unroll
            for (int nt = 0; nt < Lane::NT; ++nt) acc[m][nt] = c0;
        }
    };

    // prologue: DEPTH stages in flight, the first two landed and published
#pragma unroll
    for (int g = 0; g < DEPTH; ++g) {
        fetch_stage(0);
        fetch_stage(1);
        advance_fetch();
    }
    epi.aux_issue(0, qtile_of(0));
    __builtin_amdgcn_s_waitcnt(0x0F70);               // vmcnt(0): side data (and the P fragments) are here
    epi.aux_commit(0);
    pstat_wait<0>();
    __builtin_amdgcn_s_barrier();

    f32x4 q[NQ];
    f32x4 pl[2][Lane::NT];                            // P fragments of the LDS slabs, read one k-step ahead
    int slot = 0;                                     // ring slot of the stage being multiplied
#pragma unroll
    for (int m = 0; m < NQ; ++m) q[m] = qfrag(0, 0, m);
    start_unit(0, 0);
    const int units = UNITS * ntiles;
    for (int u = 0; u < units; ++u) {
        const int t = u >> ULOG, part = u & (UNITS - 1);
        const bool last_unit = UNITS == 2 ? part != 0 : part == UNITS - 1;      // of its tile
#pragma unroll
        for (int ks = 0; ks < KSLABS; ++ks) {
            const bool last_stage = ks == KSLABS - 1;
            const int next_slot = (slot + 1) & (PRING - 1);
            if (last_stage && last_unit && t + 1 < ntiles) epi.aux_issue(t + 1, qtile_of(t + 1));
            // ---- the multiply of the stage
#pragma unroll
            for (int c = 0; c < CSTEPS; ++c) {
                const int step = ks * CSTEPS + c;     // k-step of the unit; steps >= KSTEPS take their P fragments from LDS
                if constexpr (Body::KELEMS == 32) {
                    // 16x16x32: a ring of four Q fragments, the fragment of tile mt + 4 read right behind the MFMAs of tile mt
                    if (KLDS > 0 && step + 1 >= KSTEPS && step + 1 < KSLABS * 2) {
                        pl[(step + 1) & 1][0] = pfrag_lds(step + 1, 0);
                        pl[(step + 1) & 1][1] = pfrag_lds(step + 1, 1);
                    }
                    const f32x4 pb0 = step < KSTEPS ? pf[0][step < KSTEPS ? step : 0] : pl[step & 1][0];
                    const f32x4 pb1 = step < KSTEPS ? pf[1][step < KSTEPS ? step : 0] : pl[step & 1][1];
#pragma unroll
                    for (int mt = 0; mt < 8; ++mt) {
                        const int m = mt >> 2, t4 = (mt & 3) * 4;
#pragma unroll
                        for (int nt = 0; nt < 2; ++nt) {
                            f32x4 a = {acc[m][nt][t4], acc[m][nt][t4 + 1], acc[m][nt][t4 + 2], acc[m][nt][t4 + 3]};
                            a = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, q[mt & 3]), __builtin_bit_cast(f16x8, nt == 0 ? pb0 : pb1), a, 0, 0, 0);
                            acc[m][nt][t4] = a.x; acc[m][nt][t4 + 1] = a.y; acc[m][nt][t4 + 2] = a.z; acc[m][nt][t4 + 3] = a.w;
                        }
                        if (mt < 4) q[mt & 3] = qfrag(slot, c, mt + 4);
                        else if (c == 0) q[mt & 3] = qfrag(slot, 1, mt - 4);
                        else if (!last_stage) q[mt & 3] = qfrag(next_slot, 0, mt - 4);     // published by the barrier of the stage before
                        if (mt == 1) fetch_stage(c);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                } else {
                    // 32x32x16, ONE fragment set: the fragment of row tile m for the next k-step is read right behind the MFMAs that
                    // used this one (ubench: as fast as two sets read a k-step ahead - 1.49-1.50 us per 8.4 MFLOP - and sixteen
                    // registers less)
                    static_assert(Lane::NT == 1 || KLDS == 0, "two row tiles: every slab in registers");
                    if (KLDS > 0 && step + 1 >= KSTEPS && step + 1 < KSLABS * 4)
                        pl[(step + 1) & 1][0] = *reinterpret_cast<const f32x4*>(plds + ((step + 1) / 4 - KREG) * WTB * WROW + coff[(step + 1) & 3]);
#pragma unroll
                    for (int m = 0; m < Lane::MT; ++m) {
                        if constexpr (Lane::NT == 1) {
                            const f32x4 pfrag = step < KSTEPS ? pf[0][step < KSTEPS ? step : 0] : pl[step & 1][0];
                            acc[m][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, q[m]), __builtin_bit_cast(f16x8, pfrag), acc[m][0], 0, 0, 0);
                        } else {
#pragma unroll
                            for (int nt = 0; nt < Lane::NT; ++nt)
                                acc[m][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, q[m]), __builtin_bit_cast(f16x8, pf[nt][step]), acc[m][nt], 0, 0, 0);
                        }
                        if (c < 3) q[m] = qfrag(slot, c + 1, m);
                        else if (!last_stage) q[m] = qfrag(next_slot, 0, m);     // published by the barrier of the stage before
                        if (m == 1 && (c & 1) == 0) fetch_stage(c >> 1);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            advance_fetch();
            if (last_stage) {
                L.wm = UNITS == 2 ? (last_unit ? 1 : 0) : part;
                epi.finish(t, qtile_of(t), acc);
                if (last_unit && t + 1 < ntiles) epi.aux_commit(t + 1);
            }
            // this wave's pieces of stage g + 2 have landed; the barrier publishes that stage
            pstat_wait<PIECES>();
            __builtin_amdgcn_s_barrier();
            slot = next_slot;
            if (last_stage) {                         // a unit's first fragments are read behind its predecessor's epilogue:
#pragma unroll                                        // no fragment register is live across the epilogue
                for (int m = 0; m < NQ; ++m) q[m] = qfrag(slot, 0, m);
                // ... and its accumulators' start values (side data of a new tile: committed before the barrier above).
                // Reading them a unit earlier, in front of the barrier, was measured: the same time (profiles/r5/wide_bench_accinit_ab.txt).
                if (u + 1 < units) start_unit((u + 1) >> ULOG, UNITS == 2 ? (last_unit ? 0 : 1) : (u + 1) & (UNITS - 1));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);               // the (empty) fetches past the end: nothing in flight when LDS is reused
    __syncthreads();
}

}  // namespace am
