// What the Kernel Audio Distance family (kad.hip, kad_f64.hip, kad_groups.hip, mmd_multi.hip, mmd_rows.hip) shares whatever
// the element type: the constants and state of the radix select, the inline device helpers of the tile kernels, and the host
// launchers of the small kernels that exist once (each names the file that defines its kernel), the chunk rules, the grid
// plan and the workspace carves.  `tile_rows` is 128 on the f32 tile engine and 64 on the f64 one.
#pragma once
#include "am_common.h"

namespace am {

constexpr int KAD_MAX_CHUNK = 16;                    // Q tiles per workgroup
constexpr int KAD_BINS = 2048;                       // 11-bit first digit; the 10-bit digits use the lower half
constexpr int KAD_PASSES = 3;
constexpr int KAD_AGG_ROUNDS = 3;
constexpr int KADG_WITHIN_CHUNKS = 4;                // most Q chunks of a P tile in the within pass of the group sums
constexpr int64_t KADG_CROSS_CHUNKS = 64;            // most Q chunks of their cross pass once there are many P tiles ...
constexpr int64_t KADG_CROSS_SLOTS = 4096;           // ... (P tiles) x (chunks) may reach this with few P tiles

struct SelectState {                                 // written by the scan kernel of pass p, read by pass p + 1
    unsigned long long rank;                         // rank inside the keys that share `prefix`
    unsigned prefix;                                 // the digits fixed so far (11, 21, 31 bits)
    unsigned pad;
};

// ---------------------------------------------------------------------------------------------- device helpers
// hist[digit] += 1 for every lane with `live` set, equal digits of a wave combined first
__device__ __forceinline__ void hist_add(unsigned* __restrict__ hist, unsigned digit, bool live, int lane) {
    unsigned long long todo = __ballot(live);
#pragma unroll
    for (int round = 0; round < KAD_AGG_ROUNDS; ++round) {
        if (todo == 0ull) return;                                        // wave-uniform
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned d = (unsigned)__builtin_amdgcn_readlane((int)digit, leader);
        const bool same = live && digit == d;
        const unsigned long long mask = __ballot(same);
        if (lane == leader) atomicAdd(hist + d, (unsigned)__popcll(mask));
        live = live && !same;
        todo &= ~mask;
    }
    if (live) atomicAdd(hist + digit, 1u);
}

// first group whose end lies past position p (offs: B + 1 entries, offs[0] = 0 <= p < offs[B])
__device__ __forceinline__ int group_of(const int64_t* __restrict__ offs, int B, int64_t p) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (offs[mid + 1] > p) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// The end of a row-sum workgroup on the f32 tile engine (Lane = LaneInfo): out[row] = the sum over the workgroup's Q rows for
// each of the P tile's 128 rows, in a fixed order.  The two halves of a wave hold the same P rows against different Q rows
// (lane ^ 32); then the two wm waves, through `red` (LDS, 256 doubles, idle after the pipeline's last barrier).
template <class Lane>
__device__ __forceinline__ void fold_p_rows(const double (&sum)[Lane::NT], double* red, const Lane& L, double* __restrict__ out) {
    constexpr int ROWS = 2 * Lane::NT * 32;
    double v[Lane::NT];
#pragma unroll
    for (int nt = 0; nt < Lane::NT; ++nt) v[nt] = sum[nt] + __shfl_xor(sum[nt], 32);
    if (L.h == 0) {
#pragma unroll
        for (int nt = 0; nt < Lane::NT; ++nt) red[L.wm * ROWS + L.wn * 64 + nt * 32 + L.r] = v[nt];
    }
    __syncthreads();
    if (L.tid < ROWS) out[L.tid] = red[L.tid] + red[ROWS + L.tid];
}

// ---------------------------------------------------------------------------------------------- small kernels, by launcher
// out[i] = |X[i]|^2 in f64 for the N dense f32 rows of X (kad.hip: kad_norms_kernel)
int launch_kad_norms(const float* X, int64_t ld, int D, int64_t N, double* out, hipStream_t st);

// between two select passes (kad.hip: kad_scan_kernel<pass>): the bin that holds the wanted rank -> next prefix and the rank
// inside that bin; the last pass writes the value.  `bins` are those of the pass; rank0 is read by pass 0 only.
int launch_kad_scan(int pass, const unsigned long long* bins, SelectState* state, unsigned long long rank0, float* out, hipStream_t st);

// out[j] = sum of partial[j * count .. (j + 1) * count) for j < nout, one workgroup each, in a fixed order: strided
// per-thread sums, then a tree (mmd_multi.hip: mmd_multi_reduce_kernel)
int launch_mmd_reduce(const double* partial, int64_t count, int nout, double* out, hipStream_t st);

// rows[p] = {w_p, c_p} for p < n_total: the nw / nc chunks of a position (pw / pc[j * n_pad + p]) in chunk order
// (kad_groups.hip: kadg_rowsum_kernel)
int launch_kadg_rowsum(const double* pw, int nw, const double* pc, int nc, int64_t n_pad, int64_t n_total, double* rows, hipStream_t st);

// out[b] = {Sxx_b, Sxy_b} for the B groups, one workgroup each: strided per-thread sums over the group's positions, then a tree
// (kad_groups.hip: kadg_finish_kernel; offs is the device copy of the offsets)
int launch_kadg_finish(const double* rows, const int64_t* offs, int B, double* out, hipStream_t st);

// ---------------------------------------------------------------------------------------------- plans and carves (kad.hip)
// Q tiles per workgroup: enough workgroups to fill the chip at small sizes, few global flushes / partials at large ones;
// grid.y must stay below 65536
int kad_chunk(int64_t tiles_total, int64_t q_tiles);

// one buffer descriptor spans an f32 matrix: N * ld * 4 bytes must stay below 4 GiB
bool kad_too_large(int64_t N, int64_t ld);

// the workspace of a select: the f64 norms, the 64-bit bins of the three passes, the state
struct SelectWs {
    double* norm;
    unsigned long long* bins;
    SelectState* state;
    size_t bytes;
    bool ok;
};
SelectWs select_carve(void* ws, size_t ws_bytes, int64_t N);

// The three blocks b = 0 (XX), 1 (YY), 2 (XY) of a whole-set kernel sum: grid x = P tile, y = chunk of chunk[b] Q tiles, one
// partial per workgroup and scale (slots[b] per scale).  XX and YY sweep the upper-triangular tiles, XY all of them.
struct MmdPlan {
    int chunk[3];
    dim3 grid[3];
    size_t slots[3];
};
MmdPlan mmd_plan(int64_t N1, int64_t N2, int tile_rows);

// the f64 squared norms of the sets a block mask needs (null for a set it does not: XX and XY read X, YY and XY read Y)
struct SetNorms {
    double *n1, *n2;
};
SetNorms carve_set_norms(Carver& c, int64_t N1, int64_t N2, unsigned blocks);
int launch_set_norms(const float* X, int64_t N1, int64_t ldx, const float* Y, int64_t N2, int64_t ldy, int D, const SetNorms& n,
                     hipStream_t st);

// those norms, then nscales * slots[b] partials for each block of the mask
struct MmdWs {
    SetNorms n;
    double* partial[3];
    size_t bytes;
    bool ok;
};
MmdWs mmd_carve(void* ws, size_t ws_bytes, int64_t N1, int64_t N2, int nscales, unsigned blocks, const MmdPlan& plan);

// Q tiles per workgroup of the cross pass of the group sums: per-ROW partials, so the number of chunks is capped where the
// whole-set sums' is not
int kadg_cross_chunk(int64_t TP, int64_t TQ);

// the longest Q range (in tiles) of a P tile in the within pass of the group sums: first tile of its first group .. last tile
// of its last group.  offsets: the B + 1 host offsets; TP = P tiles of tile_rows list positions
int64_t kadg_within_span(const int64_t* offsets, int64_t TP, int64_t n_total, int tile_rows);

// Q tiles per workgroup of the within pass for that span: at most KADG_WITHIN_CHUNKS chunks
int kadg_within_chunk(int64_t span);

// what am_mmd_rbf_f32, am_mmd_multi_f32 and am_mmd_rbf_rows_f32 ask of their two f32 sets and their block mask
int check_two_sets_f32(const float* X, int64_t N1, int64_t ldx, const float* Y, int64_t N2, int64_t ldy, int D, unsigned blocks);

}  // namespace am
