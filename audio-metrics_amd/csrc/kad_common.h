// What kad.hip shares with kad_groups.hip and mmd_multi.hip (host side only): the f64 norms launch, the Q-chunk rule, the size
// rule and the grid plan of the three whole-set blocks.
#pragma once
#include "am_common.h"

namespace am {

constexpr int KAD_MAX_CHUNK = 16;                    // Q tiles per workgroup

// out[i] = |X[i]|^2 in f64 for the N dense rows of X (kad_norms_kernel)
int launch_kad_norms(const float* X, int64_t ld, int D, int64_t N, double* out, hipStream_t st);

// Q tiles per workgroup: enough workgroups to fill the chip at small sizes, few global flushes / partials at large ones;
// grid.y must stay below 65536
int kad_chunk(int64_t tiles_total, int64_t q_tiles);

// one buffer descriptor spans a matrix: N * ld * 4 bytes must stay below 4 GiB
bool kad_too_large(int64_t N, int64_t ld);

// The three blocks b = 0 (XX), 1 (YY), 2 (XY) of a whole-set kernel sum: grid x = P tile, y = chunk of chunk[b] Q tiles, one
// partial per workgroup (slots[b] of them).  XX and YY sweep the upper-triangular tiles, XY all of them.
struct MmdPlan {
    int chunk[3];
    dim3 grid[3];
    size_t slots[3];
};
MmdPlan mmd_plan(int64_t N1, int64_t N2);

}  // namespace am
