// What kad.hip shares with kad_groups.hip (host side only): the f64 norms launch, the Q-chunk rule and the size rule.
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

}  // namespace am
