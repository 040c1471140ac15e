// The group-list protocol of am_stats_gather_*, am_frechet_groups_* and am_mmd_rbf_groups_f32 (host side only): group b is
// the rows X[idx[offsets[b] + j]], j < offsets[b + 1] - offsets[b] (idx == NULL where an entry point allows it: the rows in
// stored order).  The workspace of every such call opens with one head: the flag word - 1 + the list position of an index
// outside [0, N), or 0; the kernels never dereference such an index, and the caller reads the word back from the first 8
// bytes of the workspace - then the device copy of the B + 1 offsets, then whatever small per-group data the call asks for.
#pragma once
#include "am_common.h"

namespace am {

struct GroupHead {
    unsigned long long* flag;
    int64_t* offs;
    char* tail;                    // tail_bytes behind the offsets (8-byte aligned)
};

static inline GroupHead carve_group_head(Carver& c, int B, size_t tail_bytes = 0) {
    const size_t offs_bytes = ((size_t)B + 1) * 8;
    char* head = c.take<char>(8 + offs_bytes + tail_bytes);
    return {reinterpret_cast<unsigned long long*>(head), reinterpret_cast<int64_t*>(head ? head + 8 : nullptr),
            head ? head + 8 + offs_bytes : nullptr};
}

// the stored matrix the groups name rows of.  float32: 16-byte loads through 32-bit element offsets; float64: no alignment rule
template <class T>
static inline int check_group_rows(const T* X, int64_t N, int64_t ld, int D) {
    if (sizeof(T) == 8) {
        AM_REQUIRE(D <= 8192 && ld >= D, AM_ERR_BAD_ARG, "float64 rows: D=%d (<= 8192), ld=%lld (>= D)", D, (long long)ld);
    } else {
        AM_REQUIRE(aligned16(X) && ld % 4 == 0 && ld >= D, AM_ERR_BAD_ARG,
                   "X must be 16-byte aligned with ld %% 4 == 0 and ld >= D (ld=%lld, D=%d)", (long long)ld, D);
        AM_REQUIRE(N * ld < ((int64_t)1 << 30), AM_ERR_BAD_SHAPE,
                   "float32 rows are addressed with 32-bit offsets: %lld x %lld floats is 4 GiB or more", (long long)N, (long long)ld);
    }
    return AM_OK;
}

// offsets[0] == 0 and every group holds 1 .. max_rows rows (max_rows == 0: any number); *n_total = offsets[B]
static inline int check_group_offsets(const int64_t* offsets, int B, int64_t max_rows, int64_t* n_total) {
    AM_REQUIRE(offsets[0] == 0, AM_ERR_BAD_ARG, "offsets[0]=%lld, must be 0", (long long)offsets[0]);
    for (int b = 0; b < B; ++b) {
        const int64_t n = offsets[b + 1] - offsets[b];
        if (max_rows > 0)
            AM_REQUIRE(n >= 1 && n <= max_rows, AM_ERR_BAD_SHAPE, "group %d has %lld rows (1 <= rows <= %lld)", b, (long long)n,
                       (long long)max_rows);
        else
            AM_REQUIRE(n >= 1, AM_ERR_BAD_SHAPE, "group %d has %lld rows (offsets must increase strictly)", b, (long long)n);
    }
    *n_total = offsets[B];
    return AM_OK;
}

static inline int check_stored_rows(const int64_t* idx, int64_t n_total, int64_t N) {
    AM_REQUIRE(idx || n_total <= N, AM_ERR_BAD_SHAPE, "no index list: the groups name %lld stored rows, X holds %lld", (long long)n_total,
               (long long)N);
    return AM_OK;
}

static inline int upload_group_head(const GroupHead& h, const int64_t* offsets, int B, hipStream_t st) {
    AM_HIP_TRY(hipMemsetAsync(h.flag, 0, sizeof(unsigned long long), st));
    AM_HIP_TRY(hipMemcpyAsync(h.offs, offsets, ((size_t)B + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    return AM_OK;
}

#define AM_TRY(expr)                                                                 \
    do {                                                                             \
        int _rc = (expr);                                                            \
        if (_rc != AM_OK) return _rc;                                                \
    } while (0)

}  // namespace am
