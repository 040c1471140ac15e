// The LDS-resident cyclic Jacobi of the per-group kernels (frechet_groups.hip: fg_solve_kernel, vendi.hip: vg_group_kernel):
// eigenvalues only of a symmetric m x m matrix (m even, m <= MCAP) that one 256-thread workgroup holds in LDS at the odd row
// stride MCAP + 1.  Round-robin ordering: a round holds m / 2 disjoint rotations, and A <- J^T A J is applied as (m / 2)^2
// independent 2 x 2 blocks R_a^T B R_b, of which the a <= b half is computed and mirrored, so the matrix stays exactly
// symmetric.  The sweeps stop at off-norm <= 2^-52 |A|_F or after FG_MAX_SWEEPS.  Every reduction runs in a fixed order.
#pragma once
#include "am_common.h"

namespace am {

constexpr int FG_MAX_SWEEPS = 30;
constexpr double FG_EPS = 2.220446049250313e-16;     // 2^-52

// sum of one value per thread of a 256-thread workgroup, as a fixed tree; every thread receives it
__device__ __forceinline__ double fg_block_sum(double v, double* red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}

// t-th pair (a <= b) of the h x h triangle, t < ceil(h / 2) * (h + 1): row a' of an (h + 1)-wide rectangle holds row a' of the
// triangle followed by row h - 1 - a'.  Returns false for the second half of the middle row of an odd h (a duplicate).
__device__ __forceinline__ bool fg_fold_decode(int t, int h, int& a, int& b) {
    const int ap = t / (h + 1), bp = t - ap * (h + 1);
    if (bp < h - ap) {
        a = ap;
        b = ap + bp;
        return true;
    }
    a = h - 1 - ap;
    b = a + (bp - (h - ap));
    return a != ap;
}

// the LDS a workgroup hands to fg_jacobi_lds besides the matrix: the reduction tree and one round's rotations
template <int MCAP>
struct JacobiLds {
    static constexpr int LDM = MCAP + 1;                               // odd stride: a column walk touches every bank
    static constexpr int HCAP = MCAP / 2;
    static constexpr int NBLK = (HCAP * (HCAP + 1) / 2 + 255) / 256;   // 2 x 2 blocks of the a <= b half per thread
    double* red;                                                       // [256]
    double *rc, *rs, *rt;                                              // [HCAP] the round's rotations: cos, sin, tan
    int *rp, *rq;                                                      // [HCAP] ... and their index pairs
};

// Diagonalises M (m x m, m even, stride MCAP + 1) in place; all 256 threads take part, M is complete and visible (a barrier
// lies behind its last write).  other_nonfinite: a non-finite value among the caller's own scalars, which stops the call as a
// non-finite matrix does.  Returns the stop code - 1 = converged, 2 = sweep cap reached, 4 = non-finite input - and leaves the
// eigenvalues on the diagonal; fro = |M|_F at the start, off = the off-diagonal norm at the end.
template <int MCAP>
__device__ __forceinline__ int fg_jacobi_lds(double* M, const JacobiLds<MCAP>& L, int m, bool other_nonfinite, double& fro, double& off,
                                             int& sweeps) {
    constexpr int LDM = JacobiLds<MCAP>::LDM;
    constexpr int NBLK = JacobiLds<MCAP>::NBLK;
    double* red = L.red;
    double *rc = L.rc, *rs = L.rs, *rt = L.rt;
    int *rp = L.rp, *rq = L.rq;
    const int tid = threadIdx.x;
    const int h = m / 2;

    // ---- this thread's 2 x 2 blocks (pairs of rotation slots a <= b); the same in every round
    int blk_a[NBLK], blk_b[NBLK];
    const int nfold = ((h + 1) / 2) * (h + 1);
#pragma unroll
    for (int u = 0; u < NBLK; ++u) {
        const int t = tid + u * 256;
        int a = 0, bb = 0;
        const bool ok = t < nfold && fg_fold_decode(t, h, a, bb);
        blk_a[u] = ok ? a : -1;
        blk_b[u] = bb;
    }

    double fro2 = 0.0;
    for (int e = tid; e < m * m; e += 256) {
        const double v = M[(e / m) * LDM + e % m];
        fro2 += v * v;
    }
    fro2 = fg_block_sum(fro2, red);
    fro = sqrt(fro2);
    int stop = 0;
    sweeps = 0;
    off = 0.0;
    if (!(fro2 - fro2 == 0.0) || other_nonfinite) stop = 4;            // a non-finite input reached M or the scalar terms
    while (stop == 0) {
        double off2 = 0.0;
        for (int e = tid; e < m * m; e += 256) {
            const int i = e / m, j = e - i * m;
            const double v = M[i * LDM + j];
            off2 += i != j ? v * v : 0.0;
        }
        off2 = fg_block_sum(off2, red);
        off = sqrt(off2);
        if (!(off2 - off2 == 0.0)) { stop = 4; break; }
        if (off <= FG_EPS * fro) { stop = 1; break; }
        if (sweeps == FG_MAX_SWEEPS) { stop = 2; break; }
        for (int r = 0; r < m - 1; ++r) {
            if (tid < h) {                                               // round-robin pairing: index m - 1 stays, the rest turn
                int p, q;
                if (tid == 0) {
                    p = r;
                    q = m - 1;
                } else {
                    p = r + tid;
                    if (p >= m - 1) p -= m - 1;
                    q = r - tid;
                    if (q < 0) q += m - 1;
                }
                const double app = M[p * LDM + p], aqq = M[q * LDM + q], apq = M[p * LDM + q];
                double c = 1.0, s = 0.0, tn = 0.0;
                if (apq != 0.0) {
                    const double theta = (aqq - app) / (2.0 * apq);
                    tn = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    c = 1.0 / sqrt(tn * tn + 1.0);
                    s = tn * c;
                }
                rp[tid] = p; rq[tid] = q; rc[tid] = c; rs[tid] = s; rt[tid] = tn;
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < NBLK; ++u) {
                const int a = blk_a[u], bb = blk_b[u];
                if (a < 0) continue;
                const int pa = rp[a], qa = rq[a], pb = rp[bb], qb = rq[bb];
                if (a == bb) {                                           // the pivot block: the off-diagonal element becomes 0
                    const double apq = M[pa * LDM + qa], tn = rt[a];
                    M[pa * LDM + pa] -= tn * apq;
                    M[qa * LDM + qa] += tn * apq;
                    M[pa * LDM + qa] = 0.0;
                    M[qa * LDM + pa] = 0.0;
                } else {
                    const double ca = rc[a], sa = rs[a], cb = rc[bb], sb = rs[bb];
                    const double x00 = M[pa * LDM + pb], x01 = M[pa * LDM + qb], x10 = M[qa * LDM + pb], x11 = M[qa * LDM + qb];
                    const double y00 = ca * x00 - sa * x10, y01 = ca * x01 - sa * x11;
                    const double y10 = sa * x00 + ca * x10, y11 = sa * x01 + ca * x11;
                    const double z00 = cb * y00 - sb * y01, z01 = sb * y00 + cb * y01;
                    const double z10 = cb * y10 - sb * y11, z11 = sb * y10 + cb * y11;
                    M[pa * LDM + pb] = z00; M[pb * LDM + pa] = z00;
                    M[pa * LDM + qb] = z01; M[qb * LDM + pa] = z01;
                    M[qa * LDM + pb] = z10; M[pb * LDM + qa] = z10;
                    M[qa * LDM + qb] = z11; M[qb * LDM + qa] = z11;
                }
            }
            __syncthreads();
        }
        ++sweeps;
    }
    return stop;
}

}  // namespace am
