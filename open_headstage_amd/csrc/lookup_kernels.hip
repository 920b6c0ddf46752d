// lookup_kernels.hip -- k_lookup: for every query the nearest table point, and with STAGE2 the chord's other end and the weight
// (include/ohs_lookup.h, THE ARITHMETIC).
//
// One query per lane.  The table is walked in ascending m, LOOKUP_TILE_POINTS points at a time through LDS: the workgroup copies a tile
// (coalesced), every lane then reads the same address per step -- a broadcast read, no bank conflict.  The running minimum under strict <
// keeps the first of equally near points, and since no lane shares its query with another there is no merge across lanes or waves to get
// that rule wrong.  Stage 2 is a second walk with the lane's own P[idx0].  Outputs are plain vector stores.
// Compiled with -ffp-contract=off: lookup_body.hpp's operations round one by one.
#include "lookup_internal.h"
#include "lookup_body.hpp"

namespace ohs {

template <int STAGE2>
__global__ __launch_bounds__(LOOKUP_BLOCK) void k_lookup(LookupArgs a)
{
    __shared__ double tile[LOOKUP_TILE_POINTS * 3];
    const unsigned i = blockIdx.x * LOOKUP_BLOCK + threadIdx.x;
    const bool live = i < a.n;          // (a lane beyond the chunk walks along for the barriers and stores nothing)
    double q0 = 0.0, q1 = 0.0, q2 = 0.0;
    if (live) {
        if (a.q) {
            q0 = a.q[3 * (size_t)i], q1 = a.q[3 * (size_t)i + 1], q2 = a.q[3 * (size_t)i + 2];
        } else {
            const unsigned long long g = a.g0 + i, sk = g / a.K, c = g - sk * a.K;
            const unsigned long long s = sk / a.n_segs, k = sk - s * a.n_segs;
            const double *v = a.src + ((s * a.src_a + k * a.src_b - a.src_base) * a.K + c) * 3;
            q0 = v[0], q1 = v[1], q2 = v[2];
            if (a.rot) lookup_pose(a.rot + (s * a.rot_a + k - a.rot_base) * 9, v[0], v[1], v[2], q0, q1, q2);
        }
    }
    const unsigned M = a.n_dirs;
    double best_d = __builtin_inf();
    uint32_t idx0 = 0;
    for (unsigned m0 = 0; m0 < M; m0 += LOOKUP_TILE_POINTS) {
        const unsigned cnt = M - m0 < LOOKUP_TILE_POINTS ? M - m0 : LOOKUP_TILE_POINTS;
        __syncthreads();
        for (unsigned j = threadIdx.x; j < 3 * cnt; j += LOOKUP_BLOCK) tile[j] = a.tab[3 * (size_t)m0 + j];
        __syncthreads();
        for (unsigned j = 0; j < cnt; ++j)
            lookup_nearest_step(tile[3 * j], tile[3 * j + 1], tile[3 * j + 2], q0, q1, q2, m0 + j, best_d, idx0);
    }
    if (live) a.idx0[i] = idx0;
    if (!STAGE2) return;

    const double qr0 = (double)(float)q0, qr1 = (double)(float)q1, qr2 = (double)(float)q2;
    const double a0 = a.tab[3 * (size_t)idx0], a1 = a.tab[3 * (size_t)idx0 + 1], a2 = a.tab[3 * (size_t)idx0 + 2];     // (idx0 < M in every lane)
    double best_o = __builtin_inf(), best_t = 0.0;
    uint32_t idx1 = idx0;
    for (unsigned m0 = 0; m0 < M; m0 += LOOKUP_TILE_POINTS) {
        const unsigned cnt = M - m0 < LOOKUP_TILE_POINTS ? M - m0 : LOOKUP_TILE_POINTS;
        __syncthreads();
        for (unsigned j = threadIdx.x; j < 3 * cnt; j += LOOKUP_BLOCK) tile[j] = a.tab[3 * (size_t)m0 + j];
        __syncthreads();
        for (unsigned j = 0; j < cnt; ++j)
            lookup_bracket_step(tile[3 * j], tile[3 * j + 1], tile[3 * j + 2], a0, a1, a2, qr0, qr1, qr2, m0 + j, best_o, idx1, best_t);
    }
    if (live) {
        a.idx1[i] = idx1;
        a.w[i] = lookup_weight(best_t);
    }
}

hipError_t lookup_launch(const LookupArgs &a, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    const unsigned grid = (a.n + LOOKUP_BLOCK - 1) / LOOKUP_BLOCK;
    if (a.idx1)
        hipLaunchKernelGGL(k_lookup<1>, dim3(grid), dim3(LOOKUP_BLOCK), 0, stream, a);
    else
        hipLaunchKernelGGL(k_lookup<0>, dim3(grid), dim3(LOOKUP_BLOCK), 0, stream, a);
    return hipGetLastError();
}

}  // namespace ohs
