// lookup3_kernels.hip -- k_lookup_tri: for every query the triangle of the mesh it stands in, that triangle's corners in the order of
// their shares and the two smaller shares (include/ohs_lookup3.h, THE ARITHMETIC).
//
// One query per lane.  The triangles' inverses are walked in ascending t, LOOKUP3_TILE_TRIANGLES at a time through LDS: the workgroup
// copies a tile (coalesced), every lane then reads the same address per step -- a broadcast read, no bank conflict.  A lane carries its
// best min(g) and the t it stood at, nothing else: the running maximum under strict > keeps the first of equals, and since no lane shares
// its query with another there is no merge across lanes or waves to get that rule wrong.  The winner's nine numbers are gathered once
// behind the walk and its gains computed again -- the same operations on the same numbers, so the same bits.  Outputs are plain vector
// stores.  Compiled with -ffp-contract=off: lookup3_body.hpp's operations round one by one.
#include "lookup3_internal.h"
#include "lookup3_body.hpp"

namespace ohs {

__global__ __launch_bounds__(LOOKUP3_BLOCK) void k_lookup_tri(const double *__restrict__ inv, Lookup3Args a)
{
    __shared__ __attribute__((aligned(16))) double tile[LOOKUP3_TILE_TRIANGLES * 9];
    const unsigned i = blockIdx.x * LOOKUP3_BLOCK + threadIdx.x;
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
    q0 = lookup3_round(q0), q1 = lookup3_round(q1), q2 = lookup3_round(q2);
    const unsigned T = a.n_tris;
    double best = -__builtin_inf();
    uint32_t tri = 0;
    for (unsigned t0 = 0; t0 < T; t0 += LOOKUP3_TILE_TRIANGLES) {
        const unsigned cnt = T - t0 < LOOKUP3_TILE_TRIANGLES ? T - t0 : LOOKUP3_TILE_TRIANGLES;
        __syncthreads();
        for (unsigned j = threadIdx.x; j < 9 * cnt; j += LOOKUP3_BLOCK) tile[j] = inv[9 * (size_t)t0 + j];
        __syncthreads();
#pragma unroll 4
        for (unsigned j = 0; j < cnt; ++j) lookup3_step(tile + 9 * j, q0, q1, q2, t0 + j, best, tri);
    }
    if (!live) return;
    // (tri < T in every lane: it starts at 0 and moves only to a t that was walked)
    double w[9];
    for (int j = 0; j < 9; ++j) w[j] = inv[9 * (size_t)tri + j];
    const uint32_t v[3] = {a.tris[3 * (size_t)tri], a.tris[3 * (size_t)tri + 1], a.tris[3 * (size_t)tri + 2]};
    const Lookup3Row r = lookup3_winner(w, v, q0, q1, q2);
    a.idx0[i] = r.idx0, a.idx1[i] = r.idx1, a.idx2[i] = r.idx2;
    a.w1[i] = r.w1, a.w2[i] = r.w2;
    if (a.tri) a.tri[i] = tri;
}

hipError_t lookup3_launch(const Lookup3Args &a, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    const unsigned grid = (a.n + LOOKUP3_BLOCK - 1) / LOOKUP3_BLOCK;
    hipLaunchKernelGGL(k_lookup_tri, dim3(grid), dim3(LOOKUP3_BLOCK), 0, stream, a.inv, a);
    return hipGetLastError();
}

}  // namespace ohs
