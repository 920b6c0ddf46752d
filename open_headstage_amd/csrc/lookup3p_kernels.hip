// lookup3p_kernels.hip -- k_lookup_tri_cells and k_lookup_tri_rest: the three-direction lookup of lookup3_kernels.hip with the walk
// pruned by a cube-map index over directions, and the same bits (include/ohs_lookup3p.h, HOW EXACTNESS IS KEPT; DESIGN.md section
// 4.5m).
//
// Pass 1, k_lookup_tri_cells: one query per lane, formed as k_lookup_tri forms it.  The lane finds its cell and walks the everywhere
// list and the cell's list merged in ascending t (lookup3p_walk), gathering each candidate's inverse from global memory (rows of 80
// bytes, five 16-byte loads).  Where its best min(g) exceeds the certificate's tau the answer is the full walk's: the lane recomputes
// the winner and writes the row.  Where not, the lane appends its query's index to the chunk's rest list -- one atomicAdd per wave
// through a ballot -- and writes nothing.
// Pass 2, k_lookup_tri_rest: k_lookup_tri's walk over every triangle through LDS tiles, for the queries on the rest list only.  The
// grid is sized for the chunk; a workgroup beyond the count leaves, all lanes together, before any barrier.
// Outputs are plain vector stores.  Compiled with -ffp-contract=off: the bodies' operations round one by one.
#include "lookup3p_internal.h"
#include "lookup3p_body.hpp"

namespace ohs {

// query i of the chunk: the point, posed for rows, rounded to f32 and widened (k_lookup_tri's steps)
__device__ inline void lookup3p_query(const Lookup3pArgs &a, unsigned i, double &q0, double &q1, double &q2)
{
    if (a.q) {
        q0 = a.q[3 * (size_t)i], q1 = a.q[3 * (size_t)i + 1], q2 = a.q[3 * (size_t)i + 2];
    } else {
        const unsigned long long g = a.g0 + i, sk = g / a.K, c = g - sk * a.K;
        const unsigned long long s = sk / a.n_segs, k = sk - s * a.n_segs;
        const double *v = a.src + ((s * a.src_a + k * a.src_b - a.src_base) * a.K + c) * 3;
        q0 = v[0], q1 = v[1], q2 = v[2];
        if (a.rot) lookup_pose(a.rot + (s * a.rot_a + k - a.rot_base) * 9, v[0], v[1], v[2], q0, q1, q2);
    }
    q0 = lookup3_round(q0), q1 = lookup3_round(q1), q2 = lookup3_round(q2);
}

__device__ inline void lookup3p_store(const Lookup3pArgs &a, unsigned i, uint32_t tri, double q0, double q1, double q2)
{
    double w[9];
    for (int j = 0; j < 9; ++j) w[j] = a.inv[LOOKUP3P_INV_STRIDE * (size_t)tri + j];
    const uint32_t v[3] = {a.tris[3 * (size_t)tri], a.tris[3 * (size_t)tri + 1], a.tris[3 * (size_t)tri + 2]};
    const Lookup3Row r = lookup3_winner(w, v, q0, q1, q2);
    a.idx0[i] = r.idx0, a.idx1[i] = r.idx1, a.idx2[i] = r.idx2;
    a.w1[i] = r.w1, a.w2[i] = r.w2;
    if (a.tri) a.tri[i] = tri;
}

__global__ __launch_bounds__(LOOKUP3P_BLOCK) void k_lookup_tri_cells(Lookup3pArgs a)
{
    const unsigned i = blockIdx.x * LOOKUP3P_BLOCK + threadIdx.x;
    const bool live = i < a.n;          // (a lane beyond the chunk stays for the ballot and stores nothing)
    double q0 = 0.0, q1 = 0.0, q2 = 0.0, best = -__builtin_inf();
    uint32_t tri = 0;
    bool rest = false;
    if (live) {
        lookup3p_query(a, i, q0, q1, q2);
        const uint32_t cell = lookup3p_cell(q0, q1, q2, a.grid);       // (< 6 G^2 for every input)
        const uint32_t lo = a.cell_start[cell], hi = a.cell_start[cell + 1];
        lookup3p_walk(a.inv, a.everywhere, a.n_everywhere, a.cell_tris + lo, hi - lo, q0, q1, q2, best, tri);
        rest = !(best > lookup3p_tau(a.bound, q0, q1, q2));
        // (tri < T where the answer stands: best moved off -infinity at a listed triangle)
        if (!rest) lookup3p_store(a, i, tri, q0, q1, q2);
    }
    const unsigned long long mask = __ballot(rest);
    if (mask) {
        const unsigned lane = __lane_id();
        const int leader = __ffsll((long long)mask) - 1;
        unsigned base = 0;
        if ((int)lane == leader) base = atomicAdd(a.rest_count, (unsigned)__popcll(mask));
        base = __shfl(base, leader);
        // (the chunk's n lanes append at most n entries in all: below the list's n)
        if (rest) a.rest[base + __popcll(mask & ((1ull << lane) - 1ull))] = i;
    }
}

__global__ __launch_bounds__(LOOKUP3P_BLOCK) void k_lookup_tri_rest(Lookup3pArgs a)
{
    __shared__ __attribute__((aligned(16))) double tile[LOOKUP3P_TILE_TRIANGLES * LOOKUP3P_INV_STRIDE];
    const unsigned count = *a.rest_count;       // (<= a.n: pass 1 has finished)
    if (blockIdx.x * LOOKUP3P_BLOCK >= count) return;       // the whole workgroup, before any barrier
    const unsigned k = blockIdx.x * LOOKUP3P_BLOCK + threadIdx.x;
    const bool live = k < count;                // (a lane beyond the list walks along for the barriers and stores nothing)
    const unsigned i = live ? a.rest[k] : 0;
    double q0 = 0.0, q1 = 0.0, q2 = 0.0;
    if (live) lookup3p_query(a, i, q0, q1, q2);
    const unsigned T = a.n_tris;
    double best = -__builtin_inf();
    uint32_t tri = 0;
    for (unsigned t0 = 0; t0 < T; t0 += LOOKUP3P_TILE_TRIANGLES) {
        const unsigned cnt = T - t0 < LOOKUP3P_TILE_TRIANGLES ? T - t0 : LOOKUP3P_TILE_TRIANGLES;
        __syncthreads();
        for (unsigned j = threadIdx.x; j < LOOKUP3P_INV_STRIDE * cnt; j += LOOKUP3P_BLOCK) tile[j] = a.inv[LOOKUP3P_INV_STRIDE * (size_t)t0 + j];
        __syncthreads();
#pragma unroll 4
        for (unsigned j = 0; j < cnt; ++j) lookup3_step(tile + LOOKUP3P_INV_STRIDE * j, q0, q1, q2, t0 + j, best, tri);
    }
    if (!live) return;
    lookup3p_store(a, i, tri, q0, q1, q2);
}

hipError_t lookup3p_launch(const Lookup3pArgs &a, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    const unsigned grid = (a.n + LOOKUP3P_BLOCK - 1) / LOOKUP3P_BLOCK;
    hipLaunchKernelGGL(k_lookup_tri_cells, dim3(grid), dim3(LOOKUP3P_BLOCK), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_lookup_tri_rest, dim3(grid), dim3(LOOKUP3P_BLOCK), 0, stream, a);
    return hipGetLastError();
}

}  // namespace ohs
