// scene_rows_kernels.hip -- k_scene_rows_seal: what the scene call's host scan (batch_process_objects_any, api_batch.hip) does to
// the rows of a three-direction call, on the device, where ohs_tracked_process keeps them.  One wave per (stream, segment) row of up to
// 64 objects: the row itself and the row in front of it are two loads of one shape, a pair's two objects sit in neighbouring lanes
// (or, four objects to a lane, in one), as the 64 change bits of k_conv_p1_objects_blend3 do.  Three jobs:
//   the planes in front of the call   the first segment's wave copies its own entries to front_out (FRESH; under CARRY the convolution
//                                     reads the carried rows themselves),
//   the carry                         the last segment's wave copies its entries to carry_out,
//   the launch record                 every wave counts its pairs' passes (scene_rows_body.hpp), sums them over the wave and adds them to
//                                     three 64-bit counters with one atomic each.
// Integer work only; plain C++.  Linked into libohs_tracked.so only.
#include "scene_rows_internal.h"
#include "scene_rows_body.hpp"

namespace ohs {

namespace {

// V consecutive words: one 32-bit or one 128-bit access (p is 4 V bytes aligned)
template <int V> struct RowWords;
template <> struct RowWords<1> {
    unsigned w[1];
    __device__ void load(const unsigned *p) { w[0] = *p; }
    __device__ void store(unsigned *p) const { *p = w[0]; }
};
template <> struct RowWords<4> {
    unsigned w[4];
    __device__ void load(const unsigned *p)
    {
        const uint4 v = *reinterpret_cast<const uint4 *>(p);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    }
    __device__ void store(unsigned *p) const { *reinterpret_cast<uint4 *>(p) = make_uint4(w[0], w[1], w[2], w[3]); }
};

// a pair's part of the record, five counts of at most 32 per wave in the bytes of one word
__device__ inline unsigned long long packed_counts(unsigned pair_flags)
{
    const SceneRowsPair p = scene_rows_pair(pair_flags);
    return (unsigned long long)p.fading | ((unsigned long long)p.cur4 << 8) | ((unsigned long long)p.cur6 << 16) |
           ((unsigned long long)p.old4 << 24) | ((unsigned long long)p.old6 << 32);
}

}  // namespace

// V objects per lane: 1, or 4 where K is a multiple of 4 (every row of every plane then starts on 16 bytes)
template <int V>
__global__ __launch_bounds__(SCENE_ROWS_BLOCK) void k_scene_rows_seal(SceneRowsArgs a)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned long long row = (unsigned long long)blockIdx.x * (SCENE_ROWS_BLOCK / 64u) + (threadIdx.x >> 6);   // (the wave's)
    if (row >= (unsigned long long)a.n_streams * a.n_segs) return;      // the whole wave
    const unsigned K = a.K;
    const unsigned long long s = row / a.n_segs, k = row - s * a.n_segs, front_plane = (unsigned long long)a.n_streams * K;
    // plane 0 of the row's entries and of the ones in front of them, and the plane stride that goes with each
    const unsigned *cur = a.rows + row * K;
    const bool carried = k == 0 && a.carry_in;
    const unsigned *old = k > 0 ? cur - K : carried ? a.carry_in + s * K : cur;
    const unsigned long long old_plane = carried ? front_plane : a.plane;
    const bool mine = lane * V < K;
    RowWords<V> c[SCENE_ROWS_PLANES], o[SCENE_ROWS_PLANES];
#pragma unroll
    for (unsigned pl = 0; pl < SCENE_ROWS_PLANES; ++pl) {
#pragma unroll
        for (int j = 0; j < V; ++j) c[pl].w[j] = o[pl].w[j] = 0u;       // (a lane beyond the row: entries of +0.0 that never change)
        if (mine) {
            c[pl].load(cur + pl * a.plane + lane * V);
            o[pl].load(old + pl * old_plane + lane * V);
        }
    }
    if (mine && k == 0 && a.front_out) {
#pragma unroll
        for (unsigned pl = 0; pl < SCENE_ROWS_PLANES; ++pl) c[pl].store(a.front_out + pl * front_plane + s * K + lane * V);
    }
    if (mine && k == scene_rows_carry_segment(a.n_segs)) {
#pragma unroll
        for (unsigned pl = 0; pl < SCENE_ROWS_PLANES; ++pl) c[pl].store(a.carry_out + pl * front_plane + s * K + lane * V);
    }
    unsigned f[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const SceneRowsEntry ce{c[0].w[j], c[1].w[j], c[2].w[j], c[3].w[j], c[4].w[j], c[5].w[j]};
        const SceneRowsEntry oe{o[0].w[j], o[1].w[j], o[2].w[j], o[3].w[j], o[4].w[j], o[5].w[j]};
        f[j] = scene_rows_object(ce, oe, a.fade != 0);
    }
    unsigned long long acc;
    if constexpr (V == 1) {     // the partner is the neighbouring lane; the even lane counts the pair
        const unsigned pair = f[0] | (unsigned)__shfl_xor((int)f[0], 1);
        acc = (lane & 1u) ? 0ull : packed_counts(pair);
    } else {
        acc = packed_counts(f[0] | f[1]) + packed_counts(f[2] | f[3]);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
    if (lane == 0) {
        const unsigned long long seg_len = scene_rows_seg_len(k, a.seg_blocks, a.n_blocks);
        const unsigned long long fading = acc & 0xffull, cur4 = (acc >> 8) & 0xffull, cur6 = (acc >> 16) & 0xffull;
        const unsigned long long old4 = (acc >> 24) & 0xffull, old6 = (acc >> 32) & 0xffull;
        const unsigned long long blended = cur4 * seg_len + old4, blended3 = cur6 * seg_len + old6;
        if (fading) atomicAdd(a.counts + 0, fading);
        if (blended) atomicAdd(a.counts + 1, blended);
        if (blended3) atomicAdd(a.counts + 2, blended3);
    }
}

hipError_t scene_rows_launch(const SceneRowsArgs &a, hipStream_t stream)
{
    const unsigned long long n_rows = (unsigned long long)a.n_streams * a.n_segs, per_block = SCENE_ROWS_BLOCK / 64u;
    if (n_rows == 0) return hipSuccess;
    const unsigned grid = (unsigned)((n_rows + per_block - 1) / per_block);
    if (a.K % 4u == 0u)
        hipLaunchKernelGGL(k_scene_rows_seal<4>, dim3(grid), dim3(SCENE_ROWS_BLOCK), 0, stream, a);
    else
        hipLaunchKernelGGL(k_scene_rows_seal<1>, dim3(grid), dim3(SCENE_ROWS_BLOCK), 0, stream, a);
    return hipGetLastError();
}

}  // namespace ohs
