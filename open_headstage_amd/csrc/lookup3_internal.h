// lookup3_internal.h -- between api_lookup3.hip (the C ABI of include/ohs_lookup3.h) and lookup3_kernels.hip (k_lookup_tri and its
// launcher).  libohs_lookup3.so is these two units and nothing of the product's or of libohs_lookup.so's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ohs {

constexpr unsigned LOOKUP3_TILE_TRIANGLES = 256;    // triangles' inverses staged in LDS at a time: 18 KiB of f64
constexpr unsigned LOOKUP3_BLOCK = 256;             // lanes per workgroup, one query each
constexpr size_t LOOKUP3_CHUNK_QUERIES = size_t(1) << 18;   // queries per launch: 1 024 workgroups, 6 MiB of packed points

// one chunk of a call.  Every pointer is a DEVICE pointer.
struct Lookup3Args {
    const double *inv;          // [n_tris][9], the triangles' inverses, row-major
    const uint32_t *tris;       // [n_tris][3], the triangles' corners
    uint32_t n_tris;
    uint32_t n;                 // queries in this chunk (<= LOOKUP3_CHUNK_QUERIES)
    // points: q[n][3].  rows (q == nullptr): query i is (s, k, c) of the flat index g0 + i = (s * n_segs + k) * K + c, its source the
    // entry s * src_a + k * src_b - src_base of src[..][K][3], its pose the entry s * rot_a + k - rot_base of rot[..][9] (rot ==
    // nullptr: the identity) -- the staged part of each array holds every entry the chunk names
    const double *q;
    const double *src;
    const double *rot;
    unsigned long long g0, n_segs, src_a, src_b, src_base, rot_a, rot_base;
    uint32_t K;
    uint32_t *idx0, *idx1, *idx2;   // [n] each
    float *w1, *w2;                 // [n] each
    uint32_t *tri;                  // [n], or nullptr: not asked for
};

// queues the chunk on `stream`; -> hipGetLastError() behind the launch
hipError_t lookup3_launch(const Lookup3Args &a, hipStream_t stream);

}  // namespace ohs
