// lookup_internal.h -- between api_lookup.hip (the C ABI of include/ohs_lookup.h) and lookup_kernels.hip (k_lookup and its launcher).
// libohs_lookup.so is these two units and nothing of the product's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ohs {

constexpr unsigned LOOKUP_TILE_POINTS = 1024;       // table points staged in LDS at a time: 24 KiB of f64
constexpr unsigned LOOKUP_BLOCK = 256;              // lanes per workgroup, one query each
constexpr size_t LOOKUP_CHUNK_QUERIES = size_t(1) << 18;    // queries per launch: 1 024 workgroups, 6 MiB of packed points

// one chunk of a call.  Every pointer is a DEVICE pointer.
struct LookupArgs {
    const double *tab;          // [n_dirs][3], the table's f32 coordinates widened
    uint32_t n_dirs;
    uint32_t n;                 // queries in this chunk (<= LOOKUP_CHUNK_QUERIES)
    // points: q[n][3].  rows (q == nullptr): query i is (s, k, c) of the flat index g0 + i = (s * n_segs + k) * K + c, its source the
    // entry s * src_a + k * src_b - src_base of src[..][K][3], its pose the entry s * rot_a + k - rot_base of rot[..][9] (rot ==
    // nullptr: the identity) -- the staged part of each array holds every entry the chunk names
    const double *q;
    const double *src;
    const double *rot;
    unsigned long long g0, n_segs, src_a, src_b, src_base, rot_a, rot_base;
    uint32_t K;
    uint32_t *idx0;             // [n]
    uint32_t *idx1;             // [n], or nullptr with w: nearest only
    float *w;
};

// queues the chunk on `stream`; -> hipGetLastError() behind the launch
hipError_t lookup_launch(const LookupArgs &a, hipStream_t stream);

}  // namespace ohs
