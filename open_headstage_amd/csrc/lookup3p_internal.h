// lookup3p_internal.h -- between api_lookup3p.hip (the C ABI of include/ohs_lookup3p.h) and lookup3p_kernels.hip (k_lookup_tri_cells,
// k_lookup_tri_rest and their launcher).  libohs_lookup3p.so is these two units and nothing of the product's or of the other lookup
// libraries'.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ohs {

constexpr unsigned LOOKUP3P_TILE_TRIANGLES = 256;   // pass 2: triangles' inverses staged in LDS at a time, 20 KiB of f64 (rows of 10)
constexpr unsigned LOOKUP3P_BLOCK = 256;            // lanes per workgroup, one query each
constexpr size_t LOOKUP3P_CHUNK_QUERIES = size_t(1) << 18;  // queries per pair of launches

// one chunk of a call.  Every pointer is a DEVICE pointer.
struct Lookup3pArgs {
    const double *inv;          // [n_tris][LOOKUP3P_INV_STRIDE], the triangles' inverses, row-major, the tenth number unused
    const uint32_t *tris;       // [n_tris][3], the triangles' corners
    uint32_t n_tris;
    uint32_t n;                 // queries in this chunk (<= LOOKUP3P_CHUNK_QUERIES)
    // the index: cell_start[6 G^2 + 1], cell_tris[cell_start[6 G^2]], everywhere[n_everywhere]; B of the certificate
    const uint32_t *cell_start, *cell_tris, *everywhere;
    uint32_t grid, n_everywhere;
    double bound;
    // pass 1 appends the queries it does not certify: rest[*rest_count ..], *rest_count zeroed before the chunk; rest holds n entries
    uint32_t *rest, *rest_count;
    // the queries, as Lookup3Args names them (lookup3_internal.h): points q[n][3], or rows (q == nullptr) from src / rot
    const double *q;
    const double *src;
    const double *rot;
    unsigned long long g0, n_segs, src_a, src_b, src_base, rot_a, rot_base;
    uint32_t K;
    uint32_t *idx0, *idx1, *idx2;   // [n] each
    float *w1, *w2;                 // [n] each
    uint32_t *tri;                  // [n], or nullptr: not asked for
};

// queues the chunk's two passes on `stream` (pass 2 sized for the chunk: no host round trip); -> hipGetLastError() behind them
hipError_t lookup3p_launch(const Lookup3pArgs &a, hipStream_t stream);

}  // namespace ohs
