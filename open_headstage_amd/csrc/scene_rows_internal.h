// scene_rows_internal.h -- between api_tracked.hip (the C ABI of include/ohs_tracked.h) and scene_rows_kernels.hip (k_scene_rows_seal
// and its launcher).  Linked into libohs_tracked.so only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ohs {

constexpr unsigned SCENE_ROWS_BLOCK = 256;      // lanes per workgroup: four waves, one (stream, segment) row each
constexpr unsigned SCENE_ROWS_PLANES = 6;       // idx0, idx1, idx2, w1, w2, gain

// one call's rows.  Every pointer is a DEVICE pointer.
struct SceneRowsArgs {
    const unsigned *rows;           // [6][plane]: the planes the lookup and the gains' copy have filled, entry (s * n_segs + k) * K + c
    unsigned long long plane;       // n_streams * n_segs * K
    unsigned n_streams, n_segs, K;  // K in 1 .. 64
    const unsigned *carry_in;       // [6][n_streams][K], the rows carried out of the previous call; nullptr: none (FRESH)
    unsigned *front_out;            // [6][n_streams][K], written with the first segment's own entries; nullptr: not wanted (CARRY)
    unsigned *carry_out;            // [6][n_streams][K], written with the last segment's entries (never carry_in's buffer)
    int fade;                       // CROSSFADE: changes against the entries in front are looked for
    unsigned seg_blocks, n_blocks;
    unsigned long long *counts;     // [3]: fading, blended (four rows), blended3 (six rows) passes, zeroed before the launch
};

// queues k_scene_rows_seal on `stream`; -> hipGetLastError() behind it
hipError_t scene_rows_launch(const SceneRowsArgs &a, hipStream_t stream);

}  // namespace ohs
