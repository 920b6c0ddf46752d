// delay_internal.h -- between api_delay.hip (the C ABI of include/ohs_delay.h) and delay_kernels.hip (k_object_delay, k_delay_history and
// their launcher).  libohs_delay.so is these two units and nothing of the product's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ohs {

constexpr unsigned DELAY_TILE = 256;            // output frames per workgroup, one lane each; a 512-frame block is two tiles
constexpr unsigned DELAY_LDS_WINDOW = 2048;     // input frames a tile may stage in LDS (8 KiB): a tile whose window is wider gathers
constexpr unsigned DELAY_COUNTERS = 1024;       // gather tiles are counted in this many words, spread by tile

// one call.  Every pointer is a DEVICE pointer.
struct DelayArgs {
    const float *in;            // [stream][K][frames] with the two strides
    float *out;
    unsigned long long in_ss, in_cs, out_ss, out_cs;
    unsigned long long frames;          // of the call, a multiple of 512
    unsigned long long seg_frames;      // seg_blocks * 512; the last segment may be short
    unsigned long long n_segs;
    unsigned K, n_streams;
    // rows: entry (s * row_ss + k) * K + c, row_ss = 0 (one row for all streams) or n_segs; front: [s * K + c], what stands in front
    // of the first segment
    const double *row_d, *front_d;
    const float *row_g, *front_g;
    unsigned long long row_ss;
    double max_delay;
    // the history: a ring of R = max_delay + 2 frames per stream and object, [stream][max_objects][R]; the frame in front of the call
    // is at (w + R - 1) % R.  silent: frames in front of the call read as 0 whatever the ring holds
    float *ring;
    unsigned long long R, w;
    unsigned max_objects;
    int silent;
    unsigned *gather_tiles;     // [DELAY_COUNTERS], zeroed in front of the call
};

// queues k_object_delay and, behind it, k_delay_history (the ring takes the call's last R frames) on `stream`;
// -> hipGetLastError() behind the launches
hipError_t delay_launch(const DelayArgs &a, hipStream_t stream);

}  // namespace ohs
