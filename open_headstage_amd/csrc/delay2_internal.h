// delay2_internal.h -- between api_delay2.hip (the C ABI of include/ohs_delay2.h) and delay2_kernels.hip (k_object_delay2,
// k_delay2_history and their launcher).  libohs_delay2.so is these two units and nothing of the product's or of libohs_delay.so's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ohs {

constexpr unsigned DELAY2_TILE = 256;           // output frames per workgroup, one lane each; a 512-frame block is two tiles
constexpr unsigned DELAY2_LDS_WINDOW = 2048;    // input frames a tile may stage in LDS (8 KiB): a tile whose window is wider gathers
constexpr unsigned DELAY2_COUNTERS = 1024;      // gather tiles are counted in this many words, spread by tile
constexpr unsigned DELAY2_FIR_TAPS = 5;         // H_0 .. H_4 per row (delay2_body.hpp, DELAY2_TAPS)

// one call.  Every pointer is a DEVICE pointer.
struct Delay2Args {
    const float *in;            // [stream][K][frames] with the two strides
    float *out;
    unsigned long long in_ss, in_cs, out_ss, out_cs;
    unsigned long long frames;          // of the call, a multiple of 512
    unsigned long long seg_frames;      // seg_blocks * 512; the last segment may be short
    unsigned long long n_segs;
    unsigned K, n_streams;
    // rows: entry (s * row_ss + k) * K + c, row_ss = 0 (one row for all streams) or n_segs; front: [s * K + c], what stands in front
    // of the first segment.  row_h / front_h: five taps per entry, or both NULL -- an unfiltered call, every tile takes the plain pass
    const double *row_d, *front_d;
    const float *row_g, *front_g;
    const float *row_h, *front_h;
    unsigned long long row_ss;
    double max_delay;
    // the history: a ring of R = max_delay + 2 + the FIR's radius frames per stream and object, [stream][max_objects][R]; the frame in
    // front of the call is at (w + R - 1) % R.  silent: frames in front of the call read as 0 whatever the ring holds
    float *ring;
    unsigned long long R, w;
    unsigned max_objects;
    int silent;
    unsigned *gather_tiles;     // [DELAY2_COUNTERS], zeroed in front of the call
};

// queues k_object_delay2 and, behind it, k_delay2_history (the ring takes the call's last R frames) on `stream`;
// -> hipGetLastError() behind the launches
hipError_t delay2_launch(const Delay2Args &a, hipStream_t stream);

}  // namespace ohs
