// delay_kernels.hip -- k_object_delay: per-object propagation delay and gain (include/ohs_delay.h), one lane per output frame, and
// k_delay_history, the ordered second launch that moves the call's last frames into the ring.  No recurrence, 4 bytes in and 4 out
// per sample: the job is memory-bound.
//
// A tile is DELAY_TILE frames of one object of one stream and lies inside one segment, where the delay ramp is monotone: the tile's
// input window follows from the delays at its two ends (delay_window).  A window of at most DELAY_LDS_WINDOW frames is staged in
// LDS with coalesced loads -- it may begin in the ring and end in the call's input -- and every lane reads its four taps there;
// a wider one (a jump of thousands of frames inside a segment) is gathered, four global loads per lane.  The choice is the tile's:
// every lane computes it from the same two delays.  8 KiB of LDS leave the eight workgroups a CU's wave slots admit their room.
#include "delay_internal.h"
#include "delay_body.hpp"

namespace ohs {

namespace {

// frame m of the call for one object: the input where m >= 0, in front of it the ring (or silence)
struct DelayTap {
    const float *in;
    const float *ring;
    long long R, w;
    int silent;
    __device__ float operator()(long long m) const
    {
        if (m >= 0) return in[m];
        if (silent) return 0.0f;
        long long at = w + m;           // m >= -R, 0 <= w < R
        if (at < 0) at += R;
        return ring[at];
    }
};

}  // namespace

__global__ __launch_bounds__(DELAY_TILE) void k_object_delay(DelayArgs a)
{
    __shared__ float win[DELAY_LDS_WINDOW];
    const unsigned tid = threadIdx.x, c = blockIdx.y, s = blockIdx.z;
    const unsigned long long n0 = (unsigned long long)blockIdx.x * DELAY_TILE;
    const unsigned long long k = n0 / a.seg_frames, seg0 = k * a.seg_frames;
    const unsigned long long L = a.frames - seg0 < a.seg_frames ? a.frames - seg0 : a.seg_frames;
    const unsigned long long j0 = n0 - seg0;
    const unsigned long long row = (s * a.row_ss + k) * a.K + c, front = (unsigned long long)s * a.K + c;
    const double D = a.row_d[row], Dp = k ? a.row_d[row - a.K] : a.front_d[front];
    const float G = a.row_g[row], Gp = k ? a.row_g[row - a.K] : a.front_g[front];
    const DelayTap tap{a.in + s * a.in_ss + c * a.in_cs, a.ring + ((unsigned long long)s * a.max_objects + c) * a.R, (long long)a.R,
                       (long long)a.w, a.silent};
    float *out = a.out + s * a.out_ss + c * a.out_cs;
    const DelayWindow wd = delay_window(Dp, D, j0, DELAY_TILE, L, a.max_delay, (long long)n0);
    if (wd.width <= DELAY_LDS_WINDOW) {
        for (unsigned q = tid; q < (unsigned)wd.width; q += DELAY_TILE) win[q] = tap(wd.lo + q);
        __syncthreads();
        const long long lo = wd.lo;
        out[n0 + tid] = delay_frame(Dp, D, Gp, G, j0 + tid, L, a.max_delay, (long long)(n0 + tid), [&](long long m) { return win[m - lo]; });
    } else {
        if (tid == 0) atomicAdd(a.gather_tiles + (blockIdx.x + 7u * c + 131u * s) % DELAY_COUNTERS, 1u);
        out[n0 + tid] = delay_frame(Dp, D, Gp, G, j0 + tid, L, a.max_delay, (long long)(n0 + tid), tap);
    }
}

// Behind k_object_delay on the same stream: the ring takes the call's last min(frames, R) frames at its write position; under
// `silent` all R entries are written, zeros in front of the call's first frame.  The caller moves w by frames % R.
__global__ __launch_bounds__(256) void k_delay_history(DelayArgs a, unsigned long long count)
{
    const unsigned long long q = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= count) return;
    const unsigned c = blockIdx.y, s = blockIdx.z;
    const long long m = (long long)a.frames - 1 - (long long)q;                 // the frame, counted back from the call's last
    const unsigned long long at = (a.w + a.frames % a.R + a.R - 1 - q % a.R) % a.R;    // (q < R)
    a.ring[((unsigned long long)s * a.max_objects + c) * a.R + at] = m >= 0 ? a.in[s * a.in_ss + c * a.in_cs + m] : 0.0f;
}

hipError_t delay_launch(const DelayArgs &a, hipStream_t stream)
{
    const dim3 grid((unsigned)(a.frames / DELAY_TILE), a.K, a.n_streams);
    hipLaunchKernelGGL(k_object_delay, grid, dim3(DELAY_TILE), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const unsigned long long count = a.silent ? a.R : (a.frames < a.R ? a.frames : a.R);
    hipLaunchKernelGGL(k_delay_history, dim3((unsigned)((count + 255) / 256), a.K, a.n_streams), dim3(256), 0, stream, a, count);
    return hipGetLastError();
}

}  // namespace ohs
