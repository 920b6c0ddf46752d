// delay2_kernels.hip -- k_object_delay2: per-object propagation delay, gain and a distance-dependent symmetric FIR (include/ohs_delay2.h),
// one lane per output frame, and k_delay2_history, the ordered second launch that moves the call's last frames into the ring.
//
// The stage's shape is k_object_delay's (delay_kernels.hip): a tile is DELAY2_TILE frames of one object of one stream inside one
// segment, its input window of at most DELAY2_LDS_WINDOW frames is staged in LDS with coalesced loads -- it may begin in the ring and
// end in the call's input --, a wider one is gathered from global memory.  The PASS is the segment row's: when the taps in front of
// the row and the row's own are both the identity by their bits, the tile runs delay_frame as libohs_delay.so does, bit for bit;
// every other row runs delay2_frame, whose window is the FIR's radius wider on each side and whose lanes read twelve inputs once
// into registers and form the four filtered nodes from them.  Rows, and with them the pass, are uniform across a workgroup.
#include "delay2_internal.h"
#include "delay2_body.hpp"

namespace ohs {

static_assert(DELAY2_FIR_TAPS == DELAY2_TAPS, "delay2_internal.h restates delay2_body.hpp's tap count");

namespace {

// frame m of the call for one object: the input where m >= 0, in front of it the ring (or silence)
struct Delay2Tap {
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

__global__ __launch_bounds__(DELAY2_TILE) void k_object_delay2(Delay2Args a)
{
    __shared__ float win[DELAY2_LDS_WINDOW];
    const unsigned tid = threadIdx.x, c = blockIdx.y, s = blockIdx.z;
    const unsigned long long n0 = (unsigned long long)blockIdx.x * DELAY2_TILE;
    const unsigned long long k = n0 / a.seg_frames, seg0 = k * a.seg_frames;
    const unsigned long long L = a.frames - seg0 < a.seg_frames ? a.frames - seg0 : a.seg_frames;
    const unsigned long long j0 = n0 - seg0;
    const unsigned long long row = (s * a.row_ss + k) * a.K + c, front = (unsigned long long)s * a.K + c;
    const double D = a.row_d[row], Dp = k ? a.row_d[row - a.K] : a.front_d[front];
    const float G = a.row_g[row], Gp = k ? a.row_g[row - a.K] : a.front_g[front];
    const Delay2Tap tap{a.in + s * a.in_ss + c * a.in_cs, a.ring + ((unsigned long long)s * a.max_objects + c) * a.R, (long long)a.R,
                        (long long)a.w, a.silent};
    float *out = a.out + s * a.out_ss + c * a.out_cs;
    float H[DELAY2_TAPS], Hp[DELAY2_TAPS];
    bool filtered = false;
    if (a.row_h) {
        const float *h = a.row_h + row * DELAY2_TAPS, *hp = k ? h - (unsigned long long)a.K * DELAY2_TAPS : a.front_h + front * DELAY2_TAPS;
        for (int r = 0; r < DELAY2_TAPS; ++r) H[r] = h[r], Hp[r] = hp[r];
        filtered = !(delay2_identity(H) && delay2_identity(Hp));
    }
    if (!filtered) {            // the plain pass: k_object_delay's body
        const DelayWindow wd = delay_window(Dp, D, j0, DELAY2_TILE, L, a.max_delay, (long long)n0);
        if (wd.width <= DELAY2_LDS_WINDOW) {
            for (unsigned q = tid; q < (unsigned)wd.width; q += DELAY2_TILE) win[q] = tap(wd.lo + q);
            __syncthreads();
            const long long lo = wd.lo;
            out[n0 + tid] = delay_frame(Dp, D, Gp, G, j0 + tid, L, a.max_delay, (long long)(n0 + tid), [&](long long m) { return win[m - lo]; });
        } else {
            if (tid == 0) atomicAdd(a.gather_tiles + (blockIdx.x + 7u * c + 131u * s) % DELAY2_COUNTERS, 1u);
            out[n0 + tid] = delay_frame(Dp, D, Gp, G, j0 + tid, L, a.max_delay, (long long)(n0 + tid), tap);
        }
        return;
    }
    const DelayWindow wd = delay2_window(Dp, D, j0, DELAY2_TILE, L, a.max_delay, (long long)n0);
    if (wd.width <= DELAY2_LDS_WINDOW) {
        for (unsigned q = tid; q < (unsigned)wd.width; q += DELAY2_TILE) win[q] = tap(wd.lo + q);
        __syncthreads();
        const long long lo = wd.lo;
        out[n0 + tid] = delay2_frame(Dp, D, Gp, G, Hp, H, j0 + tid, L, a.max_delay, (long long)(n0 + tid), [&](long long m) { return win[m - lo]; });
    } else {
        if (tid == 0) atomicAdd(a.gather_tiles + (blockIdx.x + 7u * c + 131u * s) % DELAY2_COUNTERS, 1u);
        out[n0 + tid] = delay2_frame(Dp, D, Gp, G, Hp, H, j0 + tid, L, a.max_delay, (long long)(n0 + tid), tap);
    }
}

// Behind k_object_delay2 on the same stream: the ring takes the call's last min(frames, R) frames at its write position; under
// `silent` all R entries are written, zeros in front of the call's first frame.  The caller moves w by frames % R.
__global__ __launch_bounds__(256) void k_delay2_history(Delay2Args a, unsigned long long count)
{
    const unsigned long long q = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= count) return;
    const unsigned c = blockIdx.y, s = blockIdx.z;
    const long long m = (long long)a.frames - 1 - (long long)q;                 // the frame, counted back from the call's last
    const unsigned long long at = (a.w + a.frames % a.R + a.R - 1 - q % a.R) % a.R;    // (q < R)
    a.ring[((unsigned long long)s * a.max_objects + c) * a.R + at] = m >= 0 ? a.in[s * a.in_ss + c * a.in_cs + m] : 0.0f;
}

hipError_t delay2_launch(const Delay2Args &a, hipStream_t stream)
{
    const dim3 grid((unsigned)(a.frames / DELAY2_TILE), a.K, a.n_streams);
    hipLaunchKernelGGL(k_object_delay2, grid, dim3(DELAY2_TILE), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const unsigned long long count = a.silent ? a.R : (a.frames < a.R ? a.frames : a.R);
    hipLaunchKernelGGL(k_delay2_history, dim3((unsigned)((count + 255) / 256), a.K, a.n_streams), dim3(256), 0, stream, a, count);
    return hipGetLastError();
}

}  // namespace ohs
