// delay_body.hpp -- the per-sample step of k_object_delay (include/ohs_delay.h, THE ARITHMETIC), written so that it compiles for the host:
// tests/delay_host_check.cpp includes it as it is.  Every operation rounds by itself: the units that include it are compiled with
// -ffp-contract=off, and nothing here is a fused multiply-add.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define OHS_DELAY_HD __host__ __device__ inline
#else
#define OHS_DELAY_HD inline
#endif

namespace ohs {

constexpr float DELAY_SIXTH = 0x1.555556p-3f;       // 1/6 as the nearest f32

// floor of a double in [1, 65536]: the truncation is exact
OHS_DELAY_HD long long delay_floor(double d) { return (long long)d; }

// the delay of frame j of a segment of L frames between Dp (in front of it) and D (reached at its last frame), clamped
OHS_DELAY_HD double delay_at(double Dp, double D, unsigned long long j, unsigned long long L, double max_delay)
{
    const double a = (double)(j + 1) / (double)L;
    double d = Dp + (D - Dp) * a;
    d = d < 1.0 ? 1.0 : d;
    return d > max_delay ? max_delay : d;
}

OHS_DELAY_HD float delay_gain_at(float Gp, float G, unsigned long long j, unsigned long long L)
{
    const double a = (double)(j + 1) / (double)L;
    return (float)((double)Gp + ((double)G - (double)Gp) * a);
}

// the four weights on the nodes -1, 0, 1, 2 at the fraction f (0 <= f <= 1; f == 1 picks the next tap exactly)
OHS_DELAY_HD void delay_weights(float f, float c[4])
{
    const float fm1 = f - 1.0f, fm2 = f - 2.0f, fp1 = f + 1.0f;
    c[0] = ((f * fm1) * fm2) * -DELAY_SIXTH;
    c[1] = ((fp1 * fm1) * fm2) * 0.5f;
    c[2] = ((fp1 * f) * fm2) * -0.5f;
    c[3] = ((fp1 * f) * fm1) * DELAY_SIXTH;
}

// y = g (((c_-1 x[n-i+1] + c_0 x[n-i]) + c_1 x[n-i-1]) + c_2 x[n-i-2]); x0 .. x3 are the taps in that order
OHS_DELAY_HD float delay_sample(const float c[4], float g, float x0, float x1, float x2, float x3)
{
    return g * (((c[0] * x0 + c[1] * x1) + c[2] * x2) + c[3] * x3);
}

// One output frame: `tap(m)` is the input at frame m of the call (m < 0: the history, -1 the frame in front of the call).
template <class Tap>
OHS_DELAY_HD float delay_frame(double Dp, double D, float Gp, float G, unsigned long long j, unsigned long long L, double max_delay,
                               long long n, Tap tap)
{
    const double d = delay_at(Dp, D, j, L, max_delay);
    const long long i = delay_floor(d);
    const float f = (float)(d - (double)i);
    float c[4];
    delay_weights(f, c);
    const long long m = n - i + 1;
    return delay_sample(c, delay_gain_at(Gp, G, j, L), tap(m), tap(m - 1), tap(m - 2), tap(m - 3));
}

// The input window of a tile of T frames that starts at frame j0 of its segment and frame n0 of the call.  Inside a segment the
// rounded delay is monotone in j (the quotient is monotone in j, the product in the quotient, the sum in the product, the clamps
// and the floor in the sum), so the two ends bound every whole delay of the tile: the taps lie in [lo, lo + width).
struct DelayWindow {
    long long lo;
    unsigned long long width;
};

OHS_DELAY_HD DelayWindow delay_window(double Dp, double D, unsigned long long j0, unsigned T, unsigned long long L, double max_delay,
                                      long long n0)
{
    const long long ia = delay_floor(delay_at(Dp, D, j0, L, max_delay)), ib = delay_floor(delay_at(Dp, D, j0 + T - 1, L, max_delay));
    const long long i_lo = ia < ib ? ia : ib, i_hi = ia < ib ? ib : ia;
    DelayWindow w;
    w.lo = n0 - i_hi - 2;                                       // the last frame's oldest tap at the longest delay
    w.width = (unsigned long long)(T + 3 + (i_hi - i_lo));      // ... up to frame n0 + T - i_lo, the last frame's newest at the shortest
    return w;
}

}  // namespace ohs
