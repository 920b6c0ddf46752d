// delay2_body.hpp -- the FILTERED per-sample step of k_object_delay2 (include/ohs_delay2.h, THE ARITHMETIC), written so that it compiles
// for the host: tests/delay2_host_check.cpp includes it as it is.  The plain step is delay_body.hpp's delay_frame, unchanged; what is
// added here is the pass with a symmetric FIR of radius DELAY2_RADIUS on the four interpolation nodes, its lower clamp of the delay
// at 1 + DELAY2_RADIUS, and the wider window that goes with it.  Every operation rounds by itself: the units that include this are
// compiled with -ffp-contract=off.
#pragma once
#include "delay_body.hpp"

namespace ohs {

constexpr int DELAY2_RADIUS = 4;                        // OHS_DELAY2_FIR_RADIUS
constexpr int DELAY2_TAPS = DELAY2_RADIUS + 1;          // H_0 .. H_4: the centre and one side
constexpr int DELAY2_INPUTS = 4 + 2 * DELAY2_RADIUS;    // distinct inputs of one output frame: x[m-7 .. m+4]

// the identity (1.0f, +0, +0, +0, +0), by its bits: a row whose H' and H both are it takes the plain pass
OHS_DELAY_HD bool delay2_identity(const float h[DELAY2_TAPS])
{
    bool same = h[0] == 1.0f;
    for (int j = 1; j < DELAY2_TAPS; ++j) same = same && h[j] == 0.0f && !__builtin_signbit(h[j]);
    return same;
}

// delay_at with the filtered pass's lower clamp: Dp + (D - Dp) * a may round one ulp below both ends, and the newest input read,
// x[n - i + 1 + DELAY2_RADIUS], has to stay causal
OHS_DELAY_HD double delay2_at(double Dp, double D, unsigned long long j, unsigned long long L, double max_delay)
{
    const double a = (double)(j + 1) / (double)L;
    double d = Dp + (D - Dp) * a;
    d = d < (double)(1 + DELAY2_RADIUS) ? (double)(1 + DELAY2_RADIUS) : d;
    return d > max_delay ? max_delay : d;
}

// v = ((((h_0 x[t] + h_1 (x[t-1] + x[t+1])) + h_2 (x[t-2] + x[t+2])) + h_3 (x[t-3] + x[t+3])) + h_4 (x[t-4] + x[t+4])); x points at x[t]
OHS_DELAY_HD float delay2_node(const float h[DELAY2_TAPS], const float *x)
{
    float v = h[0] * x[0];
    for (int r = 1; r <= DELAY2_RADIUS; ++r) v = v + h[r] * (x[-r] + x[r]);
    return v;
}

// One filtered output frame.  `tap(m)` as in delay_frame; Hp and H are the taps in front of the segment and reached at its last
// frame.  The twelve inputs are read once, oldest first, and the four nodes formed from them.
template <class Tap>
OHS_DELAY_HD float delay2_frame(double Dp, double D, float Gp, float G, const float Hp[DELAY2_TAPS], const float H[DELAY2_TAPS],
                                unsigned long long j, unsigned long long L, double max_delay, long long n, Tap tap)
{
    const double d = delay2_at(Dp, D, j, L, max_delay);
    const long long i = delay_floor(d);
    const float f = (float)(d - (double)i);
    float c[4], h[DELAY2_TAPS], x[DELAY2_INPUTS];
    delay_weights(f, c);
    for (int r = 0; r < DELAY2_TAPS; ++r) h[r] = delay_gain_at(Hp[r], H[r], j, L);
    const long long m = n - i + 1;
    for (int q = 0; q < DELAY2_INPUTS; ++q) x[q] = tap(m - 3 - DELAY2_RADIUS + q);          // x[q] is frame m - 7 + q
    const float *at = x + 3 + DELAY2_RADIUS;                                                // frame m
    return delay_sample(c, delay_gain_at(Gp, G, j, L), delay2_node(h, at), delay2_node(h, at - 1), delay2_node(h, at - 2),
                        delay2_node(h, at - 3));
}

// The input window of a filtered tile: delay_window's, with delay2_at's clamp, DELAY2_RADIUS frames wider on each side.
OHS_DELAY_HD DelayWindow delay2_window(double Dp, double D, unsigned long long j0, unsigned T, unsigned long long L, double max_delay,
                                       long long n0)
{
    const long long ia = delay_floor(delay2_at(Dp, D, j0, L, max_delay)), ib = delay_floor(delay2_at(Dp, D, j0 + T - 1, L, max_delay));
    const long long i_lo = ia < ib ? ia : ib, i_hi = ia < ib ? ib : ia;
    DelayWindow w;
    w.lo = n0 - i_hi - 2 - DELAY2_RADIUS;
    w.width = (unsigned long long)(T + 3 + 2 * DELAY2_RADIUS + (i_hi - i_lo));
    return w;
}

}  // namespace ohs
