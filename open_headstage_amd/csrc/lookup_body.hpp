// lookup_body.hpp -- the per-point steps of the direction lookup (include/ohs_lookup.h, THE ARITHMETIC), once for the device and the
// host: k_lookup (lookup_kernels.hip) inlines them, and tests/test_cpu_lookup.py compiles this header into a stand-alone program and
// holds it to tests/lookup_model.py's bits.  Everything is f64, every operation is its own statement's rounding: the units that include
// this are compiled with -ffp-contract=off, and nothing here calls fma.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define OHS_LK_HD __host__ __device__
#else
#define OHS_LK_HD
#endif

namespace ohs {

// q = R^T v, R row-major 3 x 3: q[i] = (R[0][i] v[0] + R[1][i] v[1]) + R[2][i] v[2]
OHS_LK_HD inline void lookup_pose(const double *R, double v0, double v1, double v2, double &q0, double &q1, double &q2)
{
    q0 = (R[0] * v0 + R[3] * v1) + R[6] * v2;
    q1 = (R[1] * v0 + R[4] * v1) + R[7] * v2;
    q2 = (R[2] * v0 + R[5] * v1) + R[8] * v2;
}

// stage 1 at table point m = (p0, p1, p2): D = |P[m] - q|^2; the running minimum under strict <, so that ascending m keeps the first of
// equally near points.  best_d starts at +infinity.
OHS_LK_HD inline void lookup_nearest_step(double p0, double p1, double p2, double q0, double q1, double q2, uint32_t m, double &best_d,
                                          uint32_t &best_m)
{
    const double d0 = p0 - q0, d1 = p1 - q1, d2 = p2 - q2;
    const double D = (d0 * d0 + d1 * d1) + d2 * d2;
    if (D < best_d) {
        best_d = D;
        best_m = m;
    }
}

// stage 2 at table point m = (p0, p1, p2): the chord from a = P[idx0] to it, the query qr (q in f32's precision) projected onto the
// chord and clamped, the offset's square O; the running minimum under strict <.  best_o starts at +infinity, best_t at 0, best_m at
// idx0: a table of copies of P[idx0] leaves them there.
OHS_LK_HD inline void lookup_bracket_step(double p0, double p1, double p2, double a0, double a1, double a2, double qr0, double qr1,
                                          double qr2, uint32_t m, double &best_o, uint32_t &best_m, double &best_t)
{
    const double c0 = p0 - a0, c1 = p1 - a1, c2 = p2 - a2;
    const double L = (c0 * c0 + c1 * c1) + c2 * c2;
    if (!(L > 0.0)) return;
    const double e0 = qr0 - a0, e1 = qr1 - a1, e2 = qr2 - a2;
    double t = ((c0 * e0 + c1 * e1) + c2 * e2) / L;
    t = t < 0.0 ? 0.0 : t;
    t = t > 1.0 ? 1.0 : t;
    const double o0 = (a0 + t * c0) - qr0, o1 = (a1 + t * c1) - qr1, o2 = (a2 + t * c2) - qr2;
    const double O = (o0 * o0 + o1 * o1) + o2 * o2;
    if (O < best_o) {
        best_o = O;
        best_m = m;
        best_t = t;
    }
}

// w as it is written: (float)t, a zero of either sign as +0.0 (+0.0 is what lets a pair take the one-direction pass of
// k_conv_p1_objects_blend)
OHS_LK_HD inline float lookup_weight(double t)
{
    const float w = (float)t;
    return w == 0.0f ? 0.0f : w;
}

}  // namespace ohs
