// lookup3_body.hpp -- the per-triangle and per-winner steps of the three-direction lookup (include/ohs_lookup3.h, THE ARITHMETIC), once
// for the device and the host: k_lookup_tri (lookup3_kernels.hip) inlines the walk and the winner, api_lookup3.hip the inverses, and
// tests/test_cpu_lookup3.py compiles this header into a stand-alone program and holds it to tests/lookup3_model.py's bits.  Everything
// is f64, every operation is its own statement's rounding: the units that include this are compiled with -ffp-contract=off, and nothing
// here calls fma.
#pragma once
#include <math.h>
#include <stdint.h>

#include "lookup_body.hpp"      // (lookup_pose, lookup_weight, OHS_LK_HD)

namespace ohs {

// the inverse of the vertex matrix [a b c] (columns) by cofactors, inv[3 i + j] = row_i[j] / det; -> false: the triangle is singular
// (|det| <= 1e-9 |a| |b| |c|, or not-a-number) and inv is not to be used
OHS_LK_HD inline bool lookup3_inverse(const double *a, const double *b, const double *c, double *inv)
{
    const double bc[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
    const double ca[3] = {c[1] * a[2] - c[2] * a[1], c[2] * a[0] - c[0] * a[2], c[0] * a[1] - c[1] * a[0]};
    const double ab[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const double det = (a[0] * bc[0] + a[1] * bc[1]) + a[2] * bc[2];
    const double na = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    const double nb = sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
    const double nc = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    if (!(fabs(det) > 1e-9 * ((na * nb) * nc))) return false;
    for (int j = 0; j < 3; ++j) {
        inv[j] = bc[j] / det;
        inv[3 + j] = ca[j] / det;
        inv[6 + j] = ab[j] / det;
    }
    return true;
}

// the query as the walk sees it: rounded to f32 and widened (|x| <= 3e30 on every path that reaches this: finite in f32)
OHS_LK_HD inline double lookup3_round(double x) { return (double)(float)x; }

// the query's gains over the triangle whose inverse is inv[9]
OHS_LK_HD inline void lookup3_gains(const double *inv, double q0, double q1, double q2, double &g0, double &g1, double &g2)
{
    g0 = (inv[0] * q0 + inv[1] * q1) + inv[2] * q2;
    g1 = (inv[3] * q0 + inv[4] * q1) + inv[5] * q2;
    g2 = (inv[6] * q0 + inv[7] * q1) + inv[8] * q2;
}

// the walk at triangle t: the running maximum of min(g) under strict >, so that ascending t keeps the first of equals.  best starts at
// -infinity, best_t at 0; no gain is not-a-number (the inverses and the queries are finite and bounded).
OHS_LK_HD inline void lookup3_step(const double *inv, double q0, double q1, double q2, uint32_t t, double &best, uint32_t &best_t)
{
    double g0, g1, g2;
    lookup3_gains(inv, q0, q1, q2, g0, g1, g2);
    const double m = fmin(fmin(g0, g1), g2);        // (no not-a-number here; which zero of a pair it returns does not reach the comparison)
    best_t = m > best ? t : best_t;
    best = fmax(best, m);
}

struct Lookup3Row {
    uint32_t idx0, idx1, idx2;
    float w1, w2;
};

// at the winner: its inverse inv[9] and its corners v[3] -> the row
OHS_LK_HD inline Lookup3Row lookup3_winner(const double *inv, const uint32_t *v, double q0, double q1, double q2)
{
    double g[3];
    lookup3_gains(inv, q0, q1, q2, g[0], g[1], g[2]);
    const double t01 = g[0] > g[1] ? g[0] : g[1], top = t01 > g[2] ? t01 : g[2];
    const double bar = top * 0x1p-20;
    double k[3];
    for (int i = 0; i < 3; ++i) {
        k[i] = g[i] > bar ? g[i] : 0.0;
        k[i] = k[i] < 0.0 ? 0.0 : k[i];
    }
    double s = (k[0] + k[1]) + k[2];
    if (!(s > 0.0)) {
        const int at = g[0] == top ? 0 : (g[1] == top ? 1 : 2);
        for (int i = 0; i < 3; ++i) k[i] = i == at ? 1.0 : 0.0;
        s = 1.0;
    }
    double w0 = k[0] / s, w1 = k[1] / s, w2 = k[2] / s;
    uint32_t v0 = v[0], v1 = v[1], v2 = v[2];
    // three compare-and-swaps: descending weight, equal weights (a zero of either sign is a zero) by ascending index
#define OHS_LK3_ORDER(wa, va, wb, vb)                          \
    if (wb > wa || (wb == wa && vb < va)) {                    \
        const double tw = wa;                                  \
        const uint32_t tv = va;                                \
        wa = wb, va = vb, wb = tw, vb = tv;                    \
    }
    OHS_LK3_ORDER(w0, v0, w1, v1)
    OHS_LK3_ORDER(w1, v1, w2, v2)
    OHS_LK3_ORDER(w0, v0, w1, v1)
#undef OHS_LK3_ORDER
    Lookup3Row r;
    r.idx0 = v0, r.idx1 = v1, r.idx2 = v2;
    r.w1 = lookup_weight(w1), r.w2 = lookup_weight(w2);
    return r;
}

}  // namespace ohs
