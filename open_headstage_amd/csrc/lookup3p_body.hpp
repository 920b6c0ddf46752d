// lookup3p_body.hpp -- what the pruned three-direction lookup adds to lookup3_body.hpp (include/ohs_lookup3p.h, HOW EXACTNESS IS KEPT;
// DESIGN.md section 4.5m), once for the device and the host: the cube-map cell of a query, the certificate's threshold, the walk over
// two ascending lists merged, and -- host only -- the index over the sphere that ohs_lookup3p_create builds.  k_lookup_tri_cells
// (lookup3p_kernels.hip) inlines the first three, api_lookup3p.hip calls the builder, and tests/test_cpu_lookup3p.py compiles this
// header into a stand-alone program (tests/lookup3p_host_check.cpp) and holds it to tests/lookup3p_model.py.  Everything is f64 and
// every operation rounds by itself: the units that include this are compiled with -ffp-contract=off, and nothing here calls fma.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "lookup3_body.hpp"     // (lookup3_step, OHS_LK_HD)

namespace ohs {

constexpr unsigned LOOKUP3P_INV_STRIDE = 10;        // doubles per triangle's inverse as stored: nine and one of padding, 80 B, 16-byte rows
constexpr unsigned LOOKUP3P_MAX_GRID = 256;
constexpr uint32_t LOOKUP3P_END = 0xffffffffu;      // behind the last entry of a list (no triangle has this index)
// the padding of a triangle's cap, in radians: far above every rounding between here and the kernel (the cap's own arithmetic, the
// cells' bounding caps, the kernel's cell assignment: all below 1e-12), far below any triangle worth pruning
constexpr double LOOKUP3P_PAD = 1e-6;
// a cap is "safely below 90 degrees" when the cosine of its radius is above this (88.85 degrees)
constexpr double LOOKUP3P_MIN_COS = 0.02;
// a triangle whose padded cap can touch more cells than this goes on the everywhere list instead: the lists stay below
// LOOKUP3P_MAX_CELLS_PER_TRIANGLE * n_tris entries whatever the mesh and the grid
constexpr unsigned LOOKUP3P_MAX_CELLS_PER_TRIANGLE = 64;

// grid == 0: the library's choice, about one cell per triangle -- G = ceil(sqrt(n_tris / 6)), at least 1, at most 256
inline unsigned lookup3p_choose_grid(size_t n_tris)
{
    unsigned G = 1;
    while (G < LOOKUP3P_MAX_GRID && 6 * (size_t)G * G < n_tris) ++G;
    return G;
}

// The cell of a query (the point as the walk sees it: lookup3_round's values) on the cube map of 6 G^2 cells.  The face is the
// coordinate of largest magnitude (x before y before z among equals) and its sign: face = 2 axis + (q[axis] < 0).  On it, with M =
// |q[axis]|, u = q[(axis + 1) % 3] / M and v = q[(axis + 2) % 3] / M lie in [-1, 1], and the cell is (floor((u + 1) (G / 2)), floor((v +
// 1) (G / 2))), each clamped to 0 .. G - 1: cell = (face G + iu) G + iv.  The origin has no direction: cell 0 (it is never certified).
OHS_LK_HD inline uint32_t lookup3p_cell(double q0, double q1, double q2, unsigned G)
{
    const double a0 = fabs(q0), a1 = fabs(q1), a2 = fabs(q2);
    const int axis = (a0 >= a1 && a0 >= a2) ? 0 : (a1 >= a2 ? 1 : 2);
    const double M = axis == 0 ? a0 : (axis == 1 ? a1 : a2);
    if (!(M > 0.0)) return 0;
    const double major = axis == 0 ? q0 : (axis == 1 ? q1 : q2);
    const double a = axis == 0 ? q1 : (axis == 1 ? q2 : q0);
    const double b = axis == 0 ? q2 : (axis == 1 ? q0 : q1);
    const double half = 0.5 * (double)G;
    const double fu = floor((a / M + 1.0) * half), fv = floor((b / M + 1.0) * half);
    const double top = (double)(G - 1);
    const unsigned iu = (unsigned)(fu < 0.0 ? 0.0 : (fu > top ? top : fu)), iv = (unsigned)(fv < 0.0 ? 0.0 : (fv > top ? top : fv));
    const unsigned face = 2u * (unsigned)axis + (major < 0.0 ? 1u : 0u);
    return (face * G + iu) * G + iv;
}

// B of the certificate: the largest (|inv[t][i][0]| + |inv[t][i][1]|) + |inv[t][i][2]| over every triangle and row
inline double lookup3p_bound(const double *inv, size_t n_tris, unsigned stride)
{
    double B = 0.0;
    for (size_t t = 0; t < n_tris; ++t)
        for (int i = 0; i < 3; ++i) {
            const double *r = inv + stride * t + 3 * i;
            const double s = (fabs(r[0]) + fabs(r[1])) + fabs(r[2]);
            B = s > B ? s : B;
        }
    return B;
}

// tau of the certificate: pass 1's answer stands iff its best min(g) > tau
OHS_LK_HD inline double lookup3p_tau(double B, double q0, double q1, double q2)
{
    return (0x1p-40 * B) * ((fabs(q0) + fabs(q1)) + fabs(q2));
}

// pass 1's walk: the everywhere list and the cell's list, both ascending, merged -- lookup3_step in ascending t overall, so that the
// first of equals is kept exactly as the walk over every triangle keeps it.  inv: rows of LOOKUP3P_INV_STRIDE doubles.
OHS_LK_HD inline void lookup3p_walk(const double *inv, const uint32_t *every, uint32_t n_every, const uint32_t *list, uint32_t n_list, double q0,
                                    double q1, double q2, double &best, uint32_t &best_t)
{
    uint32_t i = 0, j = 0;
    uint32_t te = n_every ? every[0] : LOOKUP3P_END, tl = n_list ? list[0] : LOOKUP3P_END;
    while ((te & tl) != LOOKUP3P_END) {         // (until both lists are behind their last entry)
        const bool e = te < tl;
        const uint32_t t = e ? te : tl;
        lookup3_step(inv + LOOKUP3P_INV_STRIDE * (size_t)t, q0, q1, q2, t, best, best_t);
        if (e) {
            ++i;
            te = i < n_every ? every[i] : LOOKUP3P_END;
        } else {
            ++j;
            tl = j < n_list ? list[j] : LOOKUP3P_END;
        }
    }
}

// ---- the index (host only) ------------------------------------------------------------------------------------------------------------
struct Lookup3pIndex {
    unsigned G = 0;
    std::vector<uint32_t> cell_start;       // [6 G^2 + 1]
    std::vector<uint32_t> cell_tris;        // [cell_start.back()], ascending within a cell
    std::vector<uint32_t> everywhere;       // ascending
    size_t longest = 0;
};

// The lists of every cell and the everywhere list for the mesh tris[T][3] over the table xyz[..][3] (f32, every triangle non-singular),
// on a grid of G >= 1.
//
// A triangle's reach is the cap around n = the normalised sum of its unit corners, out to the farthest corner and LOOKUP3P_PAD beyond.
// Below 90 degrees a cap is convex on the sphere, so it holds the whole spherical triangle, and the cone of positive combinations of
// the corners is the cone over that: a query strictly inside the cone points into the cap.  A triangle whose axis degenerates (|sum| <=
// 1e-3) or whose cap is not safely below 90 degrees makes no such promise and goes on the everywhere list.
//
// Cells are tested in the face's own frame (|n[axis]| forward, the two other coordinates as the kernel's u and v take them; a
// reflection of the sphere, so caps stay caps).  A cap can touch column iu of a face only if it is not wholly on the far side of
// either of the two planes through the origin that bound the column (u = u_k: the plane with normal (-u_k, 1, 0) / h_k) -- necessary,
// not sufficient, the same for rows; in the columns and rows that remain, a cell is listed when the triangle's cap touches the cell's
// bounding cap (around the direction of the cell's middle, out to its farthest corner -- the farthest point of a convex spherical
// polygon from a point inside it is a corner).  Every test errs towards listing.
inline void lookup3p_build_index(const float *xyz, const uint32_t *tris, size_t T, unsigned G, Lookup3pIndex &ix)
{
    const size_t cells = 6 * (size_t)G * G;
    ix.G = G;
    ix.everywhere.clear();
    // the planes' normals (-u_k, 1) / h_k for k = 0 .. G, and per cell of a face the bounding cap: its axis, cos and sin of its radius
    std::vector<double> line_u(G + 1), line_h(G + 1);
    for (unsigned k = 0; k <= G; ++k) {
        line_u[k] = 2.0 * (double)k / (double)G - 1.0;
        line_h[k] = sqrt(1.0 + line_u[k] * line_u[k]);
    }
    std::vector<double> cap(5 * (size_t)G * G);
    for (unsigned iu = 0; iu < G; ++iu)
        for (unsigned iv = 0; iv < G; ++iv) {
            const double um = 0.5 * (line_u[iu] + line_u[iu + 1]), vm = 0.5 * (line_u[iv] + line_u[iv + 1]);
            const double hm = sqrt((1.0 + um * um) + vm * vm);
            const double c[3] = {1.0 / hm, um / hm, vm / hm};
            double lo = 1.0;
            for (int corner = 0; corner < 4; ++corner) {
                const double u = line_u[iu + (corner & 1)], v = line_u[iv + (corner >> 1)];
                const double d = ((c[0] + c[1] * u) + c[2] * v) / sqrt((1.0 + u * u) + v * v);
                lo = d < lo ? d : lo;
            }
            double *o = &cap[5 * ((size_t)iu * G + iv)];
            o[0] = c[0], o[1] = c[1], o[2] = c[2], o[3] = lo, o[4] = sqrt(1.0 - lo * lo > 0.0 ? 1.0 - lo * lo : 0.0);
        }
    const double face_cos = 1.0 / sqrt(3.0), face_sin = sqrt(2.0 / 3.0);       // a face's bounding cap: out to (1, 1, 1) / sqrt 3
    std::vector<uint64_t> pairs;                // (cell << 32) | t, t ascending
    std::vector<uint32_t> mine;                 // one triangle's cells
    std::vector<unsigned char> col(G), row(G);
    for (size_t t = 0; t < T; ++t) {
        double un[3][3], s[3] = {0.0, 0.0, 0.0};
        for (int c = 0; c < 3; ++c) {
            const float *p = xyz + 3 * (size_t)tris[3 * t + c];
            const double x = p[0], y = p[1], z = p[2], len = sqrt((x * x + y * y) + z * z);
            un[c][0] = x / len, un[c][1] = y / len, un[c][2] = z / len;
            for (int j = 0; j < 3; ++j) s[j] += un[c][j];
        }
        const double ns = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
        bool everywhere = !(ns > 1e-3);
        double n[3] = {0.0, 0.0, 0.0}, c_rho = 0.0, s_rho = 0.0;
        if (!everywhere) {
            double lo = 1.0;
            for (int j = 0; j < 3; ++j) n[j] = s[j] / ns;
            for (int c = 0; c < 3; ++c) {
                const double d = (n[0] * un[c][0] + n[1] * un[c][1]) + n[2] * un[c][2];
                lo = d < lo ? d : lo;
            }
            everywhere = !(lo > LOOKUP3P_MIN_COS);
            const double rho = acos(lo) + LOOKUP3P_PAD;         // (lo <= 1; below 1.551 + 1e-6)
            c_rho = cos(rho), s_rho = sin(rho);
        }
        mine.clear();
        for (unsigned face = 0; face < 6 && !everywhere; ++face) {
            const unsigned axis = face >> 1;
            const double L[3] = {(face & 1) ? -n[axis] : n[axis], n[(axis + 1) % 3], n[(axis + 2) % 3]};
            // cos(rho + r) = cos rho cos r - sin rho sin r for both radii in [0, 90 degrees): the caps touch iff the axes' cosine is
            // at least that
            if (!(L[0] >= c_rho * face_cos - s_rho * face_sin)) continue;
            for (unsigned k = 0; k < G; ++k) {
                const double u_lo = (L[1] - line_u[k] * L[0]) / line_h[k], u_hi = (L[1] - line_u[k + 1] * L[0]) / line_h[k + 1];
                const double v_lo = (L[2] - line_u[k] * L[0]) / line_h[k], v_hi = (L[2] - line_u[k + 1] * L[0]) / line_h[k + 1];
                col[k] = u_lo >= -s_rho && u_hi <= s_rho;
                row[k] = v_lo >= -s_rho && v_hi <= s_rho;
            }
            for (unsigned iu = 0; iu < G && mine.size() <= LOOKUP3P_MAX_CELLS_PER_TRIANGLE; ++iu) {
                if (!col[iu]) continue;
                for (unsigned iv = 0; iv < G; ++iv) {
                    if (!row[iv]) continue;
                    const double *o = &cap[5 * ((size_t)iu * G + iv)];
                    const double d = (L[0] * o[0] + L[1] * o[1]) + L[2] * o[2];
                    if (d >= c_rho * o[3] - s_rho * o[4]) mine.push_back((uint32_t)((face * G + iu) * G + iv));
                }
            }
            if (mine.size() > LOOKUP3P_MAX_CELLS_PER_TRIANGLE) everywhere = true;
        }
        if (everywhere) {
            ix.everywhere.push_back((uint32_t)t);
            continue;
        }
        // (a cap below 90 degrees that touches no cell cannot be: its own axis lies in some cell.  Were it to happen the triangle
        // would be on no list; the everywhere list is the safe place for it.)
        if (mine.empty()) {
            ix.everywhere.push_back((uint32_t)t);
            continue;
        }
        for (uint32_t cell : mine) pairs.push_back(((uint64_t)cell << 32) | (uint32_t)t);
    }
    // counting sort by cell; t stays ascending within a cell
    ix.cell_start.assign(cells + 1, 0);
    for (uint64_t p : pairs) ++ix.cell_start[(size_t)(p >> 32) + 1];
    ix.longest = 0;
    for (size_t c = 0; c < cells; ++c) {
        ix.longest = ix.cell_start[c + 1] > ix.longest ? ix.cell_start[c + 1] : ix.longest;
        ix.cell_start[c + 1] += ix.cell_start[c];
    }
    ix.cell_tris.resize(pairs.size());
    std::vector<uint32_t> at(ix.cell_start.begin(), ix.cell_start.end() - 1);
    for (uint64_t p : pairs) ix.cell_tris[at[(size_t)(p >> 32)]++] = (uint32_t)p;
}

}  // namespace ohs
