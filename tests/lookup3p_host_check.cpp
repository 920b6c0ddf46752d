// lookup3p_host_check.cpp -- csrc/lookup3p_body.hpp (and lookup3_body.hpp under it) compiled for the host: the index
// ohs_lookup3p_create builds, and per query what the two kernels do -- pass 1 over the merged lists, the certificate, and for the
// queries it does not cover the walk over every triangle.  tests/test_cpu_lookup3p.py builds this (-ffp-contract=off; once more under
// the address and undefined-behaviour sanitizers), feeds it meshes and queries through a file and holds the answers to
// tests/lookup3p_model.py.
//   in:  u32 n_cases, then per case  u32 M, u32 T, u32 n, u32 grid (0: the library's choice), f32 xyz[M][3], u32 tris[T][3], f64 q[n][3]
//   out: per case  u32 G, u32 cells, u32 n_everywhere, u32 everywhere[..], u32 cell_start[cells + 1], u32 cell_tris[..],
//        then per query  u32 idx0, u32 idx1, u32 idx2, f32 w1, f32 w2, u32 tri, u32 fell_back, u32 cell
//   exit status 5: a singular triangle
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lookup3p_body.hpp"

template <class T>
static bool get(FILE *f, T *p, size_t n)
{
    return fread(p, sizeof(T), n, f) == n;
}

static bool put(FILE *f, const uint32_t *p, size_t n)
{
    return n == 0 || fwrite(p, 4, n, f) == n;      // (an empty list has no address to hand over)
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const unsigned IS = ohs::LOOKUP3P_INV_STRIDE;
    uint32_t n_cases = 0;
    if (!get(in, &n_cases, 1)) return 3;
    for (uint32_t cs = 0; cs < n_cases; ++cs) {
        uint32_t M = 0, T = 0, n = 0, grid = 0;
        if (!get(in, &M, 1) || !get(in, &T, 1) || !get(in, &n, 1) || !get(in, &grid, 1) || M == 0 || T == 0 || grid > ohs::LOOKUP3P_MAX_GRID) return 3;
        std::vector<float> xyz(3 * (size_t)M);
        std::vector<uint32_t> tris(3 * (size_t)T);
        std::vector<double> q(3 * (size_t)n), inv(IS * (size_t)T, 0.0);
        if (!get(in, xyz.data(), xyz.size()) || !get(in, tris.data(), tris.size()) || !get(in, q.data(), q.size())) return 3;
        for (uint32_t t = 0; t < T; ++t) {
            double p[3][3];
            for (int c = 0; c < 3; ++c) {
                if (tris[3 * t + c] >= M) return 3;
                for (int j = 0; j < 3; ++j) p[c][j] = (double)xyz[3 * (size_t)tris[3 * t + c] + j];
            }
            if (!ohs::lookup3_inverse(p[0], p[1], p[2], &inv[IS * (size_t)t])) return 5;
        }
        ohs::Lookup3pIndex ix;
        ohs::lookup3p_build_index(xyz.data(), tris.data(), T, grid ? grid : ohs::lookup3p_choose_grid(T), ix);
        const double B = ohs::lookup3p_bound(inv.data(), T, IS);
        const uint32_t head[3] = {ix.G, (uint32_t)(ix.cell_start.size() - 1), (uint32_t)ix.everywhere.size()};
        if (!put(out, head, 3) || !put(out, ix.everywhere.data(), ix.everywhere.size()) || !put(out, ix.cell_start.data(), ix.cell_start.size()) ||
            !put(out, ix.cell_tris.data(), ix.cell_tris.size()))
            return 4;
        for (uint32_t i = 0; i < n; ++i) {
            const double q0 = ohs::lookup3_round(q[3 * i]), q1 = ohs::lookup3_round(q[3 * i + 1]), q2 = ohs::lookup3_round(q[3 * i + 2]);
            const uint32_t cell = ohs::lookup3p_cell(q0, q1, q2, ix.G);
            if (cell >= head[1]) return 6;
            const uint32_t lo = ix.cell_start[cell], hi = ix.cell_start[cell + 1];
            double best = -INFINITY;
            uint32_t tri = 0;
            ohs::lookup3p_walk(inv.data(), ix.everywhere.data(), (uint32_t)ix.everywhere.size(), ix.cell_tris.data() + lo, hi - lo, q0, q1, q2, best, tri);
            const uint32_t rest = !(best > ohs::lookup3p_tau(B, q0, q1, q2));
            if (rest) {
                best = -INFINITY, tri = 0;
                for (uint32_t t = 0; t < T; ++t) ohs::lookup3_step(&inv[IS * (size_t)t], q0, q1, q2, t, best, tri);
            }
            const ohs::Lookup3Row r = ohs::lookup3_winner(&inv[IS * (size_t)tri], &tris[3 * (size_t)tri], q0, q1, q2);
            if (fwrite(&r.idx0, 4, 1, out) != 1 || fwrite(&r.idx1, 4, 1, out) != 1 || fwrite(&r.idx2, 4, 1, out) != 1 ||
                fwrite(&r.w1, 4, 1, out) != 1 || fwrite(&r.w2, 4, 1, out) != 1 || fwrite(&tri, 4, 1, out) != 1 || !put(out, &rest, 1) ||
                !put(out, &cell, 1))
                return 4;
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
