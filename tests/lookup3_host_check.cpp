// lookup3_host_check.cpp -- csrc/lookup3_body.hpp compiled for the host: the inverses ohs_lookup3_create computes and the walk
// k_lookup_tri makes, one query at a time.  tests/test_cpu_lookup3.py builds this (-ffp-contract=off), feeds it meshes and queries
// through a file and compares the answers with tests/lookup3_model.py bit for bit.
//   in:  u32 n_cases, then per case  u32 M, u32 T, u32 n, f32 xyz[M][3], u32 tris[T][3], f64 q[n][3]
//   out: per case and query          u32 idx0, u32 idx1, u32 idx2, f32 w1, f32 w2, u32 tri
//   exit status 5: a singular triangle
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lookup3_body.hpp"

template <class T>
static bool get(FILE *f, T *p, size_t n)
{
    return fread(p, sizeof(T), n, f) == n;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t n_cases = 0;
    if (!get(in, &n_cases, 1)) return 3;
    for (uint32_t cs = 0; cs < n_cases; ++cs) {
        uint32_t M = 0, T = 0, n = 0;
        if (!get(in, &M, 1) || !get(in, &T, 1) || !get(in, &n, 1) || M == 0 || T == 0) return 3;
        std::vector<float> xyz(3 * (size_t)M);
        std::vector<uint32_t> tris(3 * (size_t)T);
        std::vector<double> q(3 * (size_t)n), inv(9 * (size_t)T);
        if (!get(in, xyz.data(), xyz.size()) || !get(in, tris.data(), tris.size()) || !get(in, q.data(), q.size())) return 3;
        for (uint32_t t = 0; t < T; ++t) {
            double p[3][3];
            for (int c = 0; c < 3; ++c) {
                if (tris[3 * t + c] >= M) return 3;
                for (int j = 0; j < 3; ++j) p[c][j] = (double)xyz[3 * (size_t)tris[3 * t + c] + j];
            }
            if (!ohs::lookup3_inverse(p[0], p[1], p[2], &inv[9 * (size_t)t])) return 5;
        }
        for (uint32_t i = 0; i < n; ++i) {
            const double q0 = ohs::lookup3_round(q[3 * i]), q1 = ohs::lookup3_round(q[3 * i + 1]), q2 = ohs::lookup3_round(q[3 * i + 2]);
            double best = -INFINITY;
            uint32_t tri = 0;
            for (uint32_t t = 0; t < T; ++t) ohs::lookup3_step(&inv[9 * (size_t)t], q0, q1, q2, t, best, tri);
            const ohs::Lookup3Row r = ohs::lookup3_winner(&inv[9 * (size_t)tri], &tris[3 * (size_t)tri], q0, q1, q2);
            if (fwrite(&r.idx0, 4, 1, out) != 1 || fwrite(&r.idx1, 4, 1, out) != 1 || fwrite(&r.idx2, 4, 1, out) != 1 ||
                fwrite(&r.w1, 4, 1, out) != 1 || fwrite(&r.w2, 4, 1, out) != 1 || fwrite(&tri, 4, 1, out) != 1)
                return 4;
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
