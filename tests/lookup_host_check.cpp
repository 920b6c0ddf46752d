// lookup_host_check.cpp -- csrc/lookup_body.hpp compiled for the host: the walk k_lookup makes, one query at a time.
// tests/test_cpu_lookup.py builds this (-ffp-contract=off), feeds it tables and queries through a file and compares the answers with
// tests/lookup_model.py bit for bit.
//   in:  u32 n_cases, then per case  u32 M, u32 n, f32 xyz[M][3], f64 q[n][3]
//   out: per case and query          u32 idx0, u32 idx1, f32 w
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lookup_body.hpp"

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
        uint32_t M = 0, n = 0;
        if (!get(in, &M, 1) || !get(in, &n, 1) || M == 0) return 3;
        std::vector<float> xyz(3 * (size_t)M);
        std::vector<double> q(3 * (size_t)n), P(3 * (size_t)M);
        if (!get(in, xyz.data(), xyz.size()) || !get(in, q.data(), q.size())) return 3;
        for (size_t i = 0; i < P.size(); ++i) P[i] = (double)xyz[i];
        for (uint32_t i = 0; i < n; ++i) {
            const double q0 = q[3 * i], q1 = q[3 * i + 1], q2 = q[3 * i + 2];
            double best_d = INFINITY;
            uint32_t idx0 = 0;
            for (uint32_t m = 0; m < M; ++m) ohs::lookup_nearest_step(P[3 * m], P[3 * m + 1], P[3 * m + 2], q0, q1, q2, m, best_d, idx0);
            const double qr0 = (double)(float)q0, qr1 = (double)(float)q1, qr2 = (double)(float)q2;
            double best_o = INFINITY, best_t = 0.0;
            uint32_t idx1 = idx0;
            for (uint32_t m = 0; m < M; ++m)
                ohs::lookup_bracket_step(P[3 * m], P[3 * m + 1], P[3 * m + 2], P[3 * idx0], P[3 * idx0 + 1], P[3 * idx0 + 2], qr0, qr1, qr2, m,
                                         best_o, idx1, best_t);
            const float w = ohs::lookup_weight(best_t);
            if (fwrite(&idx0, 4, 1, out) != 1 || fwrite(&idx1, 4, 1, out) != 1 || fwrite(&w, 4, 1, out) != 1) return 4;
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
