// delay_host_check.cpp -- csrc/delay_body.hpp compiled for the host (tests/test_cpu_delay.py): one call of the stage per case, frame by
// frame with delay_frame, and for every tile the window delay_window promises, with every tap checked against it.
//
//   delay_host_check in.bin out.bin
// in:  u64 n_cases; per case u64 S, K, N, H, seg_frames, n_segs; f64 max_delay; f64 front_d[S][K]; f64 row_d[S][n_segs][K];
//      f32 front_g[S][K]; f32 row_g[S][n_segs][K]; f32 ext[S][K][H + N] (the history, then the call)
// out: per case f32 y[S][K][N]; u64 tiles staged, tiles gathered, taps outside their tile's window
#include "delay_body.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

constexpr unsigned TILE = 256, LDS_WINDOW = 2048;       // ohs::DELAY_TILE, ohs::DELAY_LDS_WINDOW

template <class T>
std::vector<T> get(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "short read\n");
        exit(2);
    }
    return v;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const uint64_t n_cases = get<uint64_t>(in, 1)[0];
    for (uint64_t cs = 0; cs < n_cases; ++cs) {
        const std::vector<uint64_t> h = get<uint64_t>(in, 6);
        const uint64_t S = h[0], K = h[1], N = h[2], H = h[3], seg_frames = h[4], n_segs = h[5];
        const double max_delay = get<double>(in, 1)[0];
        const std::vector<double> front_d = get<double>(in, S * K), row_d = get<double>(in, S * n_segs * K);
        const std::vector<float> front_g = get<float>(in, S * K), row_g = get<float>(in, S * n_segs * K);
        const std::vector<float> ext = get<float>(in, S * K * (H + N));
        std::vector<float> y(S * K * N);
        uint64_t counts[3] = {0, 0, 0};
        for (uint64_t s = 0; s < S; ++s)
            for (uint64_t c = 0; c < K; ++c) {
                const float *x = ext.data() + (s * K + c) * (H + N) + H;          // x[m], m >= -H
                for (uint64_t n0 = 0; n0 < N; n0 += TILE) {
                    const uint64_t k = n0 / seg_frames, seg0 = k * seg_frames, L = N - seg0 < seg_frames ? N - seg0 : seg_frames;
                    const uint64_t row = (s * n_segs + k) * K + c;
                    const double D = row_d[row], Dp = k ? row_d[row - K] : front_d[s * K + c];
                    const float G = row_g[row], Gp = k ? row_g[row - K] : front_g[s * K + c];
                    const ohs::DelayWindow w = ohs::delay_window(Dp, D, n0 - seg0, TILE, L, max_delay, (long long)n0);
                    ++counts[w.width <= LDS_WINDOW ? 0 : 1];
                    if (w.lo < -(long long)H || w.lo + (long long)w.width > (long long)N) ++counts[2];
                    for (uint64_t t = 0; t < TILE; ++t)
                        y[(s * K + c) * N + n0 + t] = ohs::delay_frame(Dp, D, Gp, G, n0 - seg0 + t, L, max_delay, (long long)(n0 + t), [&](long long m) {
                            if (m < w.lo || m >= w.lo + (long long)w.width) ++counts[2];
                            return x[m];
                        });
                }
            }
        fwrite(y.data(), sizeof(float), y.size(), out);
        fwrite(counts, sizeof(uint64_t), 3, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
