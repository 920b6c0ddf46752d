// delay2_host_check.cpp -- csrc/delay2_body.hpp compiled for the host (tests/test_cpu_delay2.py): one call of the stage per case, the pass
// chosen per segment row with delay2_identity, frame by frame with delay_frame or delay2_frame, and for every tile the window
// delay_window or delay2_window promises, with every input read checked against it.
//
//   delay2_host_check in.bin out.bin
// in:  u64 n_cases; per case u64 S, K, N, H, seg_frames, n_segs, filtered; f64 max_delay; f64 front_d[S][K]; f64 row_d[S][n_segs][K];
//      f32 front_g[S][K]; f32 row_g[S][n_segs][K]; if filtered: f32 front_h[S][K][5]; f32 row_h[S][n_segs][K][5];
//      f32 ext[S][K][H + N] (the history, then the call)
// out: per case f32 y[S][K][N]; u64 tiles staged, tiles gathered, tiles filtered, inputs outside their tile's window
#include "delay2_body.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

constexpr unsigned TILE = 256, LDS_WINDOW = 2048;       // ohs::DELAY2_TILE, ohs::DELAY2_LDS_WINDOW
constexpr uint64_t TAPS = ohs::DELAY2_TAPS;

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
        const std::vector<uint64_t> h = get<uint64_t>(in, 7);
        const uint64_t S = h[0], K = h[1], N = h[2], H = h[3], seg_frames = h[4], n_segs = h[5], with_fir = h[6];
        const double max_delay = get<double>(in, 1)[0];
        const std::vector<double> front_d = get<double>(in, S * K), row_d = get<double>(in, S * n_segs * K);
        const std::vector<float> front_g = get<float>(in, S * K), row_g = get<float>(in, S * n_segs * K);
        const std::vector<float> front_h = get<float>(in, with_fir ? S * K * TAPS : 0), row_h = get<float>(in, with_fir ? S * n_segs * K * TAPS : 0);
        const std::vector<float> ext = get<float>(in, S * K * (H + N));
        std::vector<float> y(S * K * N);
        uint64_t counts[4] = {0, 0, 0, 0};
        for (uint64_t s = 0; s < S; ++s)
            for (uint64_t c = 0; c < K; ++c) {
                const float *x = ext.data() + (s * K + c) * (H + N) + H;          // x[m], -H <= m < N
                for (uint64_t n0 = 0; n0 < N; n0 += TILE) {
                    const uint64_t k = n0 / seg_frames, seg0 = k * seg_frames, L = N - seg0 < seg_frames ? N - seg0 : seg_frames;
                    const uint64_t row = (s * n_segs + k) * K + c;
                    const double D = row_d[row], Dp = k ? row_d[row - K] : front_d[s * K + c];
                    const float G = row_g[row], Gp = k ? row_g[row - K] : front_g[s * K + c];
                    const float *Hh = with_fir ? row_h.data() + row * TAPS : nullptr;
                    const float *Hp = !with_fir ? nullptr : k ? Hh - K * TAPS : front_h.data() + (s * K + c) * TAPS;
                    const bool filtered = with_fir && !(ohs::delay2_identity(Hh) && ohs::delay2_identity(Hp));
                    const ohs::DelayWindow w = filtered ? ohs::delay2_window(Dp, D, n0 - seg0, TILE, L, max_delay, (long long)n0)
                                                        : ohs::delay_window(Dp, D, n0 - seg0, TILE, L, max_delay, (long long)n0);
                    ++counts[w.width <= LDS_WINDOW ? 0 : 1];
                    counts[2] += filtered;
                    if (w.lo < -(long long)H || w.lo + (long long)w.width > (long long)N) ++counts[3];
                    auto tap = [&](long long m) {
                        if (m < w.lo || m >= w.lo + (long long)w.width) {
                            ++counts[3];
                            return 0.0f;            // (never x[m]: an input outside the window may lie outside ext)
                        }
                        return x[m];
                    };
                    for (uint64_t t = 0; t < TILE; ++t)
                        y[(s * K + c) * N + n0 + t] =
                            filtered ? ohs::delay2_frame(Dp, D, Gp, G, Hp, Hh, n0 - seg0 + t, L, max_delay, (long long)(n0 + t), tap)
                                     : ohs::delay_frame(Dp, D, Gp, G, n0 - seg0 + t, L, max_delay, (long long)(n0 + t), tap);
                }
            }
        fwrite(y.data(), sizeof(float), y.size(), out);
        fwrite(counts, sizeof(uint64_t), 4, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
