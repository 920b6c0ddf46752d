// scene_rows_host_check.cpp -- csrc/scene_rows_body.hpp compiled for the host: k_scene_rows_seal's three jobs done serially, row by row,
// with the kernel's own per-object and per-pair step.  tests/test_cpu_tracked.py builds it (once plain, once under the sanitizers, and
// against mutated copies of the header) and holds what it writes to tests/tracked_model.py.
//   in:  u32 n_cases; per case u32 {S, n_segs, K, seg_blocks, n_blocks, fade, has_carry}, rows [6][S][n_segs][K] u32, carry [6][S][K] u32 if has_carry
//   out: per case front [6][S][K] u32, carry [6][S][K] u32, u64 {fading, blended, blended3}
#include "scene_rows_body.hpp"

#include <cstdint>
#include <cstdio>
#include <vector>

using namespace ohs;

static bool read_words(FILE *f, std::vector<uint32_t> &v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), 4, n, f) == n;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t n_cases = 0;
    if (fread(&n_cases, 4, 1, in) != 1) return 3;
    for (uint32_t cs = 0; cs < n_cases; ++cs) {
        uint32_t h[7];
        if (fread(h, 4, 7, in) != 7) return 3;
        const size_t S = h[0], n_segs = h[1], K = h[2], seg_blocks = h[3], n_blocks = h[4];
        const bool fade = h[5] != 0, has_carry = h[6] != 0;
        const size_t plane = S * n_segs * K, front_plane = S * K;
        std::vector<uint32_t> rows, carry_in;
        if (!read_words(in, rows, 6 * plane) || !read_words(in, carry_in, has_carry ? 6 * front_plane : 0)) return 3;
        std::vector<uint32_t> front(6 * front_plane), carry(6 * front_plane);
        unsigned long long fading = 0, blended = 0, blended3 = 0;
        for (size_t row = 0; row < S * n_segs; ++row) {         // (one wave of the kernel)
            const size_t s = row / n_segs, k = row % n_segs;
            const uint32_t *cur = rows.data() + row * K;
            const bool carried = k == 0 && has_carry;
            const uint32_t *old = k > 0 ? cur - K : carried ? carry_in.data() + s * K : cur;
            const size_t old_plane = carried ? front_plane : plane;
            std::vector<unsigned> flags(K + 1, 0u);             // (the absent partner of an odd last object has none)
            for (size_t o = 0; o < K; ++o) {
                const SceneRowsEntry ce{cur[o], cur[plane + o], cur[2 * plane + o], cur[3 * plane + o], cur[4 * plane + o], cur[5 * plane + o]};
                const SceneRowsEntry oe{old[o], old[old_plane + o], old[2 * old_plane + o], old[3 * old_plane + o], old[4 * old_plane + o],
                                        old[5 * old_plane + o]};
                flags[o] = scene_rows_object(ce, oe, fade);
                for (size_t pl = 0; pl < 6; ++pl) {
                    if (k == 0) front[pl * front_plane + s * K + o] = old[pl * old_plane + o];
                    if (k == scene_rows_carry_segment(n_segs)) carry[pl * front_plane + s * K + o] = cur[pl * plane + o];
                }
            }
            const unsigned long long seg_len = scene_rows_seg_len(k, seg_blocks, n_blocks);
            for (size_t p = 0; 2 * p < K; ++p) {
                const SceneRowsPair pr = scene_rows_pair(flags[2 * p] | flags[2 * p + 1]);
                fading += pr.fading;
                blended += pr.cur4 * seg_len + pr.old4;
                blended3 += pr.cur6 * seg_len + pr.old6;
            }
        }
        const unsigned long long counts[3] = {fading, blended, blended3};
        if (fwrite(front.data(), 4, front.size(), out) != front.size() || fwrite(carry.data(), 4, carry.size(), out) != carry.size() ||
            fwrite(counts, 8, 3, out) != 3)
            return 4;
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
