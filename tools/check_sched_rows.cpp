// check_sched_rows.cpp -- csrc/sched_rows.h alone, for tests/test_cpu_sched_rows.py (built with -fsanitize=address,undefined).
// stdin: native 32-bit words, one record per case; stdout: one line of 0 / 1 digits (or numbers) per case.
//   0 rows n_segs stride limit has_prev n_blocks seg_blocks idx[rows * stride] prev[has_prev ? rows : 0]
//        -> ok idx_bad prev_bad vary rows_differ prev_differ prev_boundary faded_end, as eight digits
//   1 n_blocks seg_blocks                  -> "<clamped seg_blocks> <n_segs>"
//   2 rows n stride entries[rows * stride] -> row 0 constant, all rows equal, as two digits
// Every array lives in a heap block of exactly its size, so that a read outside it is the sanitizer's to report.
#include <cstdio>
#include <memory>

#include "sched_rows.h"

static bool read_words(unsigned *p, size_t n)
{
    return std::fread(p, sizeof(unsigned), n, stdin) == n;
}

static std::unique_ptr<unsigned[]> read_array(size_t n, bool *ok)
{
    std::unique_ptr<unsigned[]> p(new unsigned[n]);
    *ok = *ok && read_words(p.get(), n);
    return p;
}

int main()
{
    unsigned kind;
    bool ok = true;
    while (ok && read_words(&kind, 1)) {
        if (kind == 0) {
            unsigned h[7];      // rows n_segs stride limit has_prev n_blocks seg_blocks
            if (!read_words(h, 7)) return 2;
            const size_t rows = h[0], n_segs = h[1], stride = h[2];
            const auto idx = read_array(rows * stride, &ok);
            const auto prev = read_array(h[4] ? rows : 0, &ok);
            if (!ok) return 2;
            const ohs_host::SchedRowScan s =
                ohs_host::sched_scan_rows(idx.get(), stride, rows, n_segs, h[3], h[4] ? prev.get() : nullptr, h[5], h[6]);
            std::printf("%d%d%d%d%d%d%d%d\n", s.ok, s.idx_bad, s.prev_bad, s.vary, s.rows_differ, s.prev_differ, s.prev_boundary,
                        s.faded_end);
        } else if (kind == 1) {
            unsigned h[2];
            if (!read_words(h, 2)) return 2;
            size_t seg_blocks = h[1];
            const size_t n_segs = ohs_host::sched_segments(h[0], &seg_blocks);
            std::printf("%zu %zu\n", seg_blocks, n_segs);
        } else if (kind == 2) {
            unsigned h[3];      // rows n stride
            if (!read_words(h, 3)) return 2;
            const auto e = read_array((size_t)h[0] * h[2], &ok);
            if (!ok) return 2;
            std::printf("%d%d\n", ohs_host::sched_row_constant(e.get(), h[1]), ohs_host::sched_rows_equal(e.get(), h[2], h[0], h[1]));
        } else {
            std::fprintf(stderr, "unknown record kind %u\n", kind);
            return 2;
        }
    }
    return 0;
}
