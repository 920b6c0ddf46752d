// sched_rows.h -- what the scheduled batch calls (api_batch.hip) have to know about a caller's schedule before anything is queued:
// the segment count, whether a row is constant, whether all rows are equal, and the one pass over rows of set indices.  Host code
// only, no HIP: tools/check_sched_rows.cpp builds it alone (tests/test_cpu_sched_rows.py).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstring>

namespace ohs_host {

// Segment k of a call = blocks [k seg_blocks, (k + 1) seg_blocks).  *seg_blocks > 0 is clamped to the call's length (a segment is
// never longer than the call); -> the number of segments.
inline size_t sched_segments(size_t n_blocks, size_t *seg_blocks)
{
    *seg_blocks = std::min(*seg_blocks, std::max<size_t>(n_blocks, 1));
    return (n_blocks + *seg_blocks - 1) / *seg_blocks;
}

// Rows of 32-bit entries, table indices or gains alike: gains compare as bits.
inline bool sched_row_constant(const void *row, size_t n)
{
    const unsigned *p = static_cast<const unsigned *>(row);
    for (size_t k = 1; k < n; ++k)
        if (p[k] != p[0]) return false;
    return true;
}

// `rows` rows of n entries, `stride` entries apart: are they all the first one?
inline bool sched_rows_equal(const void *base, size_t stride, size_t rows, size_t n)
{
    const unsigned *p = static_cast<const unsigned *>(base);
    for (size_t r = 1; r < rows; ++r)
        if (std::memcmp(p + r * stride, p, n * sizeof(unsigned)) != 0) return false;
    return true;
}

// One pass over `rows` rows of n_segs set indices, idx_stride apart (entries beyond n_segs in a padded row are never read), and over
// prev[rows] (optional): the set in front of each row's first segment.
struct SchedRowScan {
    bool ok = true;                 // every entry read is < limit; else which array held the offender(s)
    bool idx_bad = false, prev_bad = false;
    bool vary = false;              // some row changes along itself
    bool rows_differ = false;       // some row is not row 0
    bool prev_differ = false;       // some prev[r] is not prev[0]
    bool prev_boundary = false;     // some prev[r] != row r's first entry: that row's call begins on a change of set
    bool faded_end = false;         // the call's LAST block is the first block of a segment that changes the set, in some row
};

inline SchedRowScan sched_scan_rows(const unsigned *idx, size_t idx_stride, size_t rows, size_t n_segs, unsigned limit,
                                    const unsigned *prev, size_t n_blocks, size_t seg_blocks)
{
    SchedRowScan s;
    const bool last_is_first = n_blocks > 0 && (n_blocks - 1) % seg_blocks == 0;
    for (size_t r = 0; r < rows; ++r) {
        const unsigned *row = idx + r * idx_stride;
        for (size_t k = 0; k < n_segs; ++k) {
            s.idx_bad = s.idx_bad || row[k] >= limit;
            s.vary = s.vary || row[k] != row[0];
            s.rows_differ = s.rows_differ || row[k] != idx[k];
        }
        if (prev) {
            s.prev_bad = s.prev_bad || prev[r] >= limit;
            s.prev_differ = s.prev_differ || prev[r] != prev[0];
            s.prev_boundary = s.prev_boundary || (n_segs > 0 && prev[r] != row[0]);
        }
        if (last_is_first && n_segs > 1) s.faded_end = s.faded_end || row[n_segs - 1] != row[n_segs - 2];
        if (last_is_first && n_segs == 1 && prev) s.faded_end = s.faded_end || prev[r] != row[0];
    }
    s.ok = !s.idx_bad && !s.prev_bad;
    return s;
}

}  // namespace ohs_host
