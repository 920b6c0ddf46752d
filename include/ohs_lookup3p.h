/* ohs_lookup3p.h -- C ABI of libohs_lookup3p.so: the rows of libohs_lookup3.so (include/ohs_lookup3.h) -- three direction indices and
 * two weights per object, stream and segment over a triangle mesh of the measurements -- with the walk over the triangles PRUNED by a
 * grid over the sphere, and not one bit of any answer changed (k_lookup_tri_cells, k_lookup_tri_rest; DESIGN.md section 4.5m,
 * SCENES.md).
 *
 * A library of its own: it links none of the product's code and none of the other lookup libraries', exports the ohs_lookup3p_*
 * names below and nothing else, and its handle mixes with no other library's.  For every table, mesh and query that
 * ohs_lookup3_create / _points / _rows accept, idx0, idx1, idx2, w1, w2 and tri are what those calls return, bit for bit and index for
 * index: THE ARITHMETIC of ohs_lookup3.h, which tests/lookup3_model.py restates.  No answer depends on the grid.
 *
 * Conventions (ohs_lookup3.h's): every function returns a status (0 = ok; the values are ohs_hip.h's OHS_* codes, restated below),
 * ohs_lookup3p_last_error() is the thread-local detail of the last failure in THIS library.  EVERY pointer is a HOST pointer.  EVERY
 * call is SYNCHRONOUS: the answers are in the caller's arrays on return.  The handle works on a non-blocking stream of its own.  A
 * refused call writes nothing and leaves the handle as it was; the caller's current device is put back.  A handle is used from one
 * thread at a time.
 *
 * HOW EXACTNESS IS KEPT.  Everything below is f64, every operation is rounded by itself (no fused multiply-add), sums are taken in the
 * order written.  inv[t], g_i(t), m(t) = min(min(g_0, g_1), g_2) and q are ohs_lookup3.h's; "the full walk" is its walk over t = 0, 1,
 * .., and its answer tri is the smallest t at which m is maximal.
 *
 *   1. THE INDEX, built on the host at create, sent to the device once.  A cube map of 6 G^2 cells over directions: the face of a
 *      query is its coordinate of largest magnitude (x before y before z among equals) and that coordinate's sign, face = 2 axis +
 *      (q[axis] < 0); with M = |q[axis]|, u = q[(axis + 1) % 3] / M, v = q[(axis + 2) % 3] / M, the cell is (floor((u + 1) (G / 2)),
 *      floor((v + 1) (G / 2))), each clamped to 0 .. G - 1.  (The origin has no direction and is given cell 0.)  Each cell holds an
 *      ascending list of triangles in CSR form (cell_start, cell_tris).
 *        A triangle's REACH is the spherical cap around n = (a^ + b^ + c^) / |a^ + b^ + c^| (x^ = x / |x|, its unit corners) out to
 *      the farthest corner, rho = acos(min n . x^), plus a padding of 1e-6 rad.  A cap below 90 degrees is convex on the sphere, so it
 *      holds the spherical triangle a^ b^ c^ whole, and the cone of positive combinations of a, b, c is the cone over that triangle:
 *      a query strictly inside the cone points into the cap.  A triangle is put on the list of every cell that its padded cap can
 *      touch.  The cell test is coarse and errs towards listing: a cap can touch a column (row) of a face only if it is not wholly
 *      beyond either plane through the origin that bounds it, and within the columns and rows that remain a cell is listed when the
 *      cap touches the cell's bounding cap (around the direction of the cell's middle out to its farthest corner).
 *        A triangle whose cap is not safely below 90 degrees (min n . x^ <= 0.02), whose axis degenerates (|a^ + b^ + c^| <= 1e-3), or
 *      whose cap touches more than 64 cells goes on the EVERYWHERE list, which every query walks.  (The last rule only bounds the
 *      lists' size -- at most 64 entries per triangle; the everywhere list is always a safe place.)
 *        The padding is there for rounding: the cap's and the cells' own arithmetic, and the kernel's cell assignment, which can
 *      put a query within 1e-13 rad of a cell's border into the neighbour.  All of it is below 1e-12 rad; 1e-6 covers it a million
 *      times and still widens no list that matters.
 *   2. PASS 1 (k_lookup_tri_cells), one query per lane.  The query is formed exactly as libohs_lookup3.so forms it (pose, then the
 *      rounding to f32).  The lane computes its cell and evaluates m(t) for the t of the everywhere list and of the cell's list,
 *      MERGED IN ASCENDING t, keeping the running maximum under strict >: the smallest listed t at which m is maximal among the listed.
 *   3. THE CERTIFICATE.  Once per handle  B = max over t, i of (|inv[t][i][0]| + |inv[t][i][1]|) + |inv[t][i][2]|;  per query
 *          tau = (2^-40 B) ((|q0| + |q1|) + |q2|).
 *      Pass 1's answer STANDS iff its best m > tau.  Why it is then the full walk's answer:
 *        (a) a computed g_i(t) differs from the exact sum inv[t][i] . q by the rounding of three products and two sums, at most
 *            2^-51 B |q|_1 -- 2 048 times smaller than tau.  So m(t) > tau means every exact gain at t is positive: q lies strictly
 *            inside t's cone, hence in t's cap, hence t is on the everywhere list or on the list of q's cell.
 *        (b) conversely a triangle on neither list does not hold q strictly inside: some exact gain is <= 0, its computed m is at
 *            most 2^-51 B |q|_1 < tau.
 *        (c) let t* be the full walk's answer and m* its m.  m* >= pass 1's best > tau, so by (a) t* is listed and pass 1 met it:
 *            pass 1's best is m*.  Every t with m(t) = m* is listed for the same reason, both walks take the smallest of them:
 *            the same tri.  The row is computed from tri and q alone, by the same operations: the same bits.
 *      And since t* is always listed when m* > tau, a query is certified IFF THE FULL WALK'S BEST m EXCEEDS tau -- a property of the
 *      mesh and the query alone, whatever G is.  tests/lookup3p_model.py predicts the set from that.
 *   4. PASS 2 (k_lookup_tri_rest).  The queries pass 1 does not certify -- the origin, a query on a corner or an edge of the mesh
 *      (its best exact gain is 0), a query outside an open mesh -- are appended by pass 1 to a compact list (one atomic add per wave)
 *      and answered by the full walk over every triangle, as libohs_lookup3.so does it; pass 2 is launched behind pass 1 without a
 *      host round trip, sized for the chunk, and workgroups beyond the list's length leave at once.  A certified query's row is written
 *      once, by pass 1; another's once, by pass 2.
 * A call in which EVERY source stands exactly on a measurement therefore costs what libohs_lookup3.so's costs, plus pass 1.
 *
 * Out of scope (none of it is built): a walk over the mesh's adjacency; rows handed to the scene calls on the device; an index kept
 * across handles. */
#ifndef OHS_LOOKUP3P_H
#define OHS_LOOKUP3P_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OHS_LOOKUP3P_OK              0
#define OHS_LOOKUP3P_ERR_INVALID_ARG 1
#define OHS_LOOKUP3P_ERR_NO_DEVICE   2
#define OHS_LOOKUP3P_ERR_HIP         3
#define OHS_LOOKUP3P_ERR_ALLOC       6

#define OHS_LOOKUP3P_MAX_OBJECTS     64
#define OHS_LOOKUP3P_MAX_DIRECTIONS  65536
#define OHS_LOOKUP3P_MAX_TRIANGLES   131072
#define OHS_LOOKUP3P_MAX_MAGNITUDE   1e15   /* of any query, source or matrix element, as in ohs_lookup3.h */
#define OHS_LOOKUP3P_MAX_GRID        256

typedef struct ohs_lookup3p ohs_lookup3p;

/* ohs_lookup3_create's table and mesh, and the grid: 0 lets the library choose G = ceil(sqrt(n_tris / 6)) (about one cell per
 * triangle), at least 1 and at most 256; 1 .. 256 is taken as given.  The triangles' inverses, B and the index are computed here, on
 * the host, and go to the device once.
 * Refuses what ohs_lookup3_create refuses, in its words: out == NULL, xyz == NULL, tris == NULL, n_dirs or n_tris out of range, a
 * coordinate that is not finite, a corner index >= n_dirs, a singular triangle; and a grid above 256.  OHS_LOOKUP3P_ERR_NO_DEVICE
 * when no GPU is usable.  *out is NULL after a failure. */
int ohs_lookup3p_create(int device, size_t n_dirs, const float *xyz, size_t n_tris, const uint32_t *tris, unsigned grid, ohs_lookup3p **out);
/* NULL is allowed. */
void ohs_lookup3p_destroy(ohs_lookup3p *lk);
const char *ohs_lookup3p_status_string(int status);
const char *ohs_lookup3p_last_error(void);

/* ohs_lookup3_points on this handle: the same arguments, the same refusals, the same answers. */
int ohs_lookup3p_points(ohs_lookup3p *lk, size_t n, const double *q, uint32_t *idx0, uint32_t *idx1, uint32_t *idx2, float *w1, float *w2,
                        uint32_t *tri);

/* ohs_lookup3_rows on this handle: the same arguments, layout and stride rules, the same refusals, the same answers. */
int ohs_lookup3p_rows(ohs_lookup3p *lk, size_t n_streams, size_t n_segs, size_t n_objects,
                      const double *src, size_t src_stream_stride, size_t src_seg_stride,
                      const double *rot, size_t rot_stream_stride,
                      uint32_t *idx0, uint32_t *idx1, uint32_t *idx2, float *w1, float *w2, uint32_t *tri);

/* The most recent successful call: the queries per chunk, the chunks the call was cut into, and how many of its queries pass 2
 * answered (0, 0 for the last two before the first call and behind a call of no queries).  Refuses any NULL. */
int ohs_lookup3p_last_launch(const ohs_lookup3p *lk, size_t *chunk_queries, size_t *chunks, uint64_t *fallback_queries);

/* The index: G, the cells (6 G^2), the entries of all cells' lists together, the longest cell's list, and the length of the
 * everywhere list.  Refuses any NULL. */
int ohs_lookup3p_index(const ohs_lookup3p *lk, unsigned *grid, size_t *cells, size_t *entries, size_t *longest_list, size_t *everywhere);

/* The handle's table and mesh sizes.  Refuses any NULL. */
int ohs_lookup3p_mesh(const ohs_lookup3p *lk, size_t *n_dirs, size_t *n_tris);

#ifdef __cplusplus
}
#endif
#endif
