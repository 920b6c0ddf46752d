/* ohs_lookup3.h -- C ABI of libohs_lookup3.so: the rows ohs_scene3_process_blended3 reads -- three direction indices and two weights
 * per object, stream and segment over a triangle mesh of the measurements -- found on the device (k_lookup_tri; DESIGN.md section
 * 4.5l, SCENES.md).
 *
 * A library of its own: it links none of the product's code and none of libohs_lookup.so's, exports the ohs_lookup3_* names below and
 * nothing else, and its handle mixes with no other library's.  What it computes is what scene3.triangle_directions of
 * open_headstage_amd defines, bit for bit, as the arithmetic written out below; tests/lookup3_model.py restates it and the device
 * is held to that model's bits.
 *
 * Conventions (ohs_lookup.h's): every function returns a status (0 = ok; the values are ohs_hip.h's OHS_* codes, restated below),
 * ohs_lookup3_last_error() is the thread-local detail of the last failure in THIS library.  EVERY pointer is a HOST pointer.  EVERY
 * call is SYNCHRONOUS: the answers are in the caller's arrays on return.  The handle works on a non-blocking stream of its own.  A
 * refused call writes nothing and leaves the handle as it was; the caller's current device is put back.  A handle is used from
 * one thread at a time.
 *
 * THE ARITHMETIC.  Everything is f64, every operation is rounded by itself (no fused multiply-add), sums are taken in the order
 * written.  P[m] is the table's f32 coordinate widened to f64; u x v = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0).
 *   at create, per triangle (a, b, c) = (P[tris[t][0]], P[tris[t][1]], P[tris[t][2]]), on the host:
 *     row_0 = b x c, row_1 = c x a, row_2 = a x b;  det = (a0 row_0[0] + a1 row_0[1]) + a2 row_0[2];  inv[t][i][j] = row_i[j] / det
 *     |u| = sqrt((u0 u0 + u1 u1) + u2 u2);  the triangle is SINGULAR unless |det| > 1e-9 ((|a| |b|) |c|)  (not-a-number: singular)
 *   pose (rows only)   v' = (R[0][i] v[0] + R[1][i] v[1]) + R[2][i] v[2] for i = 0, 1, 2   (R^T v; rot == NULL: v' = v)
 *   query              q = the point (v', or ohs_lookup3_points' q) rounded to f32 and widened again
 *   the walk           for t = 0, 1, ..: g_i(t) = (inv[t][i][0] q0 + inv[t][i][1] q1) + inv[t][i][2] q2;  m(t) = min(min(g_0, g_1), g_2)
 *                      tri = the smallest t at which m is maximal (a running maximum under strict >)
 *   at the winner      g = g(tri);  top = max(max(g_0, g_1), g_2);  k_i = g_i if g_i > top 2^-20, else 0;  k_i = 0 if k_i < 0
 *                      s = (k_0 + k_1) + k_2;  unless s > 0: k = 1 at the smallest i with g_i = top and 0 elsewhere, s = 1
 *                      weight_i = k_i / s
 *                      the corners tris[tri][i] in the order of descending weight, equal weights by ascending table index:
 *                      idx0, idx1, idx2;  w1, w2 = the second and the third weight as f32, a zero of either sign written +0.0
 * There is no trigonometry here: angles become coordinates on the caller's side.
 *
 * The search is brute force: every query meets every triangle.  Out of scope (none of it is built): pruning the walk by mesh
 * adjacency or a spatial index; rows handed to the scene calls on the device (their ABI takes host rows); a session renderer over
 * scenes. */
#ifndef OHS_LOOKUP3_H
#define OHS_LOOKUP3_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OHS_LOOKUP3_OK              0
#define OHS_LOOKUP3_ERR_INVALID_ARG 1
#define OHS_LOOKUP3_ERR_NO_DEVICE   2
#define OHS_LOOKUP3_ERR_HIP         3
#define OHS_LOOKUP3_ERR_ALLOC       6

#define OHS_LOOKUP3_MAX_OBJECTS     64
#define OHS_LOOKUP3_MAX_DIRECTIONS  65536
#define OHS_LOOKUP3_MAX_TRIANGLES   131072  /* (a closed triangulation of 65536 points has 131068) */
#define OHS_LOOKUP3_MAX_MAGNITUDE   1e15    /* of any query, source or matrix element: R^T v stays below 3e30, finite in f32 */

typedef struct ohs_lookup3 ohs_lookup3;

/* A table of n_dirs points (1 .. 65536), xyz[n_dirs][3] Cartesian f32, and a mesh of n_tris triangles (1 .. 131072) over it,
 * tris[n_tris][3] indices into the table, on `device`.  Both are fixed for the handle's life; the triangles' inverses are computed
 * here, on the host, and go to the device once.
 * Refuses out == NULL, xyz == NULL, tris == NULL, n_dirs or n_tris out of range, a coordinate that is not finite, a corner index
 * >= n_dirs, a singular triangle (the text names the first one and its three indices); OHS_LOOKUP3_ERR_NO_DEVICE when no GPU is
 * usable.  *out is NULL after a failure. */
int ohs_lookup3_create(int device, size_t n_dirs, const float *xyz, size_t n_tris, const uint32_t *tris, ohs_lookup3 **out);
/* NULL is allowed. */
void ohs_lookup3_destroy(ohs_lookup3 *lk);
const char *ohs_lookup3_status_string(int status);
const char *ohs_lookup3_last_error(void);

/* n free-standing queries q[n][3] (f64, the table's Cartesian frame) -> idx0[n], idx1[n], idx2[n], w1[n], w2[n], and where tri is
 * not NULL tri[n], the winning triangle's index.  The five other outputs are all required.
 * n == 0 is OK and touches nothing.  Queries of any count are cut into chunks inside the call; device and pinned memory grow to the
 * largest chunk seen and are then reused.
 * Refused with OHS_LOOKUP3_ERR_INVALID_ARG: lk, q or one of the five outputs NULL; a coordinate that is not finite or above 1e15
 * in magnitude. */
int ohs_lookup3_points(ohs_lookup3 *lk, size_t n, const double *q, uint32_t *idx0, uint32_t *idx1, uint32_t *idx2, float *w1, float *w2,
                       uint32_t *tri);

/* Rows for ohs_scene3_process_blended3: out[(s * n_segs + k) * n_objects + c], i.e. idx_stride = n_segs.
 *   source c of stream s in segment k: src[((s * src_stream_stride + k * src_seg_stride) * n_objects + c) * 3 ..]  (a stride of 0 shares)
 *   pose of stream s in segment k:     rot[(s * rot_stream_stride + k) * 9 ..], row-major 3 x 3; rot == NULL: the identity
 * The query of (s, k, c) is the pose applied to the source (THE ARITHMETIC above), then ohs_lookup3_points' rule.
 * n_streams == 0 or n_segs == 0 is OK and touches nothing.
 * Refused with OHS_LOOKUP3_ERR_INVALID_ARG: everything ohs_lookup3_points refuses (src in q's place); n_objects of 0 or above 64;
 * src_stream_stride neither 0 nor >= (n_segs - 1) * src_seg_stride + 1; rot_stream_stride neither 0 nor >= n_segs; a source or
 * matrix element that would be read and is not finite or above 1e15.  Every element is checked before the first chunk runs. */
int ohs_lookup3_rows(ohs_lookup3 *lk, size_t n_streams, size_t n_segs, size_t n_objects,
                     const double *src, size_t src_stream_stride, size_t src_seg_stride,
                     const double *rot, size_t rot_stream_stride,
                     uint32_t *idx0, uint32_t *idx1, uint32_t *idx2, float *w1, float *w2, uint32_t *tri);

/* The most recent successful call: the triangles the kernel stages at a time, the queries per chunk, and the chunks the call was
 * cut into (0 before the first call and behind a call of no queries).  Refuses any NULL. */
int ohs_lookup3_last_launch(const ohs_lookup3 *lk, unsigned *tile_triangles, size_t *chunk_queries, size_t *chunks);

/* The handle's table and mesh sizes.  Refuses any NULL. */
int ohs_lookup3_mesh(const ohs_lookup3 *lk, size_t *n_dirs, size_t *n_tris);

#ifdef __cplusplus
}
#endif
#endif
