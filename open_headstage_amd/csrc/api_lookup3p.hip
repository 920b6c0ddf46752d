// api_lookup3p.hip -- ohs_lookup3p_* (include/ohs_lookup3p.h): checks, the triangles' inverses, the index over the sphere and the
// certificate's bound (lookup3p_body.hpp), packing into pinned memory, chunks, copies.  Host code only; the kernels and their launcher
// are lookup3p_kernels.hip's.  Linked into libohs_lookup3p.so with that unit and nothing else.  The checks and the staging are
// api_lookup3.hip's, restated here: that unit is frozen and none of its objects is linked.
#include "../../include/ohs_hip.h"
#include "../../include/ohs_lookup3p.h"
#include "lookup3p_internal.h"
#include "lookup3p_body.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

static_assert(OHS_LOOKUP3P_OK == OHS_OK && OHS_LOOKUP3P_ERR_INVALID_ARG == OHS_ERR_INVALID_ARG && OHS_LOOKUP3P_ERR_NO_DEVICE == OHS_ERR_NO_DEVICE &&
              OHS_LOOKUP3P_ERR_HIP == OHS_ERR_HIP && OHS_LOOKUP3P_ERR_ALLOC == OHS_ERR_ALLOC, "ohs_lookup3p.h restates ohs_hip.h's status codes");

struct ohs_lookup3p {
    int device = 0;
    size_t n_dirs = 0, n_tris = 0;
    double *d_inv = nullptr;        // [n_tris][LOOKUP3P_INV_STRIDE]
    uint32_t *d_tris = nullptr;     // [n_tris][3]
    // the index (lookup3p_body.hpp): cell_start [cells + 1], cell_tris [entries], everywhere [n_everywhere]; B of the certificate
    uint32_t *d_cell_start = nullptr, *d_cell_tris = nullptr, *d_everywhere = nullptr;
    unsigned grid = 0;
    size_t cells = 0, entries = 0, longest = 0, n_everywhere = 0;
    double bound = 0.0;
    hipStream_t stream = nullptr;
    // per chunk: packed input (f64), the six outputs and pass 2's list, on the device; input and outputs pinned on the host as well;
    // grown, never shrunk.  The list's count: one word on the device, one pinned.
    char *d_in = nullptr, *h_in = nullptr, *d_out = nullptr, *h_out = nullptr;
    uint32_t *d_rest = nullptr, *d_rest_count = nullptr, *h_rest_count = nullptr;
    size_t in_bytes = 0, out_queries = 0;
    size_t last_chunks = 0;
    uint64_t last_fallback = 0;
};

namespace {

constexpr int N_OUT = 6;        // idx0, idx1, idx2, w1, w2, tri: four bytes each per query

thread_local std::string g_err;

int fail(int status, const std::string &what)
{
    g_err = what;
    return status;
}

int hip_fail(hipError_t e, const char *what)
{
    return fail(e == hipErrorOutOfMemory ? OHS_LOOKUP3P_ERR_ALLOC : OHS_LOOKUP3P_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define LK_HIP(call)                                  \
    do {                                              \
        hipError_t e_ = (call);                       \
        if (e_ != hipSuccess) return hip_fail(e_, #call); \
    } while (0)

// the caller's current device is put back when a call returns
struct DeviceGuard {
    int prev = -1;
    bool set(int device)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        return hipSetDevice(device) == hipSuccess;
    }
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

inline bool usable(double v) { return std::fabs(v) <= OHS_LOOKUP3P_MAX_MAGNITUDE; }    // (false for NaN and the infinities)

bool all_usable(const double *p, size_t n)
{
    bool ok = true;
    for (size_t i = 0; i < n; ++i) ok &= usable(p[i]);
    return ok;
}

void release(ohs_lookup3p *lk)
{
    if (lk->d_in) (void)hipFree(lk->d_in);
    if (lk->d_out) (void)hipFree(lk->d_out);
    if (lk->h_in) (void)hipHostFree(lk->h_in);
    if (lk->h_out) (void)hipHostFree(lk->h_out);
    if (lk->d_rest) (void)hipFree(lk->d_rest);
    lk->d_in = lk->d_out = lk->h_in = lk->h_out = nullptr;
    lk->d_rest = nullptr;
    lk->in_bytes = lk->out_queries = 0;
}

// room for a chunk of `queries` with `bytes` of packed input
int ensure(ohs_lookup3p *lk, size_t bytes, size_t queries)
{
    if (bytes > lk->in_bytes) {
        if (lk->d_in) (void)hipFree(lk->d_in);
        if (lk->h_in) (void)hipHostFree(lk->h_in);
        lk->d_in = lk->h_in = nullptr;
        lk->in_bytes = 0;
        LK_HIP(hipMalloc((void **)&lk->d_in, bytes));
        LK_HIP(hipHostMalloc((void **)&lk->h_in, bytes, hipHostMallocDefault));
        lk->in_bytes = bytes;
    }
    if (queries > lk->out_queries) {
        if (lk->d_out) (void)hipFree(lk->d_out);
        if (lk->h_out) (void)hipHostFree(lk->h_out);
        if (lk->d_rest) (void)hipFree(lk->d_rest);
        lk->d_out = lk->h_out = nullptr;
        lk->d_rest = nullptr;
        lk->out_queries = 0;
        LK_HIP(hipMalloc((void **)&lk->d_out, queries * 4 * N_OUT));
        LK_HIP(hipHostMalloc((void **)&lk->h_out, queries * 4 * N_OUT, hipHostMallocDefault));
        LK_HIP(hipMalloc((void **)&lk->d_rest, queries * 4));
        lk->out_queries = queries;
    }
    return OHS_LOOKUP3P_OK;
}

// the caller's six arrays (tri may be NULL), in the order of the staging's planes
struct Outputs {
    void *p[N_OUT];
};

// the chunk's input is packed in h_in (bytes): up, the two passes, the answers and pass 2's count down and into the caller's arrays
// at `at`; fallback grows by the count
int run_chunk(ohs_lookup3p *lk, ohs::Lookup3pArgs &a, size_t bytes, size_t at, const Outputs &o, uint64_t &fallback)
{
    const size_t n = a.n, cap = lk->out_queries;
    const int planes = o.p[N_OUT - 1] ? N_OUT : N_OUT - 1;
    a.inv = lk->d_inv;
    a.tris = lk->d_tris;
    a.n_tris = (uint32_t)lk->n_tris;
    a.cell_start = lk->d_cell_start;
    a.cell_tris = lk->d_cell_tris;
    a.everywhere = lk->d_everywhere;
    a.grid = lk->grid;
    a.n_everywhere = (uint32_t)lk->n_everywhere;
    a.bound = lk->bound;
    a.rest = lk->d_rest;            // (cap >= n entries)
    a.rest_count = lk->d_rest_count;
    a.idx0 = (uint32_t *)lk->d_out;
    a.idx1 = (uint32_t *)lk->d_out + cap;
    a.idx2 = (uint32_t *)lk->d_out + 2 * cap;
    a.w1 = (float *)lk->d_out + 3 * cap;
    a.w2 = (float *)lk->d_out + 4 * cap;
    a.tri = planes == N_OUT ? (uint32_t *)lk->d_out + 5 * cap : nullptr;
    LK_HIP(hipMemcpyAsync(lk->d_in, lk->h_in, bytes, hipMemcpyHostToDevice, lk->stream));
    LK_HIP(hipMemsetAsync(lk->d_rest_count, 0, 4, lk->stream));
    LK_HIP(ohs::lookup3p_launch(a, lk->stream));
    for (int j = 0; j < planes; ++j)
        LK_HIP(hipMemcpyAsync(lk->h_out + j * cap * 4, lk->d_out + j * cap * 4, n * 4, hipMemcpyDeviceToHost, lk->stream));
    LK_HIP(hipMemcpyAsync(lk->h_rest_count, lk->d_rest_count, 4, hipMemcpyDeviceToHost, lk->stream));
    LK_HIP(hipStreamSynchronize(lk->stream));
    for (int j = 0; j < planes; ++j) std::memcpy((char *)o.p[j] + at * 4, lk->h_out + j * cap * 4, n * 4);
    fallback += *lk->h_rest_count;
    return OHS_LOOKUP3P_OK;
}

// one of the two arrays of ohs_lookup3p_rows: entries of `elems` doubles at p[(s * stream_stride + k * seg_stride) * elems], shared
// across streams and / or segments where a stride is 0
struct RowSource {
    const double *p;
    size_t stream_stride, seg_stride, elems, n_segs;
    bool per_stream() const { return stream_stride != 0; }
    bool per_seg() const { return seg_stride != 0; }
    // packed entry index of (s, k) = s * a() + k * b()
    size_t a() const { return per_stream() ? (per_seg() ? n_segs : 1) : 0; }
    size_t b() const { return per_seg() ? 1 : 0; }
    size_t entries(size_t n_streams) const { return (per_stream() ? n_streams : 1) * (per_seg() ? n_segs : 1); }
    const double *entry(size_t j) const
    {
        size_t s = 0, k = 0;
        if (per_stream() && per_seg())
            s = j / n_segs, k = j % n_segs;
        else if (per_stream())
            s = j;
        else
            k = j;
        return p + (s * stream_stride + k * seg_stride) * elems;
    }
    // the packed entries a chunk covering (s_lo, k_lo) .. (s_hi, k_hi) names: [lo, hi]
    void range(size_t s_lo, size_t k_lo, size_t s_hi, size_t k_hi, size_t &lo, size_t &hi) const
    {
        if (per_stream() && per_seg())
            lo = s_lo * n_segs + k_lo, hi = s_hi * n_segs + k_hi;
        else if (per_stream())
            lo = s_lo, hi = s_hi;
        else if (per_seg()) {
            if (s_lo == s_hi)
                lo = k_lo, hi = k_hi;
            else
                lo = 0, hi = n_segs - 1;
        } else
            lo = hi = 0;
    }
    bool all_usable_entries(size_t n_streams) const
    {
        bool ok = true;
        for (size_t j = 0, n = entries(n_streams); j < n; ++j) ok &= all_usable(entry(j), elems);
        return ok;
    }
};

int check_outputs(const uint32_t *idx0, const uint32_t *idx1, const uint32_t *idx2, const float *w1, const float *w2)
{
    if (!idx0 || !idx1 || !idx2) return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "idx0, idx1 or idx2 is NULL");
    if (!w1 || !w2) return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "w1 or w2 is NULL");
    return OHS_LOOKUP3P_OK;
}

}  // namespace

extern "C" {

const char *ohs_lookup3p_status_string(int s)
{
    switch (s) {
    case OHS_LOOKUP3P_OK: return "OHS_OK";
    case OHS_LOOKUP3P_ERR_INVALID_ARG: return "OHS_ERR_INVALID_ARG";
    case OHS_LOOKUP3P_ERR_NO_DEVICE: return "OHS_ERR_NO_DEVICE";
    case OHS_LOOKUP3P_ERR_HIP: return "OHS_ERR_HIP";
    case OHS_LOOKUP3P_ERR_ALLOC: return "OHS_ERR_ALLOC";
    default: return "OHS_ERR_UNKNOWN";
    }
}

const char *ohs_lookup3p_last_error(void) { return g_err.c_str(); }

int ohs_lookup3p_create(int device, size_t n_dirs, const float *xyz, size_t n_tris, const uint32_t *tris, unsigned grid, ohs_lookup3p **out)
{
    if (!out) return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (!xyz) return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "xyz is NULL");
    if (!tris) return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "tris is NULL");
    if (n_dirs < 1 || n_dirs > OHS_LOOKUP3P_MAX_DIRECTIONS)
        return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "n_dirs " + std::to_string(n_dirs) + " is outside 1 .. 65536");
    if (n_tris < 1 || n_tris > OHS_LOOKUP3P_MAX_TRIANGLES)
        return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "n_tris " + std::to_string(n_tris) + " is outside 1 .. 131072");
    if (grid > OHS_LOOKUP3P_MAX_GRID) return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "grid " + std::to_string(grid) + " is outside 0 .. 256");
    for (size_t i = 0; i < 3 * n_dirs; ++i)
        if (!std::isfinite(xyz[i])) return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "xyz[" + std::to_string(i) + "] is not finite");
    for (size_t i = 0; i < 3 * n_tris; ++i)
        if (tris[i] >= n_dirs)
            return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "triangle " + std::to_string(i / 3) + " names direction " + std::to_string(tris[i]) + " of " +
                                                         std::to_string(n_dirs));
    const unsigned IS = ohs::LOOKUP3P_INV_STRIDE;
    std::vector<double> inv;
    ohs::Lookup3pIndex ix;
    try {
        inv.assign(IS * n_tris, 0.0);
    } catch (const std::bad_alloc &) {
        return fail(OHS_LOOKUP3P_ERR_ALLOC, "out of host memory");
    }
    for (size_t t = 0; t < n_tris; ++t) {
        double p[3][3];
        for (int c = 0; c < 3; ++c)
            for (int j = 0; j < 3; ++j) p[c][j] = (double)xyz[3 * (size_t)tris[3 * t + c] + j];
        if (!ohs::lookup3_inverse(p[0], p[1], p[2], &inv[IS * t]))
            return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "triangle " + std::to_string(t) + " (" + std::to_string(tris[3 * t]) + ", " +
                                                         std::to_string(tris[3 * t + 1]) + ", " + std::to_string(tris[3 * t + 2]) +
                                                         ") is singular: its three directions lie in one plane through the origin");
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        return fail(OHS_LOOKUP3P_ERR_NO_DEVICE, "no HIP device");
    }
    if (device < 0 || device >= count) return fail(OHS_LOOKUP3P_ERR_NO_DEVICE, "device " + std::to_string(device) + " of " + std::to_string(count));
    DeviceGuard guard;
    if (!guard.set(device)) return fail(OHS_LOOKUP3P_ERR_NO_DEVICE, "hipSetDevice failed");
    try {
        ohs::lookup3p_build_index(xyz, tris, n_tris, grid ? grid : ohs::lookup3p_choose_grid(n_tris), ix);
    } catch (const std::bad_alloc &) {
        return fail(OHS_LOOKUP3P_ERR_ALLOC, "out of host memory");
    }
    ohs_lookup3p *lk = new (std::nothrow) ohs_lookup3p;
    if (!lk) return fail(OHS_LOOKUP3P_ERR_ALLOC, "out of host memory");
    lk->device = device;
    lk->n_dirs = n_dirs;
    lk->n_tris = n_tris;
    lk->grid = ix.G;
    lk->cells = ix.cell_start.size() - 1;
    lk->entries = ix.cell_tris.size();
    lk->longest = ix.longest;
    lk->n_everywhere = ix.everywhere.size();
    lk->bound = ohs::lookup3p_bound(inv.data(), n_tris, IS);
    // (an empty list still gets a word, so that no pointer handed to the kernels is NULL)
    const size_t start_bytes = ix.cell_start.size() * 4, tris_bytes = ix.cell_tris.size() * 4, every_bytes = ix.everywhere.size() * 4;
    hipError_t e = hipStreamCreateWithFlags(&lk->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void **)&lk->d_inv, IS * n_tris * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&lk->d_tris, 3 * n_tris * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&lk->d_cell_start, start_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&lk->d_cell_tris, tris_bytes + 4);
    if (e == hipSuccess) e = hipMalloc((void **)&lk->d_everywhere, every_bytes + 4);
    if (e == hipSuccess) e = hipMalloc((void **)&lk->d_rest_count, 4);
    if (e == hipSuccess) e = hipHostMalloc((void **)&lk->h_rest_count, 4, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMemcpyAsync(lk->d_inv, inv.data(), IS * n_tris * sizeof(double), hipMemcpyHostToDevice, lk->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(lk->d_tris, tris, 3 * n_tris * sizeof(uint32_t), hipMemcpyHostToDevice, lk->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(lk->d_cell_start, ix.cell_start.data(), start_bytes, hipMemcpyHostToDevice, lk->stream);
    if (e == hipSuccess && tris_bytes) e = hipMemcpyAsync(lk->d_cell_tris, ix.cell_tris.data(), tris_bytes, hipMemcpyHostToDevice, lk->stream);
    if (e == hipSuccess && every_bytes) e = hipMemcpyAsync(lk->d_everywhere, ix.everywhere.data(), every_bytes, hipMemcpyHostToDevice, lk->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(lk->stream);
    if (e != hipSuccess) {
        int st = hip_fail(e, "ohs_lookup3p_create");
        std::string keep = g_err;
        ohs_lookup3p_destroy(lk);
        g_err = keep;
        return st;
    }
    *out = lk;
    return OHS_LOOKUP3P_OK;
}

void ohs_lookup3p_destroy(ohs_lookup3p *lk)
{
    if (!lk) return;
    DeviceGuard guard;
    (void)guard.set(lk->device);
    if (lk->stream) (void)hipStreamSynchronize(lk->stream);
    release(lk);
    if (lk->d_inv) (void)hipFree(lk->d_inv);
    if (lk->d_tris) (void)hipFree(lk->d_tris);
    if (lk->d_cell_start) (void)hipFree(lk->d_cell_start);
    if (lk->d_cell_tris) (void)hipFree(lk->d_cell_tris);
    if (lk->d_everywhere) (void)hipFree(lk->d_everywhere);
    if (lk->d_rest_count) (void)hipFree(lk->d_rest_count);
    if (lk->h_rest_count) (void)hipHostFree(lk->h_rest_count);
    if (lk->stream) (void)hipStreamDestroy(lk->stream);
    delete lk;
}

int ohs_lookup3p_points(ohs_lookup3p *lk, size_t n, const double *q, uint32_t *idx0, uint32_t *idx1, uint32_t *idx2, float *w1, float *w2,
                        uint32_t *tri)
{
    if (!lk) return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "lookup is NULL");
    if (n == 0) {
        lk->last_chunks = 0;
        lk->last_fallback = 0;
        return OHS_LOOKUP3P_OK;
    }
    if (!q) return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "q is NULL");
    if (int st = check_outputs(idx0, idx1, idx2, w1, w2)) return st;
    if (n > (size_t(1) << 56)) return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "n is too large");
    if (!all_usable(q, 3 * n)) return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "a query coordinate is not finite or above 1e15 in magnitude");
    DeviceGuard guard;
    if (!guard.set(lk->device)) return fail(OHS_LOOKUP3P_ERR_HIP, "hipSetDevice failed");
    const Outputs o{{idx0, idx1, idx2, w1, w2, tri}};
    const size_t Q = ohs::LOOKUP3P_CHUNK_QUERIES;
    size_t chunks = 0;
    uint64_t fallback = 0;
    for (size_t at = 0; at < n; at += Q, ++chunks) {
        const size_t nq = n - at < Q ? n - at : Q, bytes = nq * 3 * sizeof(double);
        if (int st = ensure(lk, bytes, nq)) return st;
        std::memcpy(lk->h_in, q + 3 * at, bytes);
        ohs::Lookup3pArgs a{};
        a.n = (uint32_t)nq;
        a.q = (const double *)lk->d_in;
        if (int st = run_chunk(lk, a, bytes, at, o, fallback)) return st;
    }
    lk->last_chunks = chunks;
    lk->last_fallback = fallback;
    return OHS_LOOKUP3P_OK;
}

int ohs_lookup3p_rows(ohs_lookup3p *lk, size_t n_streams, size_t n_segs, size_t n_objects, const double *src, size_t src_stream_stride,
                      size_t src_seg_stride, const double *rot, size_t rot_stream_stride, uint32_t *idx0, uint32_t *idx1, uint32_t *idx2,
                      float *w1, float *w2, uint32_t *tri)
{
    if (!lk) return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "lookup is NULL");
    if (n_objects < 1 || n_objects > OHS_LOOKUP3P_MAX_OBJECTS)
        return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "n_objects " + std::to_string(n_objects) + " is outside 1 .. 64");
    if (n_streams == 0 || n_segs == 0) {
        lk->last_chunks = 0;
        lk->last_fallback = 0;
        return OHS_LOOKUP3P_OK;
    }
    if (!src) return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "src is NULL");
    if (int st = check_outputs(idx0, idx1, idx2, w1, w2)) return st;
    if (n_streams > (size_t(1) << 24) || n_segs > (size_t(1) << 24)) return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "n_streams or n_segs above 2^24");
    if (src_stream_stride != 0 && src_stream_stride < (n_segs - 1) * src_seg_stride + 1)
        return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "src_stream_stride " + std::to_string(src_stream_stride) + " is neither 0 nor >= " +
                                                     std::to_string((n_segs - 1) * src_seg_stride + 1) + ": streams' sources would overlap");
    if (rot && rot_stream_stride != 0 && rot_stream_stride < n_segs)
        return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "rot_stream_stride " + std::to_string(rot_stream_stride) + " is neither 0 nor >= n_segs " +
                                                     std::to_string(n_segs));
    const size_t K = n_objects;
    const RowSource S{src, src_stream_stride, src_seg_stride, 3 * K, n_segs};
    const RowSource R{rot, rot_stream_stride, 1, 9, n_segs};
    if (!S.all_usable_entries(n_streams)) return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "a source coordinate is not finite or above 1e15 in magnitude");
    if (rot && !R.all_usable_entries(n_streams)) return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "a matrix element is not finite or above 1e15 in magnitude");
    DeviceGuard guard;
    if (!guard.set(lk->device)) return fail(OHS_LOOKUP3P_ERR_HIP, "hipSetDevice failed");
    const Outputs o{{idx0, idx1, idx2, w1, w2, tri}};
    const size_t n = n_streams * n_segs * K, Q = ohs::LOOKUP3P_CHUNK_QUERIES;
    size_t chunks = 0;
    uint64_t fallback = 0;
    for (size_t at = 0; at < n; at += Q, ++chunks) {
        const size_t nq = n - at < Q ? n - at : Q;
        const size_t sk_lo = at / K, sk_hi = (at + nq - 1) / K;
        const size_t s_lo = sk_lo / n_segs, k_lo = sk_lo % n_segs, s_hi = sk_hi / n_segs, k_hi = sk_hi % n_segs;
        size_t src_lo, src_hi, rot_lo = 0, rot_hi = 0;
        S.range(s_lo, k_lo, s_hi, k_hi, src_lo, src_hi);
        if (rot) R.range(s_lo, k_lo, s_hi, k_hi, rot_lo, rot_hi);
        const size_t src_bytes = (src_hi - src_lo + 1) * S.elems * sizeof(double);
        const size_t rot_bytes = rot ? (rot_hi - rot_lo + 1) * R.elems * sizeof(double) : 0;
        if (int st = ensure(lk, src_bytes + rot_bytes, nq)) return st;
        for (size_t j = src_lo; j <= src_hi; ++j) std::memcpy(lk->h_in + (j - src_lo) * S.elems * sizeof(double), S.entry(j), S.elems * sizeof(double));
        for (size_t j = rot_lo; rot && j <= rot_hi; ++j)
            std::memcpy(lk->h_in + src_bytes + (j - rot_lo) * R.elems * sizeof(double), R.entry(j), R.elems * sizeof(double));
        ohs::Lookup3pArgs a{};
        a.n = (uint32_t)nq;
        a.src = (const double *)lk->d_in;
        a.rot = rot ? (const double *)(lk->d_in + src_bytes) : nullptr;
        a.g0 = at, a.n_segs = n_segs, a.K = (uint32_t)K;
        a.src_a = S.a(), a.src_b = S.b(), a.src_base = src_lo;
        a.rot_a = R.a(), a.rot_base = rot_lo;
        if (int st = run_chunk(lk, a, src_bytes + rot_bytes, at, o, fallback)) return st;
    }
    lk->last_chunks = chunks;
    lk->last_fallback = fallback;
    return OHS_LOOKUP3P_OK;
}

int ohs_lookup3p_last_launch(const ohs_lookup3p *lk, size_t *chunk_queries, size_t *chunks, uint64_t *fallback_queries)
{
    if (!lk) return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "lookup is NULL");
    if (!chunk_queries || !chunks || !fallback_queries) return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "an out-parameter is NULL");
    *chunk_queries = ohs::LOOKUP3P_CHUNK_QUERIES;
    *chunks = lk->last_chunks;
    *fallback_queries = lk->last_fallback;
    return OHS_LOOKUP3P_OK;
}

int ohs_lookup3p_index(const ohs_lookup3p *lk, unsigned *grid, size_t *cells, size_t *entries, size_t *longest_list, size_t *everywhere)
{
    if (!lk) return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "lookup is NULL");
    if (!grid || !cells || !entries || !longest_list || !everywhere) return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "an out-parameter is NULL");
    *grid = lk->grid;
    *cells = lk->cells;
    *entries = lk->entries;
    *longest_list = lk->longest;
    *everywhere = lk->n_everywhere;
    return OHS_LOOKUP3P_OK;
}

int ohs_lookup3p_mesh(const ohs_lookup3p *lk, size_t *n_dirs, size_t *n_tris)
{
    if (!lk) return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "lookup is NULL");
    if (!n_dirs || !n_tris) return fail(OHS_LOOKUP3P_ERR_INVALID_ARG, "an out-parameter is NULL");
    *n_dirs = lk->n_dirs;
    *n_tris = lk->n_tris;
    return OHS_LOOKUP3P_OK;
}

}  // extern "C"
