// api_lookup.hip -- ohs_lookup_* (include/ohs_lookup.h): checks, packing into pinned memory, chunks, copies.  Host code only; the kernel
// and its launcher are lookup_kernels.hip's.  Linked into libohs_lookup.so with that unit and nothing else.
#include "../../include/ohs_hip.h"
#include "../../include/ohs_lookup.h"
#include "lookup_internal.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>

static_assert(OHS_LOOKUP_OK == OHS_OK && OHS_LOOKUP_ERR_INVALID_ARG == OHS_ERR_INVALID_ARG && OHS_LOOKUP_ERR_NO_DEVICE == OHS_ERR_NO_DEVICE &&
              OHS_LOOKUP_ERR_HIP == OHS_ERR_HIP && OHS_LOOKUP_ERR_ALLOC == OHS_ERR_ALLOC, "ohs_lookup.h restates ohs_hip.h's status codes");

struct ohs_lookup {
    int device = 0;
    size_t n_dirs = 0;
    double *d_tab = nullptr;
    hipStream_t stream = nullptr;
    // per chunk: packed input (f64) and the three outputs, on the device and pinned on the host; grown, never shrunk
    char *d_in = nullptr, *h_in = nullptr, *d_out = nullptr, *h_out = nullptr;
    size_t in_bytes = 0, out_queries = 0;
    size_t last_chunks = 0;
};

namespace {

thread_local std::string g_err;

int fail(int status, const std::string &what)
{
    g_err = what;
    return status;
}

int hip_fail(hipError_t e, const char *what)
{
    return fail(e == hipErrorOutOfMemory ? OHS_LOOKUP_ERR_ALLOC : OHS_LOOKUP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
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

inline bool usable(double v) { return std::fabs(v) <= OHS_LOOKUP_MAX_MAGNITUDE; }     // (false for NaN and the infinities)

bool all_usable(const double *p, size_t n)
{
    bool ok = true;
    for (size_t i = 0; i < n; ++i) ok &= usable(p[i]);
    return ok;
}

void release(ohs_lookup *lk)
{
    if (lk->d_in) (void)hipFree(lk->d_in);
    if (lk->d_out) (void)hipFree(lk->d_out);
    if (lk->h_in) (void)hipHostFree(lk->h_in);
    if (lk->h_out) (void)hipHostFree(lk->h_out);
    lk->d_in = lk->d_out = lk->h_in = lk->h_out = nullptr;
    lk->in_bytes = lk->out_queries = 0;
}

// room for a chunk of `queries` with `bytes` of packed input
int ensure(ohs_lookup *lk, size_t bytes, size_t queries)
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
        lk->d_out = lk->h_out = nullptr;
        lk->out_queries = 0;
        LK_HIP(hipMalloc((void **)&lk->d_out, queries * 12));
        LK_HIP(hipHostMalloc((void **)&lk->h_out, queries * 12, hipHostMallocDefault));
        lk->out_queries = queries;
    }
    return OHS_LOOKUP_OK;
}

// the chunk's input is packed in h_in (bytes): up, the kernel, the answers down and into the caller's arrays at `at`
int run_chunk(ohs_lookup *lk, ohs::LookupArgs &a, size_t bytes, size_t at, uint32_t *idx0, uint32_t *idx1, float *w)
{
    const size_t n = a.n, cap = lk->out_queries;
    a.tab = lk->d_tab;
    a.n_dirs = (uint32_t)lk->n_dirs;
    a.idx0 = (uint32_t *)lk->d_out;
    a.idx1 = idx1 ? (uint32_t *)lk->d_out + cap : nullptr;
    a.w = idx1 ? (float *)lk->d_out + 2 * cap : nullptr;
    LK_HIP(hipMemcpyAsync(lk->d_in, lk->h_in, bytes, hipMemcpyHostToDevice, lk->stream));
    LK_HIP(ohs::lookup_launch(a, lk->stream));
    LK_HIP(hipMemcpyAsync(lk->h_out, lk->d_out, n * 4, hipMemcpyDeviceToHost, lk->stream));
    if (idx1) {
        LK_HIP(hipMemcpyAsync(lk->h_out + cap * 4, lk->d_out + cap * 4, n * 4, hipMemcpyDeviceToHost, lk->stream));
        LK_HIP(hipMemcpyAsync(lk->h_out + cap * 8, lk->d_out + cap * 8, n * 4, hipMemcpyDeviceToHost, lk->stream));
    }
    LK_HIP(hipStreamSynchronize(lk->stream));
    std::memcpy(idx0 + at, lk->h_out, n * 4);
    if (idx1) {
        std::memcpy(idx1 + at, lk->h_out + cap * 4, n * 4);
        std::memcpy(w + at, lk->h_out + cap * 8, n * 4);
    }
    return OHS_LOOKUP_OK;
}

// one of the two arrays of ohs_lookup_rows: entries of `elems` doubles at p[(s * stream_stride + k * seg_stride) * elems], shared
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

int check_outputs(const ohs_lookup *lk, const uint32_t *idx0, const uint32_t *idx1, const float *w)
{
    if (!lk) return fail(OHS_LOOKUP_ERR_INVALID_ARG, "lookup is NULL");
    if (!idx0) return fail(OHS_LOOKUP_ERR_INVALID_ARG, "idx0 is NULL");
    if ((idx1 == nullptr) != (w == nullptr)) return fail(OHS_LOOKUP_ERR_INVALID_ARG, "idx1 and w are both NULL or both given");
    return OHS_LOOKUP_OK;
}

}  // namespace

extern "C" {

const char *ohs_lookup_status_string(int s)
{
    switch (s) {
    case OHS_LOOKUP_OK: return "OHS_OK";
    case OHS_LOOKUP_ERR_INVALID_ARG: return "OHS_ERR_INVALID_ARG";
    case OHS_LOOKUP_ERR_NO_DEVICE: return "OHS_ERR_NO_DEVICE";
    case OHS_LOOKUP_ERR_HIP: return "OHS_ERR_HIP";
    case OHS_LOOKUP_ERR_ALLOC: return "OHS_ERR_ALLOC";
    default: return "OHS_ERR_UNKNOWN";
    }
}

const char *ohs_lookup_last_error(void) { return g_err.c_str(); }

int ohs_lookup_create(int device, size_t n_dirs, const float *xyz, ohs_lookup **out)
{
    if (!out) return fail(OHS_LOOKUP_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (!xyz) return fail(OHS_LOOKUP_ERR_INVALID_ARG, "xyz is NULL");
    if (n_dirs < 1 || n_dirs > OHS_LOOKUP_MAX_DIRECTIONS)
        return fail(OHS_LOOKUP_ERR_INVALID_ARG, "n_dirs " + std::to_string(n_dirs) + " is outside 1 .. 65536");
    for (size_t i = 0; i < 3 * n_dirs; ++i)
        if (!std::isfinite(xyz[i])) return fail(OHS_LOOKUP_ERR_INVALID_ARG, "xyz[" + std::to_string(i) + "] is not finite");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        return fail(OHS_LOOKUP_ERR_NO_DEVICE, "no HIP device");
    }
    if (device < 0 || device >= count) return fail(OHS_LOOKUP_ERR_NO_DEVICE, "device " + std::to_string(device) + " of " + std::to_string(count));
    DeviceGuard guard;
    if (!guard.set(device)) return fail(OHS_LOOKUP_ERR_NO_DEVICE, "hipSetDevice failed");
    ohs_lookup *lk = new (std::nothrow) ohs_lookup;
    double *wide = new (std::nothrow) double[3 * n_dirs];
    if (!lk || !wide) {
        delete lk;
        delete[] wide;
        return fail(OHS_LOOKUP_ERR_ALLOC, "out of host memory");
    }
    for (size_t i = 0; i < 3 * n_dirs; ++i) wide[i] = (double)xyz[i];
    lk->device = device;
    lk->n_dirs = n_dirs;
    hipError_t e = hipStreamCreateWithFlags(&lk->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void **)&lk->d_tab, 3 * n_dirs * sizeof(double));
    if (e == hipSuccess) e = hipMemcpyAsync(lk->d_tab, wide, 3 * n_dirs * sizeof(double), hipMemcpyHostToDevice, lk->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(lk->stream);
    delete[] wide;
    if (e != hipSuccess) {
        int st = hip_fail(e, "ohs_lookup_create");
        std::string keep = g_err;
        ohs_lookup_destroy(lk);
        g_err = keep;
        return st;
    }
    *out = lk;
    return OHS_LOOKUP_OK;
}

void ohs_lookup_destroy(ohs_lookup *lk)
{
    if (!lk) return;
    DeviceGuard guard;
    (void)guard.set(lk->device);
    if (lk->stream) (void)hipStreamSynchronize(lk->stream);
    release(lk);
    if (lk->d_tab) (void)hipFree(lk->d_tab);
    if (lk->stream) (void)hipStreamDestroy(lk->stream);
    delete lk;
}

int ohs_lookup_points(ohs_lookup *lk, size_t n, const double *q, uint32_t *idx0, uint32_t *idx1, float *w)
{
    if (!lk) return fail(OHS_LOOKUP_ERR_INVALID_ARG, "lookup is NULL");
    if (n == 0) {
        lk->last_chunks = 0;
        return OHS_LOOKUP_OK;
    }
    if (!q) return fail(OHS_LOOKUP_ERR_INVALID_ARG, "q is NULL");
    if (int st = check_outputs(lk, idx0, idx1, w)) return st;
    if (n > (size_t(1) << 56)) return fail(OHS_LOOKUP_ERR_INVALID_ARG, "n is too large");
    if (!all_usable(q, 3 * n)) return fail(OHS_LOOKUP_ERR_INVALID_ARG, "a query coordinate is not finite or above 1e100 in magnitude");
    DeviceGuard guard;
    if (!guard.set(lk->device)) return fail(OHS_LOOKUP_ERR_HIP, "hipSetDevice failed");
    const size_t Q = ohs::LOOKUP_CHUNK_QUERIES;
    size_t chunks = 0;
    for (size_t at = 0; at < n; at += Q, ++chunks) {
        const size_t nq = n - at < Q ? n - at : Q, bytes = nq * 3 * sizeof(double);
        if (int st = ensure(lk, bytes, nq)) return st;
        std::memcpy(lk->h_in, q + 3 * at, bytes);
        ohs::LookupArgs a{};
        a.n = (uint32_t)nq;
        a.q = (const double *)lk->d_in;
        if (int st = run_chunk(lk, a, bytes, at, idx0, idx1, w)) return st;
    }
    lk->last_chunks = chunks;
    return OHS_LOOKUP_OK;
}

int ohs_lookup_rows(ohs_lookup *lk, size_t n_streams, size_t n_segs, size_t n_objects, const double *src, size_t src_stream_stride,
                    size_t src_seg_stride, const double *rot, size_t rot_stream_stride, uint32_t *idx0, uint32_t *idx1, float *w)
{
    if (!lk) return fail(OHS_LOOKUP_ERR_INVALID_ARG, "lookup is NULL");
    if (n_objects < 1 || n_objects > OHS_LOOKUP_MAX_OBJECTS)
        return fail(OHS_LOOKUP_ERR_INVALID_ARG, "n_objects " + std::to_string(n_objects) + " is outside 1 .. 64");
    if (n_streams == 0 || n_segs == 0) {
        lk->last_chunks = 0;
        return OHS_LOOKUP_OK;
    }
    if (!src) return fail(OHS_LOOKUP_ERR_INVALID_ARG, "src is NULL");
    if (int st = check_outputs(lk, idx0, idx1, w)) return st;
    if (n_streams > (size_t(1) << 24) || n_segs > (size_t(1) << 24)) return fail(OHS_LOOKUP_ERR_INVALID_ARG, "n_streams or n_segs above 2^24");
    if (src_stream_stride != 0 && src_stream_stride < (n_segs - 1) * src_seg_stride + 1)
        return fail(OHS_LOOKUP_ERR_INVALID_ARG, "src_stream_stride " + std::to_string(src_stream_stride) + " is neither 0 nor >= " +
                                                    std::to_string((n_segs - 1) * src_seg_stride + 1) + ": streams' sources would overlap");
    if (rot && rot_stream_stride != 0 && rot_stream_stride < n_segs)
        return fail(OHS_LOOKUP_ERR_INVALID_ARG, "rot_stream_stride " + std::to_string(rot_stream_stride) + " is neither 0 nor >= n_segs " +
                                                    std::to_string(n_segs));
    const size_t K = n_objects;
    const RowSource S{src, src_stream_stride, src_seg_stride, 3 * K, n_segs};
    const RowSource R{rot, rot_stream_stride, 1, 9, n_segs};
    if (!S.all_usable_entries(n_streams)) return fail(OHS_LOOKUP_ERR_INVALID_ARG, "a source coordinate is not finite or above 1e100 in magnitude");
    if (rot && !R.all_usable_entries(n_streams)) return fail(OHS_LOOKUP_ERR_INVALID_ARG, "a matrix element is not finite or above 1e100 in magnitude");
    DeviceGuard guard;
    if (!guard.set(lk->device)) return fail(OHS_LOOKUP_ERR_HIP, "hipSetDevice failed");
    const size_t n = n_streams * n_segs * K, Q = ohs::LOOKUP_CHUNK_QUERIES;
    size_t chunks = 0;
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
        ohs::LookupArgs a{};
        a.n = (uint32_t)nq;
        a.src = (const double *)lk->d_in;
        a.rot = rot ? (const double *)(lk->d_in + src_bytes) : nullptr;
        a.g0 = at, a.n_segs = n_segs, a.K = (uint32_t)K;
        a.src_a = S.a(), a.src_b = S.b(), a.src_base = src_lo;
        a.rot_a = R.a(), a.rot_base = rot_lo;
        if (int st = run_chunk(lk, a, src_bytes + rot_bytes, at, idx0, idx1, w)) return st;
    }
    lk->last_chunks = chunks;
    return OHS_LOOKUP_OK;
}

int ohs_lookup_last_launch(const ohs_lookup *lk, unsigned *tile_points, size_t *chunk_queries, size_t *chunks)
{
    if (!lk) return fail(OHS_LOOKUP_ERR_INVALID_ARG, "lookup is NULL");
    if (!tile_points || !chunk_queries || !chunks) return fail(OHS_LOOKUP_ERR_INVALID_ARG, "an out-parameter is NULL");
    *tile_points = ohs::LOOKUP_TILE_POINTS;
    *chunk_queries = ohs::LOOKUP_CHUNK_QUERIES;
    *chunks = lk->last_chunks;
    return OHS_LOOKUP_OK;
}

}  // extern "C"
