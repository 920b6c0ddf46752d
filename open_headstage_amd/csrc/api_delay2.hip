// api_delay2.hip -- ohs_delay2_* (include/ohs_delay2.h): checks, the rows and their FIR taps into pinned staging, the carry, the launch
// record with the filtered tiles counted from the staged rows.  Host code only; the kernels and their launcher are
// delay2_kernels.hip's.  Linked into libohs_delay2.so with that unit and nothing else.
#include "../../include/ohs_hip.h"
#include "../../include/ohs_delay2.h"
#include "delay2_internal.h"
#include "delay2_body.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

static_assert(OHS_DELAY2_OK == OHS_OK && OHS_DELAY2_ERR_INVALID_ARG == OHS_ERR_INVALID_ARG && OHS_DELAY2_ERR_NO_DEVICE == OHS_ERR_NO_DEVICE &&
              OHS_DELAY2_ERR_HIP == OHS_ERR_HIP && OHS_DELAY2_ERR_ALLOC == OHS_ERR_ALLOC, "ohs_delay2.h restates ohs_hip.h's status codes");
static_assert(OHS_DELAY2_FIR_RADIUS == ohs::DELAY2_RADIUS, "ohs_delay2.h restates delay2_body.hpp's radius");

namespace {

constexpr int kSlots = 4;               // calls of a handle whose rows are staged at a time
constexpr size_t kSlotSegs = 16;        // segments a slot has room for from create on
constexpr size_t kSlotBytes = size_t(8) << 20;     // ... but no more than this

// the rows of one call: pinned on the host, their copy on the device, and the event behind the call that read them
struct Slot {
    char *h = nullptr, *d = nullptr;
    size_t bytes = 0;
    hipEvent_t done = nullptr;
    bool used = false;
};

}  // namespace

struct ohs_delay2 {
    int device = 0;
    size_t n_streams = 0, max_objects = 0, max_delay = 0, R = 0;
    float *d_ring = nullptr;
    unsigned *d_counts = nullptr;
    size_t w = 0;                       // the ring's write position
    // the carry: (D, G, H[5]) of the previous call's last segment, [n_streams][carried_k]; carried_k == 0: nothing is carried
    std::vector<double> carry_d;
    std::vector<float> carry_g, carry_h;
    size_t carried_k = 0;
    Slot slots[kSlots];
    int next = 0;
    int last = -1;                      // the slot of the most recent call that queued work
    unsigned long long last_tiles = 0, last_filtered = 0;
    bool failed = false;
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
    return fail(e == hipErrorOutOfMemory ? OHS_DELAY2_ERR_ALLOC : OHS_DELAY2_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define DL_HIP(call)                                  \
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

constexpr size_t kTaps = ohs::DELAY2_TAPS;

// bytes of a call's staged rows: front_d [S][K], row_d [rows], then front_g [S][K], row_g [rows] and, in a filtered call,
// front_h [S][K][5], row_h [rows][5]
size_t staged_bytes(size_t S, size_t K, size_t rows, bool filtered)
{
    return (S * K + rows) * (sizeof(double) + sizeof(float) + (filtered ? kTaps * sizeof(float) : 0));
}

int slot_room(Slot &sl, size_t bytes)
{
    if (bytes <= sl.bytes) return OHS_DELAY2_OK;
    if (sl.d) (void)hipFree(sl.d);
    if (sl.h) (void)hipHostFree(sl.h);
    sl.d = sl.h = nullptr;
    sl.bytes = 0;
    DL_HIP(hipMalloc((void **)&sl.d, bytes));
    DL_HIP(hipHostMalloc((void **)&sl.h, bytes, hipHostMallocDefault));
    sl.bytes = bytes;
    return OHS_DELAY2_OK;
}

// One pass over n rows of five taps on their way into staging: copied, checked, and plain[i] set where row i is the identity by its
// bits.  -> n, or the index of the first tap that is not finite.  (The taps are five times the other rows' bytes: one read of them.)
size_t stage_taps(const float *src, float *dst, unsigned char *plain, size_t n)
{
    uint32_t any = 0;
    for (size_t i = 0; i < n; ++i) {
        uint32_t b[kTaps];
        std::memcpy(b, src + i * kTaps, sizeof(b));
        for (size_t j = 0; j < kTaps; ++j) any |= (b[j] & 0x7f800000u) == 0x7f800000u;
        plain[i] = b[0] == 0x3f800000u && !(b[1] | b[2] | b[3] | b[4]);
        std::memcpy(dst + i * kTaps, b, sizeof(b));
    }
    if (any)
        for (size_t i = 0; i < n * kTaps; ++i)
            if (!std::isfinite(src[i])) return i;
    return n * kTaps;
}

// the floats one buffer's processed region spans, or 0 when a stride is smaller than what it strides over
size_t region(size_t S, size_t K, size_t frames, size_t ss, size_t cs)
{
    if (cs < frames && K > 1) return 0;
    const size_t per_stream = (K - 1) * cs + frames;
    if (ss < per_stream && S > 1) return 0;
    return (S - 1) * ss + per_stream;
}

}  // namespace

extern "C" {

const char *ohs_delay2_status_string(int s)
{
    switch (s) {
    case OHS_DELAY2_OK: return "OHS_OK";
    case OHS_DELAY2_ERR_INVALID_ARG: return "OHS_ERR_INVALID_ARG";
    case OHS_DELAY2_ERR_NO_DEVICE: return "OHS_ERR_NO_DEVICE";
    case OHS_DELAY2_ERR_HIP: return "OHS_ERR_HIP";
    case OHS_DELAY2_ERR_ALLOC: return "OHS_ERR_ALLOC";
    default: return "OHS_ERR_UNKNOWN";
    }
}

const char *ohs_delay2_last_error(void) { return g_err.c_str(); }

int ohs_delay2_create(int device, size_t n_streams, size_t max_objects, size_t max_delay, ohs_delay2 **out)
{
    if (!out) return fail(OHS_DELAY2_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (n_streams < 1 || n_streams > OHS_DELAY2_MAX_STREAMS)
        return fail(OHS_DELAY2_ERR_INVALID_ARG, "n_streams " + std::to_string(n_streams) + " is outside 1 .. 65535");
    if (max_objects < 1 || max_objects > OHS_DELAY2_MAX_OBJECTS)
        return fail(OHS_DELAY2_ERR_INVALID_ARG, "max_objects " + std::to_string(max_objects) + " is outside 1 .. 64");
    if (max_delay < 1 || max_delay > OHS_DELAY2_MAX_DELAY)
        return fail(OHS_DELAY2_ERR_INVALID_ARG, "max_delay " + std::to_string(max_delay) + " is outside 1 .. 65536");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        return fail(OHS_DELAY2_ERR_NO_DEVICE, "no HIP device");
    }
    if (device < 0 || device >= count) return fail(OHS_DELAY2_ERR_NO_DEVICE, "device " + std::to_string(device) + " of " + std::to_string(count));
    DeviceGuard guard;
    if (!guard.set(device)) return fail(OHS_DELAY2_ERR_NO_DEVICE, "hipSetDevice failed");
    ohs_delay2 *dl = new (std::nothrow) ohs_delay2;
    if (!dl) return fail(OHS_DELAY2_ERR_ALLOC, "out of host memory");
    dl->device = device;
    dl->n_streams = n_streams, dl->max_objects = max_objects, dl->max_delay = max_delay, dl->R = max_delay + 2 + OHS_DELAY2_FIR_RADIUS;
    const size_t ring_bytes = n_streams * max_objects * dl->R * sizeof(float);
    hipError_t e = hipMalloc((void **)&dl->d_ring, ring_bytes);
    if (e == hipSuccess) e = hipMemset(dl->d_ring, 0, ring_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&dl->d_counts, ohs::DELAY2_COUNTERS * sizeof(unsigned));
    if (e == hipSuccess) e = hipMemset(dl->d_counts, 0, ohs::DELAY2_COUNTERS * sizeof(unsigned));
    int st = e == hipSuccess ? OHS_DELAY2_OK : hip_fail(e, "ohs_delay2_create");
    for (int i = 0; i < kSlots && st == OHS_DELAY2_OK; ++i) {
        e = hipEventCreateWithFlags(&dl->slots[i].done, hipEventDisableTiming);
        const size_t room = staged_bytes(n_streams, max_objects, n_streams * kSlotSegs * max_objects, true);
        st = e == hipSuccess ? slot_room(dl->slots[i], room < kSlotBytes ? room : kSlotBytes) : hip_fail(e, "hipEventCreateWithFlags");
    }
    if (st == OHS_DELAY2_OK) {
        e = hipDeviceSynchronize();
        if (e != hipSuccess) st = hip_fail(e, "ohs_delay2_create");
    }
    if (st != OHS_DELAY2_OK) {
        std::string keep = g_err;
        ohs_delay2_destroy(dl);
        g_err = keep;
        return st;
    }
    *out = dl;
    return OHS_DELAY2_OK;
}

void ohs_delay2_destroy(ohs_delay2 *dl)
{
    if (!dl) return;
    DeviceGuard guard;
    (void)guard.set(dl->device);
    for (Slot &sl : dl->slots) {
        if (sl.done && sl.used) (void)hipEventSynchronize(sl.done);
        if (sl.d) (void)hipFree(sl.d);
        if (sl.h) (void)hipHostFree(sl.h);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    if (dl->d_ring) (void)hipFree(dl->d_ring);
    if (dl->d_counts) (void)hipFree(dl->d_counts);
    delete dl;
}

// both calls: fir == NULL is ohs_delay2_process
static int process_rows(ohs_delay2 *dl, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride, size_t in_channel_stride,
                        size_t out_stream_stride, size_t out_channel_stride, size_t n_objects, size_t seg_blocks, const double *delay,
                        const float *gain, const float *fir, size_t row_stream_stride, int carry, void *hip_stream)
{
    if (!dl) return fail(OHS_DELAY2_ERR_INVALID_ARG, "delay handle is NULL");
    if (!d_in || !d_out) return fail(OHS_DELAY2_ERR_INVALID_ARG, "d_in or d_out is NULL");
    if (!delay) return fail(OHS_DELAY2_ERR_INVALID_ARG, "delay is NULL");
    if (dl->failed) return fail(OHS_DELAY2_ERR_HIP, "an earlier call failed in the middle: ohs_delay2_reset first");
    const size_t S = dl->n_streams, K = n_objects;
    if (K < 1 || K > dl->max_objects)
        return fail(OHS_DELAY2_ERR_INVALID_ARG, "n_objects " + std::to_string(K) + " is outside 1 .. max_objects " + std::to_string(dl->max_objects));
    if (seg_blocks == 0) return fail(OHS_DELAY2_ERR_INVALID_ARG, "seg_blocks is 0");
    if (n_blocks > (size_t(1) << 24)) return fail(OHS_DELAY2_ERR_INVALID_ARG, "n_blocks above 2^24");
    if (carry != OHS_DELAY2_FRESH && carry != OHS_DELAY2_CARRY) return fail(OHS_DELAY2_ERR_INVALID_ARG, "carry " + std::to_string(carry) + " is neither 0 nor 1");
    if (carry == OHS_DELAY2_CARRY && dl->carried_k == 0) return fail(OHS_DELAY2_ERR_INVALID_ARG, "carry = 1 on a handle that carries nothing");
    if (carry == OHS_DELAY2_CARRY && dl->carried_k != K)
        return fail(OHS_DELAY2_ERR_INVALID_ARG, "carry = 1 with n_objects " + std::to_string(K) + " behind a call of " + std::to_string(dl->carried_k));
    if (d_out == d_in) return fail(OHS_DELAY2_ERR_INVALID_ARG, "d_out == d_in: the stage does not work in place");
    if (n_blocks == 0) return OHS_DELAY2_OK;
    const size_t frames = n_blocks * 512, seg_frames = seg_blocks > n_blocks ? frames : seg_blocks * 512;
    const size_t n_segs = (frames + seg_frames - 1) / seg_frames;
    const size_t in_span = region(S, K, frames, in_stream_stride, in_channel_stride);
    const size_t out_span = region(S, K, frames, out_stream_stride, out_channel_stride);
    if (!in_span || !out_span) return fail(OHS_DELAY2_ERR_INVALID_ARG, "a stride is smaller than the region it strides over");
    if (d_in < d_out + out_span && d_out < d_in + in_span) return fail(OHS_DELAY2_ERR_INVALID_ARG, "the regions of d_in and d_out overlap");
    if (row_stream_stride != 0 && row_stream_stride < n_segs)
        return fail(OHS_DELAY2_ERR_INVALID_ARG, "row_stream_stride " + std::to_string(row_stream_stride) + " is neither 0 nor >= the " +
                                                   std::to_string(n_segs) + " segments");
    const size_t row_S = row_stream_stride ? S : 1, rows = row_S * n_segs * K;
    const double max_delay = (double)dl->max_delay;
    for (size_t s = 0; s < row_S; ++s)
        for (size_t i = 0; i < n_segs * K; ++i) {
            const size_t at = s * row_stream_stride * K + i;
            if (!(delay[at] >= 1.0 && delay[at] <= max_delay))         // (false for NaN)
                return fail(OHS_DELAY2_ERR_INVALID_ARG, "delay[" + std::to_string(at) + "] is not finite or outside [1, " + std::to_string(dl->max_delay) + "]");
            if (gain && !std::isfinite(gain[at])) return fail(OHS_DELAY2_ERR_INVALID_ARG, "gain[" + std::to_string(at) + "] is not finite");
            if (!fir) continue;
            if (delay[at] < (double)(1 + OHS_DELAY2_FIR_RADIUS))
                return fail(OHS_DELAY2_ERR_INVALID_ARG, "delay[" + std::to_string(at) + "] is below 1 + OHS_DELAY2_FIR_RADIUS = 5 in a filtered call");
        }
    if (fir && carry == OHS_DELAY2_CARRY)
        for (size_t i = 0; i < S * K; ++i)
            if (dl->carry_d[i] < (double)(1 + OHS_DELAY2_FIR_RADIUS))
                return fail(OHS_DELAY2_ERR_INVALID_ARG, "the carried delay of stream " + std::to_string(i / K) + ", object " + std::to_string(i % K) +
                                                            " is below 1 + OHS_DELAY2_FIR_RADIUS = 5 in a filtered call");
    DeviceGuard guard;
    if (!guard.set(dl->device)) return fail(OHS_DELAY2_ERR_HIP, "hipSetDevice failed");
    hipStream_t stream = (hipStream_t)hip_stream;
    Slot &sl = dl->slots[dl->next];
    if (sl.used) DL_HIP(hipEventSynchronize(sl.done));
    const size_t bytes = staged_bytes(S, K, rows, fir != nullptr);
    if (int st = slot_room(sl, bytes)) return st;
    // pack: front_d [S][K], row_d [row_S][n_segs][K], front_g, row_g, and in a filtered call front_h, row_h
    double *front_d = (double *)sl.h, *row_d = front_d + S * K;
    float *front_g = (float *)(row_d + rows), *row_g = front_g + S * K;
    float *front_h = row_g + rows, *row_h = front_h + S * K * kTaps;
    std::vector<unsigned char> plain(fir ? rows : 0);           // the staged row's taps are the identity
    for (size_t s = 0; s < row_S; ++s) {
        std::memcpy(row_d + s * n_segs * K, delay + s * row_stream_stride * K, n_segs * K * sizeof(double));
        if (gain)
            std::memcpy(row_g + s * n_segs * K, gain + s * row_stream_stride * K, n_segs * K * sizeof(float));
        else
            for (size_t i = 0; i < n_segs * K; ++i) row_g[s * n_segs * K + i] = 1.0f;
        if (fir) {      // (nothing is queued yet and the handle is as it was: a tap that is not finite is still refused here)
            const size_t from = s * row_stream_stride * K * kTaps;
            const size_t bad = stage_taps(fir + from, row_h + s * n_segs * K * kTaps, plain.data() + s * n_segs * K, n_segs * K);
            if (bad != n_segs * K * kTaps) return fail(OHS_DELAY2_ERR_INVALID_ARG, "fir[" + std::to_string(from + bad) + "] is not finite");
        }
    }
    for (size_t s = 0; s < S; ++s) {
        const size_t first = (row_stream_stride ? s : 0) * n_segs * K;
        if (carry == OHS_DELAY2_CARRY) {
            std::memcpy(front_d + s * K, dl->carry_d.data() + s * K, K * sizeof(double));
            std::memcpy(front_g + s * K, dl->carry_g.data() + s * K, K * sizeof(float));
            if (fir) std::memcpy(front_h + s * K * kTaps, dl->carry_h.data() + s * K * kTaps, K * kTaps * sizeof(float));
        } else {
            std::memcpy(front_d + s * K, row_d + first, K * sizeof(double));
            std::memcpy(front_g + s * K, row_g + first, K * sizeof(float));
            if (fir) std::memcpy(front_h + s * K * kTaps, row_h + first * kTaps, K * kTaps * sizeof(float));
        }
    }
    // the pass is the row's and depends on nothing but the staged taps: the filtered tiles are counted here
    unsigned long long filtered_tiles = 0;
    if (fir) {
        for (size_t k = 0; k < n_segs; ++k) {
            const size_t seg_len = k + 1 < n_segs ? seg_frames : frames - k * seg_frames;
            const size_t count_S = k && !row_stream_stride ? 1 : S;     // (shared rows behind the first segment: every stream as stream 0)
            unsigned long long n = 0;
            for (size_t s = 0; s < count_S; ++s) {
                const size_t base = ((row_stream_stride ? s : 0) * n_segs + k) * K;
                for (size_t c = 0; c < K; ++c)
                    n += !(plain[base + c] && (k ? plain[base - K + c] : ohs::delay2_identity(front_h + (s * K + c) * kTaps)));
            }
            filtered_tiles += n * (S / count_S) * (seg_len / ohs::DELAY2_TILE);
        }
    }
    ohs::Delay2Args a{};
    a.in = d_in, a.out = d_out;
    a.in_ss = in_stream_stride, a.in_cs = in_channel_stride, a.out_ss = out_stream_stride, a.out_cs = out_channel_stride;
    a.frames = frames, a.seg_frames = seg_frames, a.n_segs = n_segs;
    a.K = (unsigned)K, a.n_streams = (unsigned)S;
    a.front_d = (const double *)sl.d, a.row_d = a.front_d + S * K;
    a.front_g = (const float *)(a.row_d + rows), a.row_g = a.front_g + S * K;
    if (fir) a.front_h = a.row_g + rows, a.row_h = a.front_h + S * K * kTaps;
    a.row_ss = row_stream_stride ? n_segs : 0;
    a.max_delay = max_delay;
    a.ring = dl->d_ring, a.R = dl->R, a.w = dl->w, a.max_objects = (unsigned)dl->max_objects;
    a.silent = carry == OHS_DELAY2_FRESH;
    a.gather_tiles = dl->d_counts;
    hipError_t e = hipMemcpyAsync(sl.d, sl.h, bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemsetAsync(dl->d_counts, 0, ohs::DELAY2_COUNTERS * sizeof(unsigned), stream);
    if (e == hipSuccess) e = ohs::delay2_launch(a, stream);
    if (e == hipSuccess) e = hipEventRecord(sl.done, stream);
    if (e != hipSuccess) {      // some of the call may be queued: the history is no longer known
        (void)hipStreamSynchronize(stream);
        dl->failed = true;
        return hip_fail(e, "ohs_delay2_process");
    }
    sl.used = true;
    dl->last = dl->next;
    dl->next = (dl->next + 1) % kSlots;
    dl->last_tiles = (unsigned long long)(frames / ohs::DELAY2_TILE) * K * S;
    dl->last_filtered = filtered_tiles;
    dl->w = (dl->w + frames % dl->R) % dl->R;
    // what stands in front of the next call: the last segment's rows as given
    dl->carry_d.resize(S * K);
    dl->carry_g.resize(S * K);
    dl->carry_h.resize(S * K * kTaps);
    for (size_t s = 0; s < S; ++s) {
        const size_t lastrow = ((row_stream_stride ? s : 0) * n_segs + n_segs - 1) * K;
        std::memcpy(dl->carry_d.data() + s * K, row_d + lastrow, K * sizeof(double));
        std::memcpy(dl->carry_g.data() + s * K, row_g + lastrow, K * sizeof(float));
        if (fir)
            std::memcpy(dl->carry_h.data() + s * K * kTaps, row_h + lastrow * kTaps, K * kTaps * sizeof(float));
        else
            for (size_t i = 0; i < K * kTaps; ++i) dl->carry_h[s * K * kTaps + i] = i % kTaps ? 0.0f : 1.0f;     // the identity
    }
    dl->carried_k = K;
    return OHS_DELAY2_OK;
}

int ohs_delay2_process(ohs_delay2 *dl, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride, size_t in_channel_stride,
                       size_t out_stream_stride, size_t out_channel_stride, size_t n_objects, size_t seg_blocks, const double *delay,
                       const float *gain, size_t row_stream_stride, int carry, void *hip_stream)
{
    return process_rows(dl, d_in, d_out, n_blocks, in_stream_stride, in_channel_stride, out_stream_stride, out_channel_stride, n_objects,
                        seg_blocks, delay, gain, nullptr, row_stream_stride, carry, hip_stream);
}

int ohs_delay2_process_filtered(ohs_delay2 *dl, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                                size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride, size_t n_objects,
                                size_t seg_blocks, const double *delay, const float *gain, const float *fir, size_t row_stream_stride,
                                int carry, void *hip_stream)
{
    return process_rows(dl, d_in, d_out, n_blocks, in_stream_stride, in_channel_stride, out_stream_stride, out_channel_stride, n_objects,
                        seg_blocks, delay, gain, fir, row_stream_stride, carry, hip_stream);
}

int ohs_delay2_reset(ohs_delay2 *dl)
{
    if (!dl) return fail(OHS_DELAY2_ERR_INVALID_ARG, "delay handle is NULL");
    DeviceGuard guard;
    if (!guard.set(dl->device)) return fail(OHS_DELAY2_ERR_HIP, "hipSetDevice failed");
    DL_HIP(hipDeviceSynchronize());
    DL_HIP(hipMemset(dl->d_ring, 0, dl->n_streams * dl->max_objects * dl->R * sizeof(float)));
    DL_HIP(hipDeviceSynchronize());
    dl->w = 0;
    dl->carried_k = 0;
    dl->failed = false;
    return OHS_DELAY2_OK;
}

int ohs_delay2_sync(ohs_delay2 *dl, void *hip_stream)
{
    if (!dl) return fail(OHS_DELAY2_ERR_INVALID_ARG, "delay handle is NULL");
    DeviceGuard guard;
    if (!guard.set(dl->device)) return fail(OHS_DELAY2_ERR_HIP, "hipSetDevice failed");
    DL_HIP(hipStreamSynchronize((hipStream_t)hip_stream));
    return OHS_DELAY2_OK;
}

int ohs_delay2_last_launch(ohs_delay2 *dl, unsigned *tile_frames, unsigned *lds_window, unsigned long long *lds_tiles,
                           unsigned long long *gather_tiles, unsigned long long *filtered_tiles)
{
    if (!dl) return fail(OHS_DELAY2_ERR_INVALID_ARG, "delay handle is NULL");
    if (!tile_frames || !lds_window || !lds_tiles || !gather_tiles || !filtered_tiles) return fail(OHS_DELAY2_ERR_INVALID_ARG, "an out-parameter is NULL");
    unsigned long long gathered = 0;
    if (dl->last >= 0) {
        DeviceGuard guard;
        if (!guard.set(dl->device)) return fail(OHS_DELAY2_ERR_HIP, "hipSetDevice failed");
        unsigned counts[ohs::DELAY2_COUNTERS];
        DL_HIP(hipEventSynchronize(dl->slots[dl->last].done));
        DL_HIP(hipMemcpy(counts, dl->d_counts, sizeof(counts), hipMemcpyDeviceToHost));
        for (unsigned v : counts) gathered += v;
    }
    *tile_frames = ohs::DELAY2_TILE;
    *lds_window = ohs::DELAY2_LDS_WINDOW;
    *gather_tiles = gathered;
    *lds_tiles = dl->last_tiles - gathered;
    *filtered_tiles = dl->last_filtered;
    return OHS_DELAY2_OK;
}

int ohs_delay2_carried(const ohs_delay2 *dl, size_t *n_objects, double *delay, float *gain, float *fir)
{
    if (!dl) return fail(OHS_DELAY2_ERR_INVALID_ARG, "delay handle is NULL");
    if (!n_objects || !delay || !gain || !fir) return fail(OHS_DELAY2_ERR_INVALID_ARG, "an out-parameter is NULL");
    *n_objects = dl->carried_k;
    if (dl->carried_k) {
        std::memcpy(delay, dl->carry_d.data(), dl->n_streams * dl->carried_k * sizeof(double));
        std::memcpy(gain, dl->carry_g.data(), dl->n_streams * dl->carried_k * sizeof(float));
        std::memcpy(fir, dl->carry_h.data(), dl->n_streams * dl->carried_k * kTaps * sizeof(float));
    }
    return OHS_DELAY2_OK;
}

}  // extern "C"
