// api_tracked.hip -- ohs_tracked_* (include/ohs_tracked.h): the pruned lookup's passes (lookup3p_kernels.hip), k_scene_rows_seal
// (scene_rows_kernels.hip) and the three-direction scene kernel joined on the caller's stream, the rows never leaving the device.  The
// scene surface's shared bodies (api_scene_bodies.inc) are compiled under internal names and called by this library's own entries; the
// mesh is prepared as api_lookup3p.hip prepares it (lookup3p_body.hpp), the checks on the audio regions are batch_process_objects_any's
// (api_batch.hip), restated here: those units are frozen.  Linked into libohs_tracked.so only.
#include "api_internal.h"
#include "sched_rows.h"
#include "../../include/ohs_tracked.h"
#include "lookup3p_internal.h"
#include "lookup3p_body.hpp"
#include "scene_rows_internal.h"

using namespace ohs;
using namespace ohs_api;
using ohs_host::sched_segments;

static_assert(OHS_TRACKED_OK == OHS_OK && OHS_TRACKED_ERR_INVALID_ARG == OHS_ERR_INVALID_ARG && OHS_TRACKED_ERR_NO_DEVICE == OHS_ERR_NO_DEVICE &&
              OHS_TRACKED_ERR_HIP == OHS_ERR_HIP && OHS_TRACKED_ERR_ALLOC == OHS_ERR_ALLOC, "ohs_tracked.h restates ohs_hip.h's status codes");

// the scene surface's bodies, once more: the handle's batch object and the shims this library's setters go through (never exported)
#define OHS_SCENE_T ohsint_trk_scene
#define OHS_SCENE_FN(name) ohsint_trk_scene_##name
#define OHS_SCENE_OWN_LAST_LAUNCH 1
#include "api_scene_bodies.inc"

struct ohs_tracked {
    ohsint_trk_scene *sc = nullptr;     // owns the batch object
    int device = 0;
    // the mesh, as ohs_lookup3p keeps it: inverses, corners, the index over the sphere, the certificate's bound
    size_t n_dirs = 0, n_tris = 0, n_everywhere = 0;
    double *d_inv = nullptr;
    uint32_t *d_tris = nullptr, *d_cell_start = nullptr, *d_cell_tris = nullptr, *d_everywhere = nullptr;
    unsigned grid = 0;
    double bound = 0.0;
    uint32_t *d_rest = nullptr;         // pass 2's list of one chunk (the chunks follow each other on the stream)
    uint32_t *d_fallback = nullptr;     // one counter per chunk
    size_t fallback_cap = 0;
    unsigned long long *d_counts = nullptr;     // fading, blended, blended3
    // the rows: [6][plane], grown, never shrunk; the planes in front of a FRESH call; the carry, two buffers in turn, [6][S][64] each
    unsigned *d_rows = nullptr, *d_front = nullptr, *d_carry[2] = {nullptr, nullptr};
    size_t rows_cap = 0;
    int carry_cur = 0;                  // the buffer the next CARRY call reads
    size_t carry_K = 0;                 // 0: nothing carried
    // staging: sources, poses and gains through one of kSlots slots of pinned memory and its device copy (SchedLease's rule)
    static constexpr int kSlots = 4;
    struct Slot {
        char *h = nullptr, *d = nullptr;
        size_t cap = 0;
        hipEvent_t done = nullptr;
        bool in_use = false;
    } slot[kSlots];
    int slot_next = 0;
    // the most recent call that queued work
    hipEvent_t last_done = nullptr;
    bool have_last = false;
    size_t last_segs = 0, last_K = 0, last_chunks = 0;
};

namespace {

inline bool usable(double v) { return std::fabs(v) <= OHS_TRACKED_MAX_MAGNITUDE; }    // (false for NaN and the infinities)

// ohs_lookup3p_rows' two arrays (api_lookup3p.hip): entries of `elems` doubles at p[(s * stream_stride + k * seg_stride) * elems], shared
// across streams and / or segments where a stride is 0; packed, entry (s, k) is number s * a() + k * b()
struct RowSource {
    const double *p;
    size_t stream_stride, seg_stride, elems, n_segs;
    bool per_stream() const { return stream_stride != 0; }
    bool per_seg() const { return seg_stride != 0; }
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
    // every entry checked and, where `to` is given, packed into it
    bool pack(size_t n_streams, double *to) const
    {
        bool ok = true;
        for (size_t j = 0, n = entries(n_streams); j < n; ++j) {
            const double *e = entry(j);
            for (size_t i = 0; i < elems; ++i) ok &= usable(e[i]);
            if (to) std::memcpy(to + j * elems, e, elems * sizeof(double));
        }
        return ok;
    }
};

// api_batch.hip's layout_strides_ok / layout_regions_ok, restated
bool strides_ok(size_t n_outer, size_t outer, size_t n_inner, size_t inner, size_t frames)
{
    if (n_inner > 1 && inner < frames) return false;
    if (n_outer > 1 && outer < frames) return false;
    if (n_outer <= 1 || n_inner <= 1) return true;
    return outer >= (n_inner - 1) * inner + frames || inner >= (n_outer - 1) * outer + frames;
}

bool regions_ok(size_t S, size_t K, size_t frames, const float *d_in, size_t in_ss, size_t in_cs, const float *d_out, size_t out_ss, size_t out_cs)
{
    if (!strides_ok(S, in_ss, K, in_cs, frames) || !strides_ok(S, out_ss, 2, out_cs, frames)) {
        fail(OHS_ERR_INVALID_ARG, "strides smaller than the processed region");
        return false;
    }
    const float *in_end = d_in + (S - 1) * in_ss + (K - 1) * in_cs + frames;
    const float *out_end = d_out + (S - 1) * out_ss + out_cs + frames;
    if (!(in_end <= d_out || out_end <= d_in)) {
        fail(OHS_ERR_INVALID_ARG, "input and output regions overlap (the tracked call is out of place only)");
        return false;
    }
    return true;
}

// the next staging slot, free of its last user and with room for `bytes`; closed by the lease on every path out of the call
struct SlotLease {
    ohs_tracked::Slot *slot = nullptr;
    hipStream_t st = nullptr;
    SlotLease() = default;
    SlotLease(const SlotLease &) = delete;
    SlotLease &operator=(const SlotLease &) = delete;
    ~SlotLease()
    {
        if (!slot) return;
        if (hipEventRecord(slot->done, st) == hipSuccess) slot->in_use = true;
        else hipStreamSynchronize(st);
    }
};

int slot_lease(ohs_tracked *tr, size_t bytes, hipStream_t st, SlotLease &lease)
{
    ohs_tracked::Slot &slot = tr->slot[tr->slot_next];
    tr->slot_next = (tr->slot_next + 1) % ohs_tracked::kSlots;
    if (slot.in_use) HIP_TRY(hipEventSynchronize(slot.done));
    slot.in_use = false;
    if (!slot.done) HIP_TRY(hipEventCreateWithFlags(&slot.done, hipEventDisableTiming));
    lease.slot = &slot; lease.st = st;
    if (slot.cap < bytes) {
        if (slot.h) hipHostFree(slot.h);
        if (slot.d) {
            DeviceWideSection dws;
            hipFree(slot.d);
        }
        slot.h = nullptr; slot.d = nullptr; slot.cap = 0;
        const size_t cap = std::max<size_t>(8192, bytes + bytes / 2);
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&slot.h), cap, hipHostMallocDefault));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&slot.d), cap));
        slot.cap = cap;
    }
    return OHS_OK;
}

// room for six planes of `plane` entries and for `chunks` fallback counters (growing waits for the device: an earlier call may read them)
int ensure_rows(ohs_tracked *tr, size_t plane, size_t chunks)
{
    if (6 * plane > tr->rows_cap) {
        if (tr->d_rows) {
            DeviceWideSection dws;
            hipFree(tr->d_rows);
        }
        tr->d_rows = nullptr; tr->rows_cap = 0;
        tr->have_last = false;      // (the last call's planes went with the buffer; the call being made sets it again)
        const size_t cap = 6 * (plane + plane / 2);
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&tr->d_rows), cap * sizeof(unsigned)));
        tr->rows_cap = cap;
    }
    if (chunks > tr->fallback_cap) {
        if (tr->d_fallback) {
            DeviceWideSection dws;
            hipFree(tr->d_fallback);
        }
        tr->d_fallback = nullptr; tr->fallback_cap = 0;
        const size_t cap = std::max<size_t>(16, 2 * chunks);
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&tr->d_fallback), cap * sizeof(uint32_t)));
        tr->fallback_cap = cap;
    }
    return OHS_OK;
}

int tracked_null(const char *what) { return fail(OHS_ERR_INVALID_ARG, what); }

void release(ohs_tracked *tr)
{
    void *dev[] = {tr->d_inv, tr->d_tris, tr->d_cell_start, tr->d_cell_tris, tr->d_everywhere, tr->d_rest, tr->d_fallback, tr->d_counts,
                   tr->d_rows, tr->d_front, tr->d_carry[0], tr->d_carry[1]};
    for (void *p : dev)
        if (p) (void)hipFree(p);
    for (ohs_tracked::Slot &s : tr->slot) {
        if (s.h) (void)hipHostFree(s.h);
        if (s.d) (void)hipFree(s.d);
        if (s.done) (void)hipEventDestroy(s.done);
    }
    if (tr->last_done) (void)hipEventDestroy(tr->last_done);
}

}  // namespace

extern "C" {

const char *ohs_tracked_status_string(int status) { return ohs_status_string(status); }
const char *ohs_tracked_last_error(void) { return ohs_last_error(); }

int ohs_tracked_create(int device, size_t n_streams, size_t num_bands, size_t n_dirs, const float *xyz, size_t n_tris, const uint32_t *tris,
                       unsigned grid, ohs_tracked **out)
{
    if (!out) return fail(OHS_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    // the mesh: ohs_lookup3p_create's checks, in its words
    if (!xyz) return fail(OHS_ERR_INVALID_ARG, "xyz is NULL");
    if (!tris) return fail(OHS_ERR_INVALID_ARG, "tris is NULL");
    if (n_dirs < 1 || n_dirs > OHS_TRACKED_MAX_DIRECTIONS)
        return fail(OHS_ERR_INVALID_ARG, "n_dirs " + std::to_string(n_dirs) + " is outside 1 .. 65536");
    if (n_tris < 1 || n_tris > OHS_TRACKED_MAX_TRIANGLES)
        return fail(OHS_ERR_INVALID_ARG, "n_tris " + std::to_string(n_tris) + " is outside 1 .. 131072");
    if (grid > OHS_TRACKED_MAX_GRID) return fail(OHS_ERR_INVALID_ARG, "grid " + std::to_string(grid) + " is outside 0 .. 256");
    for (size_t i = 0; i < 3 * n_dirs; ++i)
        if (!std::isfinite(xyz[i])) return fail(OHS_ERR_INVALID_ARG, "xyz[" + std::to_string(i) + "] is not finite");
    for (size_t i = 0; i < 3 * n_tris; ++i)
        if (tris[i] >= n_dirs)
            return fail(OHS_ERR_INVALID_ARG, "triangle " + std::to_string(i / 3) + " names direction " + std::to_string(tris[i]) + " of " +
                                                 std::to_string(n_dirs));
    const unsigned IS = LOOKUP3P_INV_STRIDE;
    std::vector<double> inv;
    Lookup3pIndex ix;
    try {
        inv.assign(IS * n_tris, 0.0);
    } catch (const std::bad_alloc &) {
        return fail(OHS_ERR_ALLOC, "out of host memory");
    }
    for (size_t t = 0; t < n_tris; ++t) {
        double p[3][3];
        for (int c = 0; c < 3; ++c)
            for (int j = 0; j < 3; ++j) p[c][j] = (double)xyz[3 * (size_t)tris[3 * t + c] + j];
        if (!lookup3_inverse(p[0], p[1], p[2], &inv[IS * t]))
            return fail(OHS_ERR_INVALID_ARG, "triangle " + std::to_string(t) + " (" + std::to_string(tris[3 * t]) + ", " +
                                                 std::to_string(tris[3 * t + 1]) + ", " + std::to_string(tris[3 * t + 2]) +
                                                 ") is singular: its three directions lie in one plane through the origin");
    }
    ohs_tracked *tr = new (std::nothrow) ohs_tracked();
    if (!tr) return fail(OHS_ERR_ALLOC, "out of host memory");
    int rc = ohsint_trk_scene_create(device, n_streams, num_bands, &tr->sc);     // (the device's and the streams' checks; sets the device)
    if (rc) {
        delete tr;
        return rc;
    }
    tr->device = device;
    try {
        lookup3p_build_index(xyz, tris, n_tris, grid ? grid : lookup3p_choose_grid(n_tris), ix);
    } catch (const std::bad_alloc &) {
        ohs_tracked_destroy(tr);
        return fail(OHS_ERR_ALLOC, "out of host memory");
    }
    tr->n_dirs = n_dirs;
    tr->n_tris = n_tris;
    tr->grid = ix.G;
    tr->n_everywhere = ix.everywhere.size();
    tr->bound = lookup3p_bound(inv.data(), n_tris, IS);
    // (an empty list still gets a word, so that no pointer handed to the kernels is NULL)
    const size_t start_bytes = ix.cell_start.size() * 4, tris_bytes = ix.cell_tris.size() * 4, every_bytes = ix.everywhere.size() * 4;
    const size_t S = n_streams, carry_bytes = SCENE_ROWS_PLANES * S * OHS_TRACKED_MAX_OBJECTS * sizeof(unsigned);
    hipStream_t st = tr->sc->b->st;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc((void **)&tr->d_inv, IS * n_tris * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&tr->d_tris, 3 * n_tris * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&tr->d_cell_start, start_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&tr->d_cell_tris, tris_bytes + 4);
    if (e == hipSuccess) e = hipMalloc((void **)&tr->d_everywhere, every_bytes + 4);
    if (e == hipSuccess) e = hipMalloc((void **)&tr->d_rest, LOOKUP3P_CHUNK_QUERIES * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&tr->d_counts, 3 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void **)&tr->d_front, carry_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&tr->d_carry[0], carry_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&tr->d_carry[1], carry_bytes);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&tr->last_done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMemsetAsync(tr->d_counts, 0, 3 * sizeof(unsigned long long), st);
    if (e == hipSuccess) e = hipMemcpyAsync(tr->d_inv, inv.data(), IS * n_tris * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(tr->d_tris, tris, 3 * n_tris * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(tr->d_cell_start, ix.cell_start.data(), start_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && tris_bytes) e = hipMemcpyAsync(tr->d_cell_tris, ix.cell_tris.data(), tris_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && every_bytes) e = hipMemcpyAsync(tr->d_everywhere, ix.everywhere.data(), every_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        const std::string what = std::string("ohs_tracked_create: ") + hipGetErrorString(e);
        ohs_tracked_destroy(tr);
        return fail(e == hipErrorOutOfMemory ? OHS_ERR_ALLOC : OHS_ERR_HIP, what);
    }
    *out = tr;
    return OHS_OK;
}

void ohs_tracked_destroy(ohs_tracked *tr)
{
    if (!tr) return;
    (void)hipSetDevice(tr->device);
    {
        DeviceWideSection dws;
        (void)hipDeviceSynchronize();       // (whatever the handle has queued reads its buffers)
        release(tr);
    }
    ohsint_trk_scene_destroy(tr->sc);
    delete tr;
}

int ohs_tracked_set_direction_irs(ohs_tracked *tr, size_t n_dirs, const float *irs, size_t len)
{
    if (!tr) return tracked_null("tracked scene is NULL");
    return ohsint_trk_scene_set_direction_irs(tr->sc, n_dirs, irs, len);
}

int ohs_tracked_set_gain(ohs_tracked *tr, float gain)
{
    if (!tr) return tracked_null("tracked scene is NULL");
    return ohsint_trk_scene_set_gain(tr->sc, gain);
}

int ohs_tracked_set_eq_band_coeffs(ohs_tracked *tr, size_t band, const float coeffs[5], int enabled)
{
    if (!tr) return tracked_null("tracked scene is NULL");
    return ohsint_trk_scene_set_eq_band_coeffs(tr->sc, band, coeffs, enabled);
}

int ohs_tracked_set_eq_enabled(ohs_tracked *tr, int eq_enable)
{
    if (!tr) return tracked_null("tracked scene is NULL");
    return ohsint_trk_scene_set_eq_enabled(tr->sc, eq_enable);
}

int ohs_tracked_set_flush_denormals(ohs_tracked *tr, int mode)
{
    if (!tr) return tracked_null("tracked scene is NULL");
    return ohsint_trk_scene_set_flush_denormals(tr->sc, mode);
}

int ohs_tracked_reset(ohs_tracked *tr)
{
    if (!tr) return tracked_null("tracked scene is NULL");
    const int rc = ohsint_trk_scene_reset(tr->sc);
    if (rc == OHS_OK) tr->carry_K = 0;      // nothing stands in front of the next call
    return rc;
}

int ohs_tracked_sync(ohs_tracked *tr, void *hip_stream)
{
    if (!tr) return tracked_null("tracked scene is NULL");
    return ohsint_trk_scene_sync(tr->sc, hip_stream);
}

int ohs_tracked_process(ohs_tracked *tr, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride, size_t in_channel_stride,
                        size_t out_stream_stride, size_t out_channel_stride, size_t n_objects, size_t seg_blocks, const double *src,
                        size_t src_stream_stride, size_t src_seg_stride, const double *rot, size_t rot_stream_stride, const float *obj_gain,
                        int switch_mode, int carry, void *hip_stream)
{
    if (!tr) return tracked_null("tracked scene is NULL");
    if (!d_in || !d_out) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    if (!src) return fail(OHS_ERR_INVALID_ARG, "src is NULL");
    if (n_objects < 1 || n_objects > OHS_TRACKED_MAX_OBJECTS)
        return fail(OHS_ERR_INVALID_ARG, "n_objects " + std::to_string(n_objects) + " is outside 1 .. 64");
    if (seg_blocks == 0) return fail(OHS_ERR_INVALID_ARG, "seg_blocks is 0");
    if (switch_mode != OHS_TRACKED_SWITCH_RING_OUT && switch_mode != OHS_TRACKED_SWITCH_CROSSFADE)
        return fail(OHS_ERR_INVALID_ARG, "switch_mode must be OHS_TRACKED_SWITCH_RING_OUT or OHS_TRACKED_SWITCH_CROSSFADE");
    if (carry != OHS_TRACKED_FRESH && carry != OHS_TRACKED_CARRY) return fail(OHS_ERR_INVALID_ARG, "carry must be OHS_TRACKED_FRESH or OHS_TRACKED_CARRY");
    ohs_batch *b = tr->sc->b;
    ConvState &c = b->conv;
    if (c.obj_n == 0 || !c.d_obj_ah) return fail(OHS_ERR_INVALID_ARG, "no direction table uploaded (ohs_tracked_set_direction_irs)");
    if (c.obj_n < tr->n_dirs)
        return fail(OHS_ERR_INVALID_ARG, "the direction table has " + std::to_string(c.obj_n) + " rows, the mesh names " + std::to_string(tr->n_dirs) +
                                             " directions: a lookup result could lie outside the table");
    if (n_blocks > (size_t)1 << 24) return fail(OHS_ERR_INVALID_ARG, "n_blocks too large");
    const size_t K = n_objects, S = c.S;
    if (carry == OHS_TRACKED_CARRY && tr->carry_K == 0)
        return fail(OHS_ERR_INVALID_ARG, "OHS_TRACKED_CARRY, but the handle carries no rows (no call since create or ohs_tracked_reset)");
    if (carry == OHS_TRACKED_CARRY && tr->carry_K != K)
        return fail(OHS_ERR_INVALID_ARG, "OHS_TRACKED_CARRY with n_objects " + std::to_string(K) + ", but the carried rows hold " +
                                             std::to_string(tr->carry_K) + " objects");
    if (b->failed)
        return fail(OHS_ERR_HIP, "this tracked scene failed in the middle of an earlier call (" + b->fail_msg +
                                     "): its per-stream state is half-advanced; ohs_tracked_reset starts it afresh");
    if (n_blocks == 0) return OHS_OK;
    const size_t n_segs = sched_segments(n_blocks, &seg_blocks), frames = n_blocks * BS;
    if (6 * S * n_segs * K > (size_t)0x7fffffff) return fail(OHS_ERR_INVALID_ARG, "schedule too large");
    // ohs_lookup3p_rows' stride rules
    if (src_stream_stride != 0 && src_stream_stride < (n_segs - 1) * src_seg_stride + 1)
        return fail(OHS_ERR_INVALID_ARG, "src_stream_stride " + std::to_string(src_stream_stride) + " is neither 0 nor >= " +
                                             std::to_string((n_segs - 1) * src_seg_stride + 1) + ": streams' sources would overlap");
    if (rot && rot_stream_stride != 0 && rot_stream_stride < n_segs)
        return fail(OHS_ERR_INVALID_ARG, "rot_stream_stride " + std::to_string(rot_stream_stride) + " is neither 0 nor >= n_segs " +
                                             std::to_string(n_segs));
    if (!regions_ok(S, K, frames, d_in, in_stream_stride, in_channel_stride, d_out, out_stream_stride, out_channel_stride))
        return OHS_ERR_INVALID_ARG;
    const RowSource SR{src, src_stream_stride, src_seg_stride, 3 * K, n_segs};
    const RowSource RR{rot, rot_stream_stride, 1, 9, n_segs};
    // (checked before a staging slot is taken: a refused call leaves the ring as it was)
    if (!SR.pack(S, nullptr)) return fail(OHS_ERR_INVALID_ARG, "a source coordinate is not finite or above 1e15 in magnitude");
    if (rot && !RR.pack(S, nullptr)) return fail(OHS_ERR_INVALID_ARG, "a matrix element is not finite or above 1e15 in magnitude");
    const size_t plane = S * n_segs * K, Q = LOOKUP3P_CHUNK_QUERIES, chunks = (plane + Q - 1) / Q;
    const size_t src_bytes = SR.entries(S) * SR.elems * sizeof(double), rot_bytes = rot ? RR.entries(S) * RR.elems * sizeof(double) : 0;
    const size_t gain_bytes = obj_gain ? plane * sizeof(float) : 0;
    const bool fade = switch_mode == OHS_TRACKED_SWITCH_CROSSFADE, carried = carry == OHS_TRACKED_CARRY;

    HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = (hipStream_t)hip_stream;
    SlotLease lease;
    bool queued = false;
    auto body = [&]() -> int {
        int rc = ensure_rows(tr, plane, chunks);
        if (rc) return rc;
        rc = slot_lease(tr, src_bytes + rot_bytes + gain_bytes, st, lease);
        if (rc) return rc;
        char *h = lease.slot->h, *d = lease.slot->d;
        SR.pack(S, reinterpret_cast<double *>(h));
        if (rot) RR.pack(S, reinterpret_cast<double *>(h + src_bytes));
        if (obj_gain) std::memcpy(h + src_bytes + rot_bytes, obj_gain, gain_bytes);
        if (b->join_pending) {      // (a deferred call's last convolutions: the EQ state and d_out may be theirs)
            HIP_TRY(hipStreamWaitEvent(st, b->chunk_done[(size_t)b->chunk_done_n - 1], 0));
            b->join_pending = false;
        }
        queued = true;
        // 1. sources and poses up; the gains straight into the gain plane (1.0 where there are none)
        unsigned *rows = tr->d_rows;
        HIP_TRY(hipMemcpyAsync(d, h, src_bytes + rot_bytes, hipMemcpyHostToDevice, st));
        if (obj_gain)
            HIP_TRY(hipMemcpyAsync(rows + 5 * plane, h + src_bytes + rot_bytes, gain_bytes, hipMemcpyHostToDevice, st));
        else
            HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(rows + 5 * plane), 0x3f800000, plane, st));
        HIP_TRY(hipMemsetAsync(tr->d_fallback, 0, chunks * sizeof(uint32_t), st));
        HIP_TRY(hipMemsetAsync(tr->d_counts, 0, 3 * sizeof(unsigned long long), st));
        // 2. the lookup, chunk by chunk, its answers written where the convolution reads them
        for (size_t ch = 0; ch < chunks; ++ch) {
            const size_t at = ch * Q, nq = plane - at < Q ? plane - at : Q;
            Lookup3pArgs a{};
            a.inv = tr->d_inv; a.tris = tr->d_tris; a.n_tris = (uint32_t)tr->n_tris; a.n = (uint32_t)nq;
            a.cell_start = tr->d_cell_start; a.cell_tris = tr->d_cell_tris; a.everywhere = tr->d_everywhere;
            a.grid = tr->grid; a.n_everywhere = (uint32_t)tr->n_everywhere; a.bound = tr->bound;
            a.rest = tr->d_rest; a.rest_count = tr->d_fallback + ch;
            a.src = reinterpret_cast<const double *>(d);
            a.rot = rot ? reinterpret_cast<const double *>(d + src_bytes) : nullptr;
            a.g0 = at; a.n_segs = n_segs; a.K = (uint32_t)K;
            a.src_a = SR.a(); a.src_b = SR.b(); a.src_base = 0;
            a.rot_a = RR.a(); a.rot_base = 0;
            a.idx0 = rows + at; a.idx1 = rows + plane + at; a.idx2 = rows + 2 * plane + at;
            a.w1 = reinterpret_cast<float *>(rows + 3 * plane + at); a.w2 = reinterpret_cast<float *>(rows + 4 * plane + at);
            a.tri = nullptr;
            const hipError_t e = lookup3p_launch(a, st);
            if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("lookup3p launch: ") + hipGetErrorString(e));
        }
        // 3. the seal: the planes in front, the carry into the other buffer, the record
        const int next = tr->carry_cur ^ 1;
        SceneRowsArgs sa{};
        sa.rows = rows; sa.plane = plane; sa.n_streams = (unsigned)S; sa.n_segs = (unsigned)n_segs; sa.K = (unsigned)K;
        sa.carry_in = carried ? tr->d_carry[tr->carry_cur] : nullptr;
        sa.front_out = carried ? nullptr : tr->d_front;
        sa.carry_out = tr->d_carry[next];
        sa.fade = fade ? 1 : 0; sa.seg_blocks = (unsigned)seg_blocks; sa.n_blocks = (unsigned)n_blocks;
        sa.counts = tr->d_counts;
        const hipError_t e = scene_rows_launch(sa, st);
        if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("scene_rows_seal launch: ") + hipGetErrorString(e));
        // 4. the scene kernel on the planes, then the EQ, as batch_process_objects_any ends
        ConvObjectBlendRows br;
        br.rows = rows; br.plane = (int)plane; br.has_gain = true;
        if (fade) br.prev = carried ? tr->d_carry[tr->carry_cur] : tr->d_front;
        br.prev_plane = (int)(S * K);
        br.seg_blocks = (int)seg_blocks; br.stream_stride = (int)(n_segs * K); br.prev_stride = (int)K;
        br.fade = fade;
        rc = conv_launch_objects_blend(c, b->ctx, d_in, (long long)in_stream_stride, (long long)in_channel_stride, d_out,
                                       (long long)out_stream_stride, (long long)out_channel_stride, (int)n_blocks, b->gain, st, (int)K, 3, br);
        if (rc) return rc;
        tr->carry_cur = next; tr->carry_K = K;
        tr->last_segs = n_segs; tr->last_K = K; tr->last_chunks = chunks; tr->have_last = true;
        if (b->eq_enable && eq_any_enabled(b->eq))      // EQ(gain * conv(x)): the two ear channels, in place, behind the whole call
            rc = eq_launch(b->eq, d_out, d_out, (long long)out_stream_stride, (long long)out_channel_stride, (long long)frames, st);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(tr->last_done, st));
        return OHS_OK;
    };
    const int rc = body();
    if (rc == OHS_OK || !queued) return rc;
    // a HIP call failed with part of the call queued: refused until ohs_tracked_reset (batch_mark_failed's rule)
    const std::string why = g_err;
    b->failed = true;
    b->fail_msg = why;
    return fail(rc, why);
}

int ohs_tracked_last_launch(ohs_tracked *tr, int *n_pairs, int *ranges_per_stream, unsigned long long *fading_passes,
                            unsigned long long *blended_passes, unsigned long long *blended3_passes, unsigned long long *fallback_queries)
{
    if (!tr) return tracked_null("tracked scene is NULL");
    if (!n_pairs || !ranges_per_stream || !fading_passes || !blended_passes || !blended3_passes || !fallback_queries)
        return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    *n_pairs = *ranges_per_stream = 0;
    *fading_passes = *blended_passes = *blended3_passes = *fallback_queries = 0;
    if (!tr->have_last) return OHS_OK;
    const ohs_batch *b = tr->sc->b;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipEventSynchronize(tr->last_done));
    unsigned long long counts[3];
    std::vector<uint32_t> fb(tr->last_chunks);
    HIP_TRY(hipMemcpy(counts, tr->d_counts, sizeof counts, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(fb.data(), tr->d_fallback, fb.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *n_pairs = b->conv.last_obj_pairs;
    *ranges_per_stream = b->conv.last_obj_ranges;
    *fading_passes = counts[0];
    *blended_passes = counts[1];
    *blended3_passes = counts[2];
    for (uint32_t v : fb) *fallback_queries += v;
    return OHS_OK;
}

int ohs_tracked_rows(ohs_tracked *tr, uint32_t *idx0, uint32_t *idx1, uint32_t *idx2, float *w1, float *w2)
{
    if (!tr) return tracked_null("tracked scene is NULL");
    if (!idx0 || !idx1 || !idx2 || !w1 || !w2) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    if (!tr->have_last) return fail(OHS_ERR_INVALID_ARG, "no call has been made on this handle");
    const ohs_batch *b = tr->sc->b;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipEventSynchronize(tr->last_done));
    const size_t plane = b->conv.S * tr->last_segs * tr->last_K;
    void *const to[5] = {idx0, idx1, idx2, w1, w2};
    for (int pl = 0; pl < 5; ++pl) HIP_TRY(hipMemcpy(to[pl], tr->d_rows + pl * plane, plane * sizeof(unsigned), hipMemcpyDeviceToHost));
    return OHS_OK;
}

}  // extern "C"
