// api_batch.hip -- ohs_batch_*: S independent streams sharing the four impulse responses and the EQ table (the offline
// many-stream job of BASELINE.json's north_star): EQ || convolution over time chunks on two streams, the deferred form,
// the PCIe-fed host pipeline, per-kernel profiling, fail-closed error handling.
#include "api_internal.h"
#include "sched_rows.h"

using namespace ohs;
using namespace ohs_api;
using ohs_host::rbj;
using ohs_host::sched_row_constant;
using ohs_host::sched_rows_equal;
using ohs_host::sched_segments;

extern "C" {

// ---- batch -----------------------------------------------------------------------------
int ohs_batch_create(int device, size_t n_streams, size_t num_bands, ohs_batch **out)
{
    if (!out) return fail(OHS_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (n_streams == 0 || n_streams > (1u << 20)) return fail(OHS_ERR_INVALID_ARG, "n_streams out of range");
    DeviceCtx *ctx = nullptr;
    int rc = get_ctx(device, &ctx);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    ohs_batch *b = new (std::nothrow) ohs_batch();
    if (!b) return fail(OHS_ERR_ALLOC, "out of host memory");
    b->device = device; b->ctx = ctx;
    if (hipStreamCreateWithFlags(&b->st, hipStreamNonBlocking) != hipSuccess) {
        delete b;
        return fail(OHS_ERR_HIP, "hipStreamCreate failed");
    }
    {
        hipError_t se = hipErrorUnknown;
        const Tuning &tn = tuning();
        if (!tn.conv_cu_mask.empty()) {      // (experiments: the overlapped convolution's stream confined to a CU set)
            se = hipExtStreamCreateWithCUMask(&b->st2, (uint32_t)tn.conv_cu_mask.size(), tn.conv_cu_mask.data());
            if (se != hipSuccess) fprintf(stderr, "[ohs] conv_cu_mask ignored: %s\n", hipGetErrorString(se));
        }
        if (se != hipSuccess) se = hipStreamCreateWithFlags(&b->st2, hipStreamNonBlocking);
        if (se != hipSuccess) {
            hipStreamDestroy(b->st);
            delete b;
            return fail(OHS_ERR_HIP, "hipStreamCreate failed");
        }
        // EQ || convolution overlap policy.  An EQ wave saturates the vector unit of its SIMD (every instruction of
        // the ring form is a 4-cycle DPP / packed operation: two EQ waves on one SIMD take 1.82x the time of one,
        // four 3.47x -- profiles/r03_eq_share.txt), so the convolution only makes progress on CUs that host no EQ
        // wave; from one EQ wave per SIMD on (almost) every CU upwards the two kernels merely get in each other's
        // way (2048 streams: 13.7-16.1 ms overlapped, 11.5 ms one after the other).  Overlap while at least an
        // eighth of the CUs stays free of EQ waves, serialise beyond.
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
        const size_t eq_waves = (2 * n_streams + 3) / 4;            // 4 chains per wave
        const size_t eq_cus = (eq_waves + 3) / 4;                   // one wave per SIMD once there is a wave per CU
        b->overlap = eq_cus * 8 <= (size_t)cus * 7;
        if (tn.no_overlap) b->overlap = false;
        if (tn.force_overlap) b->overlap = true;
        b->xcd_split = tn.xcd_split;        // (experiments: EQ launches on XCDs [0, x), overlapped convolution on [x, 8))
    }
    rc = conv_init(b->conv, n_streams, b->st);
    if (rc == OHS_OK) rc = conv_enable_lazy_state(b->conv);
    if (rc == OHS_OK) rc = eq_init(b->eq, num_bands, 2 * n_streams, 48000.0f, b->st);
    if (rc == OHS_OK && hipStreamSynchronize(b->st) != hipSuccess) rc = fail(OHS_ERR_HIP, "sync failed");
    if (rc) { ohs_batch_destroy(b); return rc; }
    *out = b;
    return OHS_OK;
}

void ohs_batch_destroy(ohs_batch *b)
{
    if (!b) return;
    hipSetDevice(b->device);
    DeviceWideSection dws;
    hipDeviceSynchronize();
    conv_free(b->conv);
    eq_free(b->eq);
    for (auto &sp : b->spans) { hipEventDestroy(sp.a); hipEventDestroy(sp.b); }
    for (hipEvent_t e : b->ev_pool) hipEventDestroy(e);
    for (hipEvent_t e : b->ev_inflight) hipEventDestroy(e);
    for (hipEvent_t e : b->chunk_done) hipEventDestroy(e);
    for (auto &sl : b->sched_slot) {
        if (sl.h) hipHostFree(sl.h);
        if (sl.d) hipFree(sl.d);
        if (sl.done) hipEventDestroy(sl.done);
    }
    for (int k = 0; k < ohs_batch::kHostSlots; ++k) {
        if (b->d_slot[k]) hipFree(b->d_slot[k]);
        if (b->ev_h2d[k]) hipEventDestroy(b->ev_h2d[k]);
        if (b->ev_comp[k]) hipEventDestroy(b->ev_comp[k]);
        if (b->ev_d2h[k]) hipEventDestroy(b->ev_d2h[k]);
    }
    if (b->st_h2d) hipStreamDestroy(b->st_h2d);
    if (b->st_comp) hipStreamDestroy(b->st_comp);
    if (b->st_d2h) hipStreamDestroy(b->st_d2h);
    if (b->st2) hipStreamDestroy(b->st2);
    if (b->st) hipStreamDestroy(b->st);
    delete b;
}

int ohs_batch_set_ir(ohs_batch *b, int path, const float *ir, size_t len)
{
    if (!b) return fail(OHS_ERR_INVALID_ARG, "batch is NULL");
    HIP_TRY(hipSetDevice(b->device));
    DeviceWideSection dws;
    HIP_TRY(hipDeviceSynchronize());
    return conv_set_ir(b->conv, b->ctx, path, ir, len, b->st);
}

// node_batch.cpp: the same with the IR already on the batch's device (a broadcast buffer)
extern "C" int ohsint_batch_set_ir_device(ohs_batch *b, int path, const float *d_ir, size_t len)
{
    if (!b) return fail(OHS_ERR_INVALID_ARG, "batch is NULL");
    HIP_TRY(hipSetDevice(b->device));
    DeviceWideSection dws;
    HIP_TRY(hipDeviceSynchronize());
    return conv_set_ir(b->conv, b->ctx, path, d_ir, len, b->st, true);
}

int ohs_batch_set_eq_band_coeffs(ohs_batch *b, size_t band, const float coeffs[5], int enabled)
{
    if (!b || !coeffs) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    if (band >= b->eq.nb) return OHS_OK;
    eq_set_shared_band(b->eq, band, coeffs, enabled);
    return OHS_OK;
}

int ohs_batch_set_stream_eq_band_coeffs(ohs_batch *b, size_t stream, size_t band, const float coeffs[5], int enabled)
{
    if (!b || !coeffs) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    return eq_set_stream_band(b->eq, stream, band, coeffs, enabled);
}

int ohs_batch_update_stream_eq_band(ohs_batch *b, size_t stream, size_t band, float fs, int filter_type, float fc, float q,
                                    float gain_db, int enabled)
{
    if (!b) return fail(OHS_ERR_INVALID_ARG, "batch is NULL");
    if (stream >= b->conv.S) return fail(OHS_ERR_INVALID_ARG, "stream index out of range");
    if (band >= b->eq.nb) return OHS_OK;
    float c[5];
    int rc = rbj(filter_type, fs, fc, q, gain_db, c);
    if (rc) return rc;
    return eq_set_stream_band(b->eq, stream, band, c, enabled);
}

int ohs_batch_share_eq_table(ohs_batch *b)
{
    if (!b) return fail(OHS_ERR_INVALID_ARG, "batch is NULL");
    eq_share_table(b->eq);
    return OHS_OK;
}

int ohs_batch_update_eq_band(ohs_batch *b, size_t band, float fs, int filter_type, float fc, float q,
                             float gain_db, int enabled)
{
    if (!b) return fail(OHS_ERR_INVALID_ARG, "batch is NULL");
    if (band >= b->eq.nb) return OHS_OK;
    float c[5];
    int rc = rbj(filter_type, fs, fc, q, gain_db, c);
    if (rc) return rc;
    eq_set_shared_band(b->eq, band, c, enabled);
    return OHS_OK;
}

int ohs_batch_set_eq_enabled(ohs_batch *b, int eq_enable)
{
    if (!b) return fail(OHS_ERR_INVALID_ARG, "batch is NULL");
    b->eq_enable = eq_enable != 0;
    return OHS_OK;
}

int ohs_batch_set_flush_denormals(ohs_batch *b, int mode)
{
    if (!b) return fail(OHS_ERR_INVALID_ARG, "batch is NULL");
    if (mode < 0 || mode > 2) return fail(OHS_ERR_INVALID_ARG, "mode must be 0 (IEEE), 1 (FTZ) or 2 (FTZ | DAZ)");
    b->conv.fp_mode = mode;
    b->eq.fp_mode = mode;
    return OHS_OK;
}

int ohs_batch_set_eq_exact_specials(ohs_batch *b, int enable)
{
    if (!b) return fail(OHS_ERR_INVALID_ARG, "batch is NULL");
    b->eq.exact_specials = enable != 0;
    return OHS_OK;
}

int ohs_batch_set_conv_plan(ohs_batch *b, int plan)
{
    if (!b) return fail(OHS_ERR_INVALID_ARG, "batch is NULL");
    if (plan < 0 || plan > 2)
        return fail(OHS_ERR_INVALID_ARG, "plan must be 0 (library's choice), 1 (block 512) or 2 (large transforms: hop 1536 / block 2048)");
    b->conv.conv_plan = plan;
    return OHS_OK;
}

int ohs_batch_last_conv_plan(const ohs_batch *b, int *kernel, int *ranges_per_stream)
{
    if (!b || !kernel || !ranges_per_stream) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    *kernel = b->conv.last_kernel;
    *ranges_per_stream = b->conv.last_ranges;
    return OHS_OK;
}

int ohs_batch_conv_plan_counts(ohs_batch *b, uint64_t counts[OHS_CONV_KERNEL_COUNT], int reset)
{
    if (!b || !counts) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    for (int k = 0; k < OHS_CONV_KERNEL_COUNT; ++k) counts[k] = b->conv.kernel_calls[k];
    if (reset)
        for (int k = 0; k < OHS_CONV_KERNEL_COUNT; ++k) b->conv.kernel_calls[k] = 0;
    return OHS_OK;
}

int ohs_batch_set_gain(ohs_batch *b, float gain)
{
    if (!b) return fail(OHS_ERR_INVALID_ARG, "batch is NULL");
    b->gain = gain;
    return OHS_OK;
}

int ohs_batch_reset(ohs_batch *b)
{
    if (!b) return fail(OHS_ERR_INVALID_ARG, "batch is NULL");
    HIP_TRY(hipSetDevice(b->device));
    DeviceWideSection dws;
    HIP_TRY(hipDeviceSynchronize());
    ConvState &c = b->conv;
    HIP_TRY(hipMemsetAsync(c.d_hist, 0, c.S * (size_t)c.cap * NF * sizeof(float2), b->st));
    HIP_TRY(hipMemsetAsync(c.d_tails, 0, c.S * 2 * 8 * 64 * sizeof(float2), b->st));
    c.tails_lazy = false; c.tails_both = false;     // (the zeroed per-path overlaps are the state)
    c.lb_lazy = false; c.lb_valid = 0;
    c.pt_active = false;        // (pending tails belong to the frames in front of the reset)
    if (c.d_xhist) {            // (the block-2048 plan's state: zeros are what every path may see of the past)
        HIP_TRY(hipMemsetAsync(c.d_xhist, 0, c.S * 2 * (size_t)(2 * c.xh_len) * sizeof(float), b->st));
        c.xh_valid = c.xh_len;
        c.xh_head = 0;
    }
    c.cnt = 0;
    for (int p = 0; p < 4; ++p) c.since[p] = 0;
    if (c.d_lay_ov) HIP_TRY(hipMemsetAsync(c.d_lay_ov, 0, c.S * 8 * 64 * sizeof(float2), b->st));     // (the layout's overlap)
    int rc = eq_reset(b->eq, b->st);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(b->st));
    b->failed = false;          // (zeroed state is consistent state)
    b->fail_msg.clear();
    return OHS_OK;
}

// ---- what the processing entry points share -----------------------------------------------------------------------
// [S][2][frames] fits its strides: the channels inside a stream's stride, or the streams inside a channel's
static bool batch_strides_ok(size_t S, size_t ss, size_t cs, size_t frames)
{
    return cs >= frames && (S <= 1 || ss >= 2 * frames || ss >= cs + frames);
}

static int batch_refuse_failed(const ohs_batch *b)
{
    return fail(OHS_ERR_HIP, "this batch failed in the middle of an earlier call (" + b->fail_msg +
                                 "): its per-stream state is half-advanced; ohs_batch_reset starts it afresh");
}

// A HIP call failed (rc, its message in g_err) with part of a processing call queued: some of the work has advanced the per-stream
// state, the rest has not.  Every later processing call is refused until ohs_batch_reset.
static int batch_mark_failed(ohs_batch *b, int rc)
{
    const std::string why = g_err;
    b->failed = true;
    b->fail_msg = why;
    return fail(rc, why);
}

// the handle's EQ table becomes schedule table t (what the setters do)
static void batch_adopt_table(ohs_batch *b, size_t t)
{
    for (size_t band = 0; band < b->eq.nb; ++band)
        eq_set_shared_band(b->eq, band, &b->eq.sched_coeffs[(t * b->eq.nb + band) * 5], b->eq.sched_en[t * b->eq.nb + band]);
}

static int batch_process_body(ohs_batch *b, const float *d_in, float *d_out, size_t n_blocks,
                              size_t stream_stride, size_t channel_stride, void *hip_stream, bool deferred,
                              const BatchSchedule *sc, const ConvIrs *irs);

// sc (optional): the schedule of ohs_batch_process_scheduled, its device copies already queued on hip_stream
// irs (optional): the rows of ohs_batch_process_ir_scheduled, likewise
static int batch_process_impl(ohs_batch *b, const float *d_in, float *d_out, size_t n_blocks,
                              size_t stream_stride, size_t channel_stride, void *hip_stream, bool deferred,
                              const BatchSchedule *sc = nullptr, const ConvIrs *irs = nullptr)
{
    if (!b || !d_in || !d_out) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    if (b->failed) return batch_refuse_failed(b);
    const size_t spans_before = b->spans.size();
    const int rc = batch_process_body(b, d_in, d_out, n_blocks, stream_stride, channel_stride, hip_stream, deferred, sc, irs);
    if (rc == OHS_OK || rc == OHS_ERR_INVALID_ARG) return rc;      // (argument errors are found before anything is queued)
    // A HIP call failed with part of the work queued.  Leave nothing dangling (none of this touches the message):
    //  * the caller's stream must not run ahead of what this call put on the second stream
    hipStream_t st = (hipStream_t)hip_stream;
    hipEvent_t ev = nullptr;
    // (a timing-enabled event: ev_inflight feeds ev_pool, whose events the profiling spans time with)
    if (hipEventCreate(&ev) == hipSuccess) {
        if (hipEventRecord(ev, b->st2) != hipSuccess || hipStreamWaitEvent(st, ev, 0) != hipSuccess)
            hipStreamSynchronize(b->st2);
        b->ev_inflight.push_back(ev);
    } else {
        hipStreamSynchronize(b->st2);
    }
    b->join_pending = false;
    //  * timing spans opened by this call may hold events that were never recorded: drop them
    while (b->spans.size() > spans_before) {
        ohs_batch::Span sp = b->spans.back();
        b->spans.pop_back();
        if (sp.a) hipEventDestroy(sp.a);
        if (sp.b) hipEventDestroy(sp.b);
    }
    //  * some time chunks have advanced the per-stream state, others have not
    return batch_mark_failed(b, rc);
}

static int batch_process_body(ohs_batch *b, const float *d_in, float *d_out, size_t n_blocks,
                              size_t stream_stride, size_t channel_stride, void *hip_stream, bool deferred,
                              const BatchSchedule *sc, const ConvIrs *irs)
{
    if (n_blocks == 0) return OHS_OK;
    if (n_blocks > (size_t)1 << 24) return fail(OHS_ERR_INVALID_ARG, "n_blocks too large");
    if (!batch_strides_ok(b->conv.S, stream_stride, channel_stride, n_blocks * BS))
        return fail(OHS_ERR_INVALID_ARG, "strides smaller than the processed region");
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = (hipStream_t)hip_stream;
    auto get_event = [&](hipEvent_t *e) -> int {
        if (!b->ev_pool.empty()) { *e = b->ev_pool.back(); b->ev_pool.pop_back(); return OHS_OK; }
        HIP_TRY(hipEventCreate(e));
        return OHS_OK;
    };
    // ordering events of earlier calls that have completed go back to the pool
    for (size_t i = 0; i < b->ev_inflight.size();) {
        if (hipEventQuery(b->ev_inflight[i]) == hipSuccess) {
            b->ev_pool.push_back(b->ev_inflight[i]);
            b->ev_inflight[i] = b->ev_inflight.back();
            b->ev_inflight.pop_back();
        } else ++i;
    }
    auto span_begin = [&](hipStream_t s_, int kind) -> int {
        if (!b->profiling) return OHS_OK;
        ohs_batch::Span sp; sp.kind = kind; sp.a = nullptr; sp.b = nullptr;
        int rc = get_event(&sp.a); if (rc) return rc;
        rc = get_event(&sp.b); if (rc) return rc;
        HIP_TRY(hipEventRecord(sp.a, s_));
        b->spans.push_back(sp);
        return OHS_OK;
    };
    auto span_end = [&](hipStream_t s_) -> int {
        if (!b->profiling) return OHS_OK;
        HIP_TRY(hipEventRecord(b->spans.back().b, s_));
        return OHS_OK;
    };
    if (b->profiling) b->prof_calls++;

    // a schedule of tables: the EQ runs if any segment's table has a band enabled; a schedule of gains: every convolution launch
    // gets the table and where its first block lies in the call
    const bool sched_tabs = sc != nullptr && sc->tab != nullptr;
    bool eq_active = b->eq_enable && eq_any_enabled(b->eq);
    if (sched_tabs) {
        eq_active = false;
        const size_t rows = sc->tab_stride ? b->conv.S : 1;
        for (size_t r = 0; r < rows && b->eq_enable && !eq_active; ++r)
            for (size_t k = 0; k < sc->n_segs && !eq_active; ++k)
                eq_active = eq_schedule_table_any_enabled(b->eq, sc->tab[r * sc->tab_stride + k]);
    }
    ConvGains cg;
    if (sc && sc->d_gain) { cg.tab = sc->d_gain; cg.seg_blocks = (int)sc->seg_blocks; cg.stream_stride = (int)sc->gain_stride; }
    ConvIrs ci;         // (every convolution launch is told where its first block lies in the call, as for the gains)
    if (irs) ci = *irs;

    const long long ss = (long long)stream_stride, cs = (long long)channel_stride;
    int rc;
    // A deferred call may have left convolutions running on st2.  If this call repeats its geometry and
    // overlaps again, EQ chunk c only has to wait for THAT call's convolution of chunk c (same frames of
    // d_out); anything else joins completely first.
    const bool will_overlap = eq_active && b->overlap && n_blocks >= 64;
    bool chunk_waits = false;
    if (b->join_pending) {
        chunk_waits = will_overlap && b->pend_out == d_out && b->pend_blocks == n_blocks &&
                      b->pend_ss == stream_stride && b->pend_cs == channel_stride;
        if (!chunk_waits) {
            HIP_TRY(hipStreamWaitEvent(st, b->chunk_done[(size_t)b->chunk_done_n - 1], 0));
            b->join_pending = false;
        }
    }
    if (!eq_active) {     // lib.rs:1179 eq_enable false (or every band disabled: identity)
#ifdef OHS_EXPERIMENTS
        if (g_inject_batch_failure.load() > 0 && g_inject_batch_failure.fetch_sub(1) == 1)
            return fail(OHS_ERR_HIP, "injected failure (ohs_debug_inject_batch_failure)");
#endif
        rc = span_begin(st, 1); if (rc) return rc;
        rc = conv_launch(b->conv, b->ctx, d_in, ss, cs, d_out, ss, cs, (int)n_blocks, b->gain, st, true, nullptr, nullptr, &cg, &ci);
        if (rc) return rc;
        return span_end(st);
    }
    // The EQ is a serial recurrence (latency-bound, ~128 waves at 256 streams) and leaves most of the
    // chip idle, so the convolution of time chunk i runs on a second stream underneath the EQ of
    // chunk i+1.  Chunks touch disjoint frame ranges; state (EQ s1/s2, overlaps) chains per stream.
    // Uneven chunks: only the LAST chunk's convolution is not hidden under an EQ launch, so it is short
    // (2 % of the frames; six chunks measure 6.00-6.02 ms per headline step, the four of {0.34, 0.66, 0.92} 6.05,
    // seven 6.03-6.04: every extra EQ launch costs its ramp).
    const std::vector<double> &kCut = tuning().overlap_cuts;
    const int nch = (b->overlap && n_blocks >= 64) ? (int)kCut.size() - 1 : 1;
    // XCD partition of the overlapped launches: the EQ on XCDs [0, x), the convolution on [x, 8)
    struct XcdScope {
        ohs_batch *b;
        XcdScope(ohs_batch *b_, int x) : b(b_)
        {
            if (x > 0 && x < 8) { b->eq.xcd_lo = 0; b->eq.xcd_n = x; b->conv.xcd_lo = x; b->conv.xcd_n = 8 - x; }
        }
        ~XcdScope() { b->eq.xcd_lo = 0; b->eq.xcd_n = 8; b->conv.xcd_lo = 0; b->conv.xcd_n = 8; }
    } xcd_scope(b, nch > 1 ? b->xcd_split : 0);
    bool joined = false;        // the last convolution ran on the caller's stream: nothing left to join
    for (int i = 0; i < nch; ++i) {
        const size_t blk0 = nch == 1 ? 0 : (size_t)(kCut[i] * (double)n_blocks);
        const size_t blk1 = nch == 1 ? n_blocks : (i == nch - 1 ? n_blocks : (size_t)(kCut[i + 1] * (double)n_blocks));
        const size_t off = blk0 * BS;
        const int nb_i = (int)(blk1 - blk0);
        if (nb_i <= 0) {
            // two cut points truncated to the same block (OHS_OVERLAP_CUTS experiments): an empty chunk.
            // Its "done" event is recorded all the same so that a later deferred call's per-chunk wait
            // finds every event of this call on st2.
            if (nch > 1 && deferred) {
                while (b->chunk_done.size() <= (size_t)i) {
                    hipEvent_t ev;
                    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
                    b->chunk_done.push_back(ev);
                }
                HIP_TRY(hipEventRecord(b->chunk_done[(size_t)i], b->st2));
            }
            continue;
        }
        if (chunk_waits) HIP_TRY(hipStreamWaitEvent(st, b->chunk_done[(size_t)i], 0));
#ifdef OHS_EXPERIMENTS
        if (g_inject_batch_failure.load() > 0 && g_inject_batch_failure.fetch_sub(1) == 1)
            return fail(OHS_ERR_HIP, "injected failure (ohs_debug_inject_batch_failure)");
#endif
        // The EQ launch carries its own events (start / completion of the dispatch: no marker packets between the
        // back-to-back EQ launches of a step); the completion event is what the convolution's stream waits for.
        hipEvent_t ev_a = nullptr, ev_b = nullptr;
        if (b->profiling) {
            ohs_batch::Span sp; sp.kind = 0; sp.a = nullptr; sp.b = nullptr;
            rc = get_event(&sp.a); if (rc) return rc;
            rc = get_event(&sp.b); if (rc) return rc;
            b->spans.push_back(sp);
            ev_a = sp.a; ev_b = sp.b;
        } else if (nch > 1) {
            rc = get_event(&ev_b); if (rc) return rc;
            b->ev_inflight.push_back(ev_b);
        }
        // (the time chunks cut at block positions that need not be segment boundaries: every launch is told where it starts)
        if (sched_tabs && sc->streams)
            rc = eq_launch_scheduled_streams(b->eq, *sc, blk0, (size_t)nb_i, d_in + off, d_out + off, ss, cs, st, ev_a, ev_b);
        else if (sched_tabs) rc = eq_launch_scheduled(b->eq, *sc, blk0, (size_t)nb_i, d_in + off, d_out + off, ss, cs, st, ev_a, ev_b);
        else rc = eq_launch(b->eq, d_in + off, d_out + off, ss, cs, (long long)nb_i * BS, st, nullptr, ev_a, ev_b);
        if (rc) return rc;
        hipStream_t cst = st;
        // The LAST chunk's convolution has nothing to hide under: it runs on the caller's stream right behind its EQ
        // launch (after the earlier convolutions on st2, whose state it continues), which spares the step the hop to
        // st2 and the join back -- two cross-stream waits of 10-25 us each in front of the caller's next launch.
        const bool tail_on_caller = nch > 1 && !deferred && i == nch - 1;
        if (tail_on_caller) {
            hipEvent_t ev;
            rc = get_event(&ev); if (rc) return rc;
            HIP_TRY(hipEventRecord(ev, b->st2));
            HIP_TRY(hipStreamWaitEvent(st, ev, 0));
            b->ev_inflight.push_back(ev);
            joined = true;
        } else if (nch > 1) {
            HIP_TRY(hipStreamWaitEvent(b->st2, ev_b, 0));
            cst = b->st2;
        }
        {
            hipEvent_t cv_a = nullptr, cv_b = nullptr;
            if (b->profiling) {
                ohs_batch::Span sp; sp.kind = 1; sp.a = nullptr; sp.b = nullptr;
                rc = get_event(&sp.a); if (rc) return rc;
                rc = get_event(&sp.b); if (rc) return rc;
                b->spans.push_back(sp);
                cv_a = sp.a; cv_b = sp.b;
            }
            cg.blk_off = (int)blk0; ci.blk_off = (int)blk0;
            rc = conv_launch(b->conv, b->ctx, d_out + off, ss, cs, d_out + off, ss, cs, nb_i, b->gain, cst, true, cv_a, cv_b, &cg, &ci);
            if (rc) return rc;
        }
        if (nch > 1 && deferred) {
            while (b->chunk_done.size() <= (size_t)i) {
                hipEvent_t ev;
                HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
                b->chunk_done.push_back(ev);
            }
            HIP_TRY(hipEventRecord(b->chunk_done[(size_t)i], b->st2));
        }
    }
    b->join_pending = false;
    if (nch > 1 && deferred) {      // the caller joins later (ohs_batch_join / ohs_batch_sync / the next call)
        b->join_pending = true;
        b->chunk_done_n = nch;
        b->pend_out = d_out; b->pend_blocks = n_blocks; b->pend_ss = stream_stride; b->pend_cs = channel_stride;
    } else if (nch > 1 && !joined) {    // join: the caller's stream continues only after the last convolution
        hipEvent_t ev;
        rc = get_event(&ev); if (rc) return rc;
        HIP_TRY(hipEventRecord(ev, b->st2));
        HIP_TRY(hipStreamWaitEvent(st, ev, 0));
        b->ev_inflight.push_back(ev);
    }
    return OHS_OK;
}

int ohs_batch_process(ohs_batch *b, const float *d_in, float *d_out, size_t n_blocks,
                      size_t stream_stride, size_t channel_stride, void *hip_stream)
{
    return batch_process_impl(b, d_in, d_out, n_blocks, stream_stride, channel_stride, hip_stream, false);
}

int ohs_batch_set_schedule_tables(ohs_batch *b, size_t n_tables, const float *coeffs, const uint8_t *enabled)
{
    if (!b) return fail(OHS_ERR_INVALID_ARG, "batch is NULL");
    if (n_tables > 0 && (!coeffs || !enabled)) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    if (n_tables > ((size_t)1 << 24)) return fail(OHS_ERR_INVALID_ARG, "n_tables too large");
    HIP_TRY(hipSetDevice(b->device));
    return eq_set_schedule_tables(b->eq, n_tables, coeffs, enabled, b->st);
}

int ohs_batch_last_eq_form(const ohs_batch *b, int *form, int *scheduled)
{
    if (!b || !form || !scheduled) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    *form = b->eq.last_form;
    *scheduled = b->eq.last_scheduled ? 1 : 0;
    return OHS_OK;
}

// ---- the staging slots of the scheduled calls ---------------------------------------------------------------------
// A scheduled call's rows travel through the next of the handle's kSchedSlots staging slots (pinned host memory: the caller's
// arrays are free on return, the copy to the device is asynchronous).  The lease closes the slot on every path out of the call
// that took it: `done` recorded behind whatever the call queued on its stream, waited for before the slot is filled again.
struct SchedLease {
    ohs_batch::SchedSlot *slot = nullptr;
    hipStream_t st = nullptr;
    SchedLease() = default;
    SchedLease(const SchedLease &) = delete;
    SchedLease &operator=(const SchedLease &) = delete;
    ~SchedLease()
    {
        if (!slot) return;
        if (hipEventRecord(slot->done, st) == hipSuccess) slot->in_use = true;
        else hipStreamSynchronize(st);
    }
};

// the next slot, free of its last user and with room for n_entries 32-bit entries
static int sched_lease(ohs_batch *b, size_t n_entries, hipStream_t st, SchedLease &lease)
{
    ohs_batch::SchedSlot &slot = b->sched_slot[b->sched_next];
    b->sched_next = (b->sched_next + 1) % ohs_batch::kSchedSlots;
    if (slot.in_use) HIP_TRY(hipEventSynchronize(slot.done));
    slot.in_use = false;
    if (!slot.done) HIP_TRY(hipEventCreateWithFlags(&slot.done, hipEventDisableTiming));
    lease.slot = &slot; lease.st = st;
    if (slot.cap < n_entries) {
        if (slot.h) hipHostFree(slot.h);
        if (slot.d) {
            DeviceWideSection dws;
            hipFree(slot.d);
        }
        slot.h = nullptr; slot.d = nullptr; slot.cap = 0;
        const size_t cap = std::max<size_t>(2048, n_entries + n_entries / 2);
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&slot.h), cap * sizeof(unsigned), hipHostMallocDefault));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&slot.d), cap * sizeof(unsigned)));
        slot.cap = cap;
    }
    return OHS_OK;
}

// `rows` rows of n 32-bit entries (table indices, gains), read `stride` entries apart; src NULL: nothing
struct SchedRows {
    const void *src;
    size_t stride, rows, n;
    size_t entries() const { return src ? rows * n : 0; }
};

// Arrays of rows into a slot, each packed n apart whatever the caller's stride and each right behind the one before, and ONE
// copy to the device on st.  -> lease.slot->d: the first array, the second first.entries() behind it, and so on.
static int sched_stage(ohs_batch *b, std::initializer_list<const SchedRows *> arrays, hipStream_t st, SchedLease &lease)
{
    size_t n_all = 0;
    for (const SchedRows *a : arrays) n_all += a->entries();
    const int rc = sched_lease(b, n_all, st, lease);
    if (rc) return rc;
    unsigned *h = lease.slot->h;
    for (const SchedRows *a : arrays)
        for (size_t r = 0; a->src && r < a->rows; ++r, h += a->n)
            std::memcpy(h, static_cast<const unsigned *>(a->src) + r * a->stride, a->n * sizeof(unsigned));
    HIP_TRY(hipMemcpyAsync(lease.slot->d, lease.slot->h, n_all * sizeof(unsigned), hipMemcpyHostToDevice, st));
    return OHS_OK;
}
static int sched_stage(ohs_batch *b, const SchedRows &first, const SchedRows &second, hipStream_t st, SchedLease &lease)
{
    return sched_stage(b, {&first, &second}, st, lease);
}

int ohs_batch_process_scheduled(ohs_batch *b, const float *d_in, float *d_out, size_t n_blocks, size_t stream_stride,
                                size_t channel_stride, size_t seg_blocks, const unsigned *table_idx, const float *gain,
                                void *hip_stream)
{
    if (!b || !d_in || !d_out) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    if (seg_blocks == 0) return fail(OHS_ERR_INVALID_ARG, "seg_blocks is 0");
    if (n_blocks > (size_t)1 << 24) return fail(OHS_ERR_INVALID_ARG, "n_blocks too large");
    if (b->eq.per_stream)
        return fail(OHS_ERR_INVALID_ARG, "a scheduled call on a handle with per-stream EQ tables is not supported "
                                         "(ohs_batch_share_eq_table goes back to the one shared table)");
    if (table_idx && b->eq.sched_n == 0)
        return fail(OHS_ERR_INVALID_ARG, "table_idx given, but no tables uploaded (ohs_batch_set_schedule_tables)");
    const size_t n_segs = sched_segments(n_blocks, &seg_blocks);
    if (table_idx)
        for (size_t k = 0; k < n_segs; ++k)
            if (table_idx[k] >= b->eq.sched_n) return fail(OHS_ERR_INVALID_ARG, "table_idx entry out of range");
    if (b->failed || n_blocks == 0)     // (the plain call's answers)
        return batch_process_impl(b, d_in, d_out, n_blocks, stream_stride, channel_stride, hip_stream, false);
    if (!batch_strides_ok(b->conv.S, stream_stride, channel_stride, n_blocks * BS))
        return fail(OHS_ERR_INVALID_ARG, "strides smaller than the processed region");
    // A constant schedule is the plain call: same launches, same bits.
    if (table_idx && sched_row_constant(table_idx, n_segs)) { batch_adopt_table(b, table_idx[0]); table_idx = nullptr; }
    if (gain && sched_row_constant(gain, n_segs)) { b->gain = gain[0]; gain = nullptr; }
    if (!table_idx && !gain)
        return batch_process_impl(b, d_in, d_out, n_blocks, stream_stride, channel_stride, hip_stream, false);

    HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const SchedRows tab_row{table_idx, 0, 1, n_segs}, gain_row{gain, 0, 1, n_segs};
    SchedLease lease;
    int rc = sched_stage(b, tab_row, gain_row, st, lease);
    if (rc) return rc;
    BatchSchedule sc;
    sc.seg_blocks = seg_blocks; sc.n_segs = n_segs; sc.tab = table_idx; sc.gain = gain;
    if (table_idx) sc.d_tab = lease.slot->d;
    if (gain) sc.d_gain = reinterpret_cast<const float *>(lease.slot->d + tab_row.entries());
    rc = batch_process_impl(b, d_in, d_out, n_blocks, stream_stride, channel_stride, hip_stream, false, &sc);
    if (rc) return rc;
    // the handle's table / gain are the last segment's now (what the setters do)
    if (table_idx) batch_adopt_table(b, table_idx[n_segs - 1]);
    if (gain) b->gain = gain[n_segs - 1];
    return OHS_OK;
}

int ohs_batch_process_scheduled_streams(ohs_batch *b, const float *d_in, float *d_out, size_t n_blocks, size_t stream_stride,
                                        size_t channel_stride, size_t seg_blocks, const unsigned *table_idx, size_t idx_stride,
                                        const float *gain, size_t gain_stride, void *hip_stream)
{
    if (!b || !d_in || !d_out) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    if (seg_blocks == 0) return fail(OHS_ERR_INVALID_ARG, "seg_blocks is 0");
    if (n_blocks > (size_t)1 << 24) return fail(OHS_ERR_INVALID_ARG, "n_blocks too large");
    if (table_idx && b->eq.per_stream)
        return fail(OHS_ERR_INVALID_ARG, "table_idx on a handle with static per-stream EQ tables is not supported: the schedule "
                                         "tables take their place (ohs_batch_share_eq_table), or pass table_idx = NULL");
    if (table_idx && b->eq.sched_n == 0)
        return fail(OHS_ERR_INVALID_ARG, "table_idx given, but no tables uploaded (ohs_batch_set_schedule_tables)");
    const size_t n_segs = sched_segments(n_blocks, &seg_blocks), S = b->conv.S;
    if ((table_idx && idx_stride != 0 && idx_stride < n_segs) || (gain && gain_stride != 0 && gain_stride < n_segs))
        return fail(OHS_ERR_INVALID_ARG, "a row stride is 0 (one row for all streams) or >= the number of segments");
    if (S * n_segs > (size_t)0x7fffffff) return fail(OHS_ERR_INVALID_ARG, "schedule too large");
    if (!table_idx) idx_stride = 0;
    if (!gain) gain_stride = 0;
    BatchSchedule sc;
    sc.seg_blocks = seg_blocks; sc.n_segs = n_segs; sc.streams = true;
    if (table_idx) {        // one pass over the caller's rows: the range check, and what the EQ launches have to know about the segments
        sc.tab = table_idx; sc.tab_stride = idx_stride;
        if (!eq_schedule_streams_scan(b->eq, sc)) return fail(OHS_ERR_INVALID_ARG, "table_idx entry out of range");
    }
    if (b->failed || n_blocks == 0)     // (the plain call's answers)
        return batch_process_impl(b, d_in, d_out, n_blocks, stream_stride, channel_stride, hip_stream, false);
    if (!batch_strides_ok(S, stream_stride, channel_stride, n_blocks * BS))
        return fail(OHS_ERR_INVALID_ARG, "strides smaller than the processed region");
    // rows that are all the same are one row
    if (idx_stride && sched_rows_equal(table_idx, idx_stride, S, n_segs)) idx_stride = 0;
    if (gain_stride && sched_rows_equal(gain, gain_stride, S, n_segs)) gain_stride = 0;
    // The schedule governs this call only: what the handle holds is put back behind it, whatever the call returns.
    struct Restore {
        ohs_batch *b;
        std::vector<float> coeffs; std::vector<int> en; float gain;
        explicit Restore(ohs_batch *b_) : b(b_), coeffs(b_->eq.coeffs), en(b_->eq.en.begin(), b_->eq.en.end()), gain(b_->gain) {}
        ~Restore()
        {
            b->gain = gain;
            if (!b->eq.per_stream)
                for (size_t band = 0; band < b->eq.nb; ++band) eq_set_shared_band(b->eq, band, &coeffs[5 * band], en[band]);
        }
    } restore(b);
    // one row of each for all streams: the launches of ohs_batch_process_scheduled (its bits); only the adoption differs
    if (!idx_stride && !gain_stride && !b->eq.per_stream)
        return ohs_batch_process_scheduled(b, d_in, d_out, n_blocks, stream_stride, channel_stride, seg_blocks, table_idx, gain, hip_stream);
    // a constant row of its own kind is the plain call's table / gain
    if (table_idx && !idx_stride && sched_row_constant(table_idx, n_segs)) { batch_adopt_table(b, table_idx[0]); table_idx = nullptr; }
    if (gain && !gain_stride && sched_row_constant(gain, n_segs)) { b->gain = gain[0]; gain = nullptr; }
    if (!table_idx && !gain)
        return batch_process_impl(b, d_in, d_out, n_blocks, stream_stride, channel_stride, hip_stream, false);

    HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = (hipStream_t)hip_stream;
    // a row per stream, or one for all: up to streams x n_segs entries per array
    const SchedRows tab_rows{table_idx, idx_stride, idx_stride ? S : 1, n_segs}, gain_rows{gain, gain_stride, gain_stride ? S : 1, n_segs};
    SchedLease lease;
    const int rc = sched_stage(b, tab_rows, gain_rows, st, lease);
    if (rc) return rc;
    sc.tab = nullptr; sc.tab_stride = 0;
    if (table_idx) { sc.tab = lease.slot->h; sc.d_tab = lease.slot->d; sc.tab_stride = idx_stride ? n_segs : 0; }
    if (gain) {
        sc.gain = reinterpret_cast<const float *>(lease.slot->h + tab_rows.entries());
        sc.d_gain = reinterpret_cast<const float *>(lease.slot->d + tab_rows.entries());
        sc.gain_stride = gain_stride ? n_segs : 0;
    }
    return batch_process_impl(b, d_in, d_out, n_blocks, stream_stride, channel_stride, hip_stream, false, &sc);
}

// ---- a schedule of HRIR sets inside one call -------------------------------------------------------------------
int ohs_batch_set_schedule_irs(ohs_batch *b, size_t n_sets, const float *irs, size_t len)
{
    if (!b) return fail(OHS_ERR_INVALID_ARG, "batch is NULL");
    if (n_sets > 0 && !irs) return fail(OHS_ERR_INVALID_ARG, "irs is NULL");
    if (n_sets > 0 && (len == 0 || len > (size_t)BS)) return fail(OHS_ERR_INVALID_ARG, "len must be 1 .. 512 (one partition)");
    if (n_sets > ((size_t)1 << 16)) return fail(OHS_ERR_INVALID_ARG, "n_sets too large");
    HIP_TRY(hipSetDevice(b->device));
    DeviceWideSection dws;
    HIP_TRY(hipDeviceSynchronize());
    return conv_set_schedule_irs(b->conv, b->ctx, n_sets, irs, len, b->st);
}

int ohs_batch_last_conv_ir_scheduled(const ohs_batch *b, int *scheduled)
{
    if (!b || !scheduled) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    *scheduled = b->conv.last_ir_crossfaded ? 2 : b->conv.last_ir_scheduled ? 1 : 0;
    return OHS_OK;
}

// ohs_batch_process_ir_scheduled (crossfade false) and ohs_batch_process_ir_crossfaded (crossfade true; switch_mode RING_OUT, prev_idx
// optional) share the validation pass, the staging slot and the state rules
static int batch_process_irs(ohs_batch *b, const float *d_in, float *d_out, size_t n_blocks, size_t stream_stride,
                             size_t channel_stride, size_t seg_blocks, const unsigned *ir_idx, size_t idx_stride,
                             int switch_mode, bool crossfade, const unsigned *prev_idx, void *hip_stream)
{
    if (!b || !d_in || !d_out || !ir_idx) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    if (seg_blocks == 0) return fail(OHS_ERR_INVALID_ARG, "seg_blocks is 0");
    if (switch_mode != OHS_IR_SWITCH_RING_OUT && switch_mode != OHS_IR_SWITCH_CUT)
        return fail(OHS_ERR_INVALID_ARG, "switch_mode must be OHS_IR_SWITCH_RING_OUT or OHS_IR_SWITCH_CUT");
    if (n_blocks > (size_t)1 << 24) return fail(OHS_ERR_INVALID_ARG, "n_blocks too large");
    ConvState &c = b->conv;
    if (c.irs_n == 0) return fail(OHS_ERR_INVALID_ARG, "no sets uploaded (ohs_batch_set_schedule_irs)");
    if (conv_max_p(c) != 1)
        return fail(OHS_ERR_INVALID_ARG, "the handle holds a response longer than one partition (512 taps): not supported in a schedule");
    if (c.pt_active) return fail(OHS_ERR_INVALID_ARG, "the handle has pending tails of a longer response: not supported in a schedule");
    if (!c.lazy_ok) return fail(OHS_ERR_INVALID_ARG, "the handle does not keep the lazy state the scheduled kernel leaves");
    const size_t n_segs = sched_segments(n_blocks, &seg_blocks), S = c.S;
    if (idx_stride != 0 && idx_stride < n_segs)
        return fail(OHS_ERR_INVALID_ARG, "idx_stride is 0 (one row for all streams) or >= the number of segments");
    if (S * n_segs > (size_t)0x7fffffff) return fail(OHS_ERR_INVALID_ARG, "schedule too large");
    // one pass over the rows (and prev_idx, which the crossfaded call alone reads)
    if (!crossfade) prev_idx = nullptr;
    const ohs_host::SchedRowScan rs = ohs_host::sched_scan_rows(ir_idx, idx_stride, idx_stride ? S : 1, n_segs, (unsigned)c.irs_n, prev_idx,
                                                                n_blocks, seg_blocks);
    if (rs.idx_bad) return fail(OHS_ERR_INVALID_ARG, "ir_idx entry out of range");
    if (rs.prev_bad) return fail(OHS_ERR_INVALID_ARG, "prev_idx entry out of range");
    // The crossfaded call: a fade begins at a change along a row, or at the call's start against prev_idx.  A call without any such
    // boundary takes the RING_OUT paths below: their launches, their bits.
    crossfade = crossfade && (rs.vary || rs.prev_boundary);
    if (b->failed || n_blocks == 0)     // (the plain call's answers)
        return batch_process_impl(b, d_in, d_out, n_blocks, stream_stride, channel_stride, hip_stream, false);
    if (!batch_strides_ok(S, stream_stride, channel_stride, n_blocks * BS))
        return fail(OHS_ERR_INVALID_ARG, "strides smaller than the processed region");
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const bool cut = switch_mode == OHS_IR_SWITCH_CUT, shared = idx_stride == 0;
    if (shared && !rs.vary && !crossfade) {
        // One set throughout, for all streams: the plain kernel on that set's table -- the plain call's launches and bits.  The overlaps
        // at rest belong to the responses that go: under RING_OUT they are computed now (and ring out), under CUT the call's start is a
        // boundary and they are zero, as after four set_ir.
        if (cut) {
            HIP_TRY(hipMemsetAsync(c.d_tails, 0, S * 2 * 8 * 64 * sizeof(float2), st));
            c.tails_lazy = false; c.tails_both = false;
        } else {
            const int rcm = conv_materialise_keep_lazy(c, b->ctx, st);
            if (rcm) return rcm;
        }
        const int rca = conv_adopt_schedule_set(c, ir_idx[0], st);
        if (rca) return rca;
        return batch_process_impl(b, d_in, d_out, n_blocks, stream_stride, channel_stride, hip_stream, false);
    }
    // the rows' staging slot: equal rows travel as one; the crossfaded call's prev_idx travels behind the rows.  The slot is closed
    // right behind the call's launches.
    const size_t n_rows_src = rs.rows_differ ? S : 1, n_rows = n_rows_src * n_segs;
    const size_t n_prev = (crossfade && prev_idx) ? (rs.prev_differ ? S : 1) : 0;
    int rc;
    {
        SchedLease lease;
        rc = sched_stage(b, {ir_idx, idx_stride, n_rows_src, n_segs}, {prev_idx, 0, 1, n_prev}, st, lease);
        if (rc) return rc;
        ConvIrs ci;
        ci.tab = lease.slot->d; ci.seg_blocks = (int)seg_blocks; ci.stream_stride = rs.rows_differ ? (int)n_segs : 0;
        ci.call_blocks = (int)n_blocks; ci.cut = cut;
        ci.per_stream_state = !shared;      // (a shared row is adopted below: the handle's spectra rebuild the overlaps when asked)
        if (crossfade) {
            // faded_end: the call's last block is a fade in some stream, its per-path overlaps the sum of both halves of the fade
            ci.xfade = true; ci.faded_end = rs.faded_end;
            if (n_prev) { ci.prev = lease.slot->d + n_rows; ci.prev_stride = rs.prev_differ ? 1 : 0; }
        }
        rc = batch_process_impl(b, d_in, d_out, n_blocks, stream_stride, channel_stride, hip_stream, false, nullptr, &ci);
    }
    if (rc) return rc;
    // one row for all streams: the handle's responses ARE the last segment's now (what ohs_batch_process_scheduled does with its table)
    if (shared) return conv_adopt_schedule_set(c, ir_idx[n_segs - 1], st);
    return OHS_OK;
}

int ohs_batch_process_ir_scheduled(ohs_batch *b, const float *d_in, float *d_out, size_t n_blocks, size_t stream_stride,
                                   size_t channel_stride, size_t seg_blocks, const unsigned *ir_idx, size_t idx_stride,
                                   int switch_mode, void *hip_stream)
{
    return batch_process_irs(b, d_in, d_out, n_blocks, stream_stride, channel_stride, seg_blocks, ir_idx, idx_stride, switch_mode,
                             false, nullptr, hip_stream);
}

int ohs_batch_process_ir_crossfaded(ohs_batch *b, const float *d_in, float *d_out, size_t n_blocks, size_t stream_stride,
                                    size_t channel_stride, size_t seg_blocks, const unsigned *ir_idx, size_t idx_stride,
                                    const unsigned *prev_idx, void *hip_stream)
{
    return batch_process_irs(b, d_in, d_out, n_blocks, stream_stride, channel_stride, seg_blocks, ir_idx, idx_stride,
                             OHS_IR_SWITCH_RING_OUT, true, prev_idx, hip_stream);
}

// ---- speaker layouts: K channels -> two ears in one kernel ---------------------------------------------------------
int ohs_batch_set_layout_irs(ohs_batch *b, size_t n_channels, const float *irs, size_t len)
{
    if (!b) return fail(OHS_ERR_INVALID_ARG, "batch is NULL");
    if (n_channels > 0 && !irs) return fail(OHS_ERR_INVALID_ARG, "irs is NULL");
    if (n_channels > 16) return fail(OHS_ERR_INVALID_ARG, "n_channels must be at most 16");
    if (n_channels > 0 && (len == 0 || len > (size_t)BS)) return fail(OHS_ERR_INVALID_ARG, "len must be 1 .. 512 (one partition)");
    HIP_TRY(hipSetDevice(b->device));
    DeviceWideSection dws;
    HIP_TRY(hipDeviceSynchronize());
    return conv_set_layout_irs(b->conv, b->ctx, n_channels, irs, len, b->st);
}

int ohs_batch_last_layout_launch(const ohs_batch *b, int *n_pairs, int *ranges_per_stream)
{
    if (!b || !n_pairs || !ranges_per_stream) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    *n_pairs = b->conv.last_lay_pairs;
    *ranges_per_stream = b->conv.last_lay_ranges;
    return OHS_OK;
}

// one strided region [n_outer][n_inner][frames] fits its strides: the inner index inside the outer stride, or the other way round
static bool layout_strides_ok(size_t n_outer, size_t outer, size_t n_inner, size_t inner, size_t frames)
{
    if (n_inner > 1 && inner < frames) return false;
    if (n_outer > 1 && outer < frames) return false;
    if (n_outer <= 1 || n_inner <= 1) return true;
    return outer >= (n_inner - 1) * inner + frames || inner >= (n_outer - 1) * outer + frames;
}

// The layout calls' regions, in [S][K][frames] and out [S][2][frames]: each fits its strides, and -- out of place only -- the two, first
// to last frame touched, do not meet.  false: refused, the message set.
static bool layout_regions_ok(size_t S, size_t K, size_t frames, const float *d_in, size_t in_ss, size_t in_cs, const float *d_out,
                              size_t out_ss, size_t out_cs)
{
    if (!layout_strides_ok(S, in_ss, K, in_cs, frames) || !layout_strides_ok(S, out_ss, 2, out_cs, frames)) {
        fail(OHS_ERR_INVALID_ARG, "strides smaller than the processed region");
        return false;
    }
    const float *in_end = d_in + (S - 1) * in_ss + (K - 1) * in_cs + frames;
    const float *out_end = d_out + (S - 1) * out_ss + out_cs + frames;
    if (!(in_end <= d_out || out_end <= d_in)) {
        fail(OHS_ERR_INVALID_ARG, "input and output regions overlap (the layout call is out of place only)");
        return false;
    }
    return true;
}

int ohs_batch_process_layout(ohs_batch *b, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                             size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride, void *hip_stream)
{
    if (!b || !d_in || !d_out) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    ConvState &c = b->conv;
    if (c.lay_K == 0 || !c.d_lay_cd) return fail(OHS_ERR_INVALID_ARG, "no layout uploaded (ohs_batch_set_layout_irs)");
    if (n_blocks > (size_t)1 << 24) return fail(OHS_ERR_INVALID_ARG, "n_blocks too large");
    if (b->failed) return batch_refuse_failed(b);
    if (n_blocks == 0) return OHS_OK;
    const size_t frames = n_blocks * BS, S = c.S, K = c.lay_K;
    if (!layout_regions_ok(S, K, frames, d_in, in_stream_stride, in_channel_stride, d_out, out_stream_stride, out_channel_stride))
        return OHS_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = (hipStream_t)hip_stream;
    auto body = [&]() -> int {
        if (b->join_pending) {      // (a deferred call's last convolutions: the EQ state and d_out may be theirs)
            HIP_TRY(hipStreamWaitEvent(st, b->chunk_done[(size_t)b->chunk_done_n - 1], 0));
            b->join_pending = false;
        }
        int rc = conv_launch_layout(c, b->ctx, d_in, (long long)in_stream_stride, (long long)in_channel_stride, d_out,
                                    (long long)out_stream_stride, (long long)out_channel_stride, (int)n_blocks, b->gain, st);
        if (rc) return rc;
        if (b->eq_enable && eq_any_enabled(b->eq))      // EQ(gain * conv(x)): the two ear channels, in place, behind the whole call
            rc = eq_launch(b->eq, d_out, d_out, (long long)out_stream_stride, (long long)out_channel_stride, (long long)frames, st);
        return rc;
    };
    const int rc = body();
    if (rc == OHS_OK || rc == OHS_ERR_INVALID_ARG) return rc;
    return batch_mark_failed(b, rc);
}

// ---- head-tracked speaker layouts: a table of layouts walked per stream and segment ----------------------------------
int ohs_batch_set_layout_schedule_irs(ohs_batch *b, size_t n_sets, size_t n_channels, const float *irs, size_t len)
{
    if (!b) return fail(OHS_ERR_INVALID_ARG, "batch is NULL");
    if (n_sets > 0) {
        if (!irs) return fail(OHS_ERR_INVALID_ARG, "irs is NULL");
        if (n_sets > 65536) return fail(OHS_ERR_INVALID_ARG, "n_sets must be at most 65536");
        if (n_channels == 0 || n_channels > 16) return fail(OHS_ERR_INVALID_ARG, "n_channels must be 1 .. 16");
        if (len == 0 || len > (size_t)BS) return fail(OHS_ERR_INVALID_ARG, "len must be 1 .. 512 (one partition)");
    }
    HIP_TRY(hipSetDevice(b->device));
    DeviceWideSection dws;
    HIP_TRY(hipDeviceSynchronize());
    return conv_set_layout_schedule_irs(b->conv, b->ctx, n_sets, n_channels, irs, len, b->st);
}

int ohs_batch_last_layout_scheduled(const ohs_batch *b, int *scheduled)
{
    if (!b || !scheduled) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    *scheduled = b->conv.last_lay_scheduled ? 1 : 0;
    return OHS_OK;
}

int ohs_batch_process_layout_scheduled(ohs_batch *b, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                                       size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride,
                                       size_t seg_blocks, const unsigned *set_idx, size_t idx_stride, const unsigned *prev_idx,
                                       int switch_mode, void *hip_stream)
{
    if (!b || !d_in || !d_out || !set_idx) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    if (seg_blocks == 0) return fail(OHS_ERR_INVALID_ARG, "seg_blocks is 0");
    if (switch_mode != OHS_LAYOUT_SWITCH_RING_OUT && switch_mode != OHS_LAYOUT_SWITCH_CROSSFADE)
        return fail(OHS_ERR_INVALID_ARG, "switch_mode must be OHS_LAYOUT_SWITCH_RING_OUT or OHS_LAYOUT_SWITCH_CROSSFADE");
    ConvState &c = b->conv;
    if (c.lays_n == 0 || !c.d_lays_cd) return fail(OHS_ERR_INVALID_ARG, "no table uploaded (ohs_batch_set_layout_schedule_irs)");
    if (n_blocks > (size_t)1 << 24) return fail(OHS_ERR_INVALID_ARG, "n_blocks too large");
    if (b->failed) return batch_refuse_failed(b);
    if (n_blocks == 0) return OHS_OK;
    const size_t n_segs = sched_segments(n_blocks, &seg_blocks), frames = n_blocks * BS, S = c.S, K = c.lays_K;
    if (idx_stride != 0 && idx_stride < n_segs)
        return fail(OHS_ERR_INVALID_ARG, "idx_stride is 0 (one row for all streams) or >= the number of segments");
    if (S * n_segs > (size_t)0x7fffffff) return fail(OHS_ERR_INVALID_ARG, "schedule too large");
    const bool fade = switch_mode == OHS_LAYOUT_SWITCH_CROSSFADE, shared = idx_stride == 0;
    if (!fade) prev_idx = nullptr;      // (read under CROSSFADE only)
    // one pass over the rows, prev_idx beside them
    const ohs_host::SchedRowScan rs = ohs_host::sched_scan_rows(set_idx, idx_stride, shared ? 1 : S, n_segs, (unsigned)c.lays_n, prev_idx,
                                                                n_blocks, seg_blocks);
    if (rs.idx_bad) return fail(OHS_ERR_INVALID_ARG, "set_idx entry out of range");
    if (rs.prev_bad) return fail(OHS_ERR_INVALID_ARG, "prev_idx entry out of range");
    if (!layout_regions_ok(S, K, frames, d_in, in_stream_stride, in_channel_stride, d_out, out_stream_stride, out_channel_stride))
        return OHS_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = (hipStream_t)hip_stream;
    // one set throughout, for all streams, and no boundary at the call's start: k_conv_p1_layout on that set's slice of the table
    const bool plain = shared && !rs.vary && !rs.prev_boundary;
    SchedLease lease;
    auto body = [&]() -> int {
        if (b->join_pending) {      // (a deferred call's last convolutions: the EQ state and d_out may be theirs)
            HIP_TRY(hipStreamWaitEvent(st, b->chunk_done[(size_t)b->chunk_done_n - 1], 0));
            b->join_pending = false;
        }
        ConvLayoutRows lr;
        if (!plain) {
            // the rows' staging slot (the IR-scheduled calls'): rows packed n_segs apart, equal rows travel as one; prev_idx behind them
            const size_t n_rows_src = rs.rows_differ ? S : 1, n_prev = prev_idx ? (rs.prev_differ ? S : 1) : 0;
            const int rcs = sched_stage(b, {set_idx, idx_stride, n_rows_src, n_segs}, {prev_idx, 0, 1, n_prev}, st, lease);
            if (rcs) return rcs;
            lr.tab = lease.slot->d; lr.seg_blocks = (int)seg_blocks; lr.stream_stride = rs.rows_differ ? (int)n_segs : 0;
            lr.fade = fade;
            if (n_prev) { lr.prev = lease.slot->d + n_rows_src * n_segs; lr.prev_stride = rs.prev_differ ? 1 : 0; }
        }
        int rc = conv_launch_layout_scheduled(c, b->ctx, d_in, (long long)in_stream_stride, (long long)in_channel_stride, d_out,
                                              (long long)out_stream_stride, (long long)out_channel_stride, (int)n_blocks, b->gain, st,
                                              plain ? nullptr : &lr, set_idx[0]);
        if (rc) return rc;
        if (b->eq_enable && eq_any_enabled(b->eq))      // EQ(gain * conv(x)): the two ear channels, in place, behind the whole call
            rc = eq_launch(b->eq, d_out, d_out, (long long)out_stream_stride, (long long)out_channel_stride, (long long)frames, st);
        return rc;
    };
    const int rc = body();
    if (rc == OHS_OK || rc == OHS_ERR_INVALID_ARG) return rc;
    return batch_mark_failed(b, rc);
}

// ---- object scenes: K moving sources per stream -> two ears (libohs_scene.so; no entry of ohs_hip.h) -------------------
// Library-internal: api_scene.hip's shims are the only callers, and exports.map keeps the names local.
extern "C" int ohsint_batch_set_object_dirs(ohs_batch *b, size_t n_dirs, const float *irs, size_t len)
{
    if (!b) return fail(OHS_ERR_INVALID_ARG, "scene is NULL");
    if (n_dirs > 0) {
        if (!irs) return fail(OHS_ERR_INVALID_ARG, "irs is NULL");
        if (n_dirs > 65536) return fail(OHS_ERR_INVALID_ARG, "n_dirs must be at most 65536");
        if (len == 0 || len > (size_t)BS) return fail(OHS_ERR_INVALID_ARG, "len must be 1 .. 512 (one partition)");
    }
    HIP_TRY(hipSetDevice(b->device));
    DeviceWideSection dws;
    HIP_TRY(hipDeviceSynchronize());
    return conv_set_object_dirs(b->conv, b->ctx, n_dirs, irs, len, b->st);
}

extern "C" int ohsint_batch_last_objects_launch(const ohs_batch *b, int *n_pairs, int *ranges_per_stream, unsigned long long *fading_passes)
{
    if (!b || !n_pairs || !ranges_per_stream || !fading_passes) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    *n_pairs = b->conv.last_obj_pairs;
    *ranges_per_stream = b->conv.last_obj_ranges;
    *fading_passes = b->conv.last_obj_fading;
    return OHS_OK;
}

// The scene call, one direction per object (dir_idx1 == weight == nullptr: k_conv_p1_objects), two with a weight (both given:
// k_conv_p1_objects_blend) or three with two weights (dir_idx2 and weight2 given as well: k_conv_p1_objects_blend3): one set of
// checks, one scan over every row that will be read, one staging path, one epilogue.
static int batch_process_objects_any(ohs_batch *b, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                                     size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride, size_t n_objects,
                                     size_t seg_blocks, const unsigned *dir_idx, const float *obj_gain, size_t idx_stride,
                                     const unsigned *prev_idx, const float *prev_gain, int switch_mode, void *hip_stream,
                                     const unsigned *dir_idx1, const float *weight, const unsigned *prev_idx1, const float *prev_weight,
                                     const unsigned *dir_idx2 = nullptr, const float *weight2 = nullptr, const unsigned *prev_idx2 = nullptr,
                                     const float *prev_weight2 = nullptr)
{
    if (!b || !d_in || !d_out || !dir_idx) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    if ((dir_idx1 == nullptr) != (weight == nullptr)) return fail(OHS_ERR_INVALID_ARG, "dir_idx1 and weight are both NULL or both given");
    if ((dir_idx2 == nullptr) != (weight2 == nullptr)) return fail(OHS_ERR_INVALID_ARG, "dir_idx2 and weight2 are both NULL or both given");
    if (dir_idx2 && !dir_idx1) return fail(OHS_ERR_INVALID_ARG, "dir_idx2 and weight2 need dir_idx1 and weight");
    const bool blend = dir_idx1 != nullptr, tri = dir_idx2 != nullptr;
    if (!blend) { prev_idx1 = nullptr; prev_weight = nullptr; }     // (nothing for them to stand in front of)
    if (!tri) { prev_idx2 = nullptr; prev_weight2 = nullptr; }
    if (n_objects == 0 || n_objects > 64) return fail(OHS_ERR_INVALID_ARG, "n_objects must be 1 .. 64");
    if (seg_blocks == 0) return fail(OHS_ERR_INVALID_ARG, "seg_blocks is 0");
    if (switch_mode != 0 && switch_mode != 1) return fail(OHS_ERR_INVALID_ARG, "switch_mode must be OHS_SCENE_SWITCH_RING_OUT or OHS_SCENE_SWITCH_CROSSFADE");
    ConvState &c = b->conv;
    if (c.obj_n == 0 || !c.d_obj_ah)
        return fail(OHS_ERR_INVALID_ARG, tri ? "no direction table uploaded (ohs_scene3_set_direction_irs)"
                                             : "no direction table uploaded (ohs_scene_set_direction_irs)");
    if (n_blocks > (size_t)1 << 24) return fail(OHS_ERR_INVALID_ARG, "n_blocks too large");
    if (b->failed) return batch_refuse_failed(b);
    if (n_blocks == 0) return OHS_OK;
    const size_t n_segs = sched_segments(n_blocks, &seg_blocks), frames = n_blocks * BS, S = c.S, K = n_objects;
    if (idx_stride != 0 && idx_stride < n_segs)
        return fail(OHS_ERR_INVALID_ARG, "idx_stride is 0 (one row for all streams) or >= the number of segments");
    if ((tri ? 6 : blend ? 4 : 1) * S * n_segs * K > (size_t)0x7fffffff) return fail(OHS_ERR_INVALID_ARG, "schedule too large");
    const bool fade = switch_mode == 1, shared = idx_stride == 0;
    if (!fade) { prev_idx = nullptr; prev_gain = nullptr; prev_idx1 = nullptr; prev_weight = nullptr; }    // (read under CROSSFADE only)
    if (!fade) { prev_idx2 = nullptr; prev_weight2 = nullptr; }
    const size_t n_rows = shared ? 1 : S;
    // The blended kernels read 2 n_dirs planes of one shape -- four for two directions, six for three -- and, under CROSSFADE, as many
    // planes in front of the call that the host always stages (the first segment's own entries where the caller names none).  A gain
    // in front of the call beside no gain rows: the rows read as 1.0, so they are staged as that.
    std::vector<float> ones;
    std::vector<unsigned> prev;     // [4][n_rows][K]: idx, idx1, weight, gain in front of the call; [6]: idx, idx1, idx2, w1, w2, gain
    size_t gain_stride = idx_stride;
    if (blend) {
        try {
            if (!obj_gain && prev_gain) ones.assign(n_rows * n_segs * K, 1.0f);
            if (fade) prev.resize((tri ? 6 : 4) * n_rows * K);
        } catch (const std::bad_alloc &) {
            return fail(OHS_ERR_ALLOC, "out of host memory for the rows' staging");
        }
        if (!ones.empty()) { obj_gain = ones.data(); gain_stride = shared ? 0 : n_segs; }
    }
    const unsigned kOne = 0x3f800000u;
    const unsigned *gain_bits = reinterpret_cast<const unsigned *>(obj_gain), *pgain_bits = reinterpret_cast<const unsigned *>(prev_gain);
    const unsigned *w_bits = reinterpret_cast<const unsigned *>(weight), *pw_bits = reinterpret_cast<const unsigned *>(prev_weight);
    const unsigned *w2_bits = reinterpret_cast<const unsigned *>(weight2), *pw2_bits = reinterpret_cast<const unsigned *>(prev_weight2);
    auto weight_ok = [](unsigned bits) {
        float w;
        std::memcpy(&w, &bits, sizeof w);
        return w >= 0.0f && w <= 1.0f;      // (NaN fails both; -0.0 passes)
    };
    auto weights_ok = [](unsigned bits1, unsigned bits2) {
        float w1, w2;
        std::memcpy(&w1, &bits1, sizeof w1);
        std::memcpy(&w2, &bits2, sizeof w2);
        const volatile float sum = w1 + w2;     // (the sum in f32, whatever the host compiler would keep it in)
        return w1 >= 0.0f && w2 >= 0.0f && sum <= 1.0f;     // (NaN fails; -0.0 passes)
    };
    // one pass over every row that will be read: the indices against the table, the weights against [0, 1] (three directions: against
    // the triangle), the passes through old directions, the passes that load four rows and the passes that load six
    unsigned long long fading = 0, blended = 0, blended3 = 0;
    for (size_t r = 0; r < n_rows; ++r) {
        const size_t ro = r * idx_stride * K;
        const unsigned *row = dir_idx + ro, *row1 = blend ? dir_idx1 + ro : nullptr, *wrow = blend ? w_bits + ro : nullptr;
        const unsigned *grow = gain_bits ? gain_bits + r * gain_stride * K : nullptr;
        const unsigned *oi = prev_idx ? prev_idx + r * K : nullptr, *oj = prev_idx1 ? prev_idx1 + r * K : nullptr;
        const unsigned *ow = pw_bits ? pw_bits + r * K : nullptr, *og = pgain_bits ? pgain_bits + r * K : nullptr;
        const unsigned *row2 = tri ? dir_idx2 + ro : nullptr, *w2row = tri ? w2_bits + ro : nullptr;
        const unsigned *ok = prev_idx2 ? prev_idx2 + r * K : nullptr, *ov = pw2_bits ? pw2_bits + r * K : nullptr;
        for (size_t o = 0; o < K; ++o) {
            if (oi && oi[o] >= c.obj_n) return fail(OHS_ERR_INVALID_ARG, "prev_idx entry out of range");
            if (oj && oj[o] >= c.obj_n) return fail(OHS_ERR_INVALID_ARG, "prev_idx1 entry out of range");
            if (ok && ok[o] >= c.obj_n) return fail(OHS_ERR_INVALID_ARG, "prev_idx2 entry out of range");
            if (!tri && ow && !weight_ok(ow[o])) return fail(OHS_ERR_INVALID_ARG, "prev_weight entry outside [0, 1]");
        }
        const bool prev_w_named = ow || ov;
        if (fade) {         // (no boundary at the call's start for what the caller does not name)
            if (!oi) oi = row;
            if (!oj) oj = row1;
            if (!ow) ow = wrow;
            if (!og) og = grow;
            if (!ok) ok = row2;
            if (!ov) ov = w2row;
            // (the pair in front of the call, whichever half of it the caller named; with neither named it is the first segment's
            // own pair, which the scan below checks under its own name)
            for (size_t o = 0; tri && o < K; ++o)
                if (prev_w_named && !weights_ok(ow[o], ov[o]))
                    return fail(OHS_ERR_INVALID_ARG, "prev_weight / prev_weight2 entry outside w1 >= 0, w2 >= 0, w1 + w2 <= 1");
            // the planes in front of the call, in the kernel's order: the directions, the weights, the gain
            if (blend) {        // (one direction: prev is empty, the kernel reads prev_idx / prev_gain themselves)
                const unsigned *const front3[6] = {oi, oj, ok, ow, ov, og}, *const front2[4] = {oi, oj, ow, og};
                const unsigned *const *front = tri ? front3 : front2;
                for (size_t pl = 0; pl < (tri ? 6u : 4u); ++pl)
                    for (size_t o = 0; o < K; ++o) prev[(pl * n_rows + r) * K + o] = front[pl] ? front[pl][o] : kOne;     // (only the gain can be absent)
            }
        }
        for (size_t k = 0; k < n_segs; ++k) {
            const unsigned *ci = row + k * K, *cj = blend ? row1 + k * K : nullptr, *cw = blend ? wrow + k * K : nullptr;
            const unsigned *cg = grow ? grow + k * K : nullptr;
            const unsigned *ck = tri ? row2 + k * K : nullptr, *cv = tri ? w2row + k * K : nullptr;
            for (size_t o = 0; o < K; ++o) {
                if (ci[o] >= c.obj_n) return fail(OHS_ERR_INVALID_ARG, "dir_idx entry out of range");
                if (blend && cj[o] >= c.obj_n) return fail(OHS_ERR_INVALID_ARG, "dir_idx1 entry out of range");
                if (tri && ck[o] >= c.obj_n) return fail(OHS_ERR_INVALID_ARG, "dir_idx2 entry out of range");
                if (blend && !tri && !weight_ok(cw[o])) return fail(OHS_ERR_INVALID_ARG, "weight entry outside [0, 1]");
                if (tri && !weights_ok(cw[o], cv[o]))
                    return fail(OHS_ERR_INVALID_ARG, "weight / weight2 entry outside w1 >= 0, w2 >= 0, w1 + w2 <= 1");
            }
            const unsigned long long seg_len = std::min(seg_blocks, n_blocks - k * seg_blocks);
            for (size_t p = 0; 2 * p < K; ++p) {
                bool ch = false, cur_blend = false, old_blend = false, cur_tri = false, old_tri = false;
                for (size_t o = 2 * p; o < std::min(2 * p + 2, K); ++o) {
                    cur_blend = cur_blend || (blend && cw[o] != 0u);
                    cur_tri = cur_tri || (tri && cv[o] != 0u);
                    if (!fade) continue;
                    old_blend = old_blend || (blend && ow[o] != 0u);
                    old_tri = old_tri || (tri && ov[o] != 0u);
                    // (idx2 beside a w2 of +0.0 before and after is never read either)
                    ch = ch || (tri && (cv[o] != ov[o] || ((cv[o] | ov[o]) != 0u && ck[o] != ok[o])));
                    ch = ch || ci[o] != oi[o] || (cg ? cg[o] : kOne) != (og ? og[o] : kOne);
                    // (idx1 beside a weight of +0.0 before and after is never read: no change, as in the kernel)
                    ch = ch || (blend && (cw[o] != ow[o] || ((cw[o] | ow[o]) != 0u && cj[o] != oj[o])));
                }
                fading += ch ? 1 : 0;
                // (a pass with a nonzero w2 loads six rows; one without it and with a nonzero w1 loads four)
                blended += (cur_blend && !cur_tri ? seg_len : 0) + (ch && old_blend && !old_tri ? 1 : 0);
                blended3 += (cur_tri ? seg_len : 0) + (ch && old_tri ? 1 : 0);
            }
            oi = ci; oj = cj; ow = cw; og = cg; ok = ck; ov = cv;
        }
    }
    if (shared) { fading *= S; blended *= S; blended3 *= S; }
    if (!layout_regions_ok(S, K, frames, d_in, in_stream_stride, in_channel_stride, d_out, out_stream_stride, out_channel_stride))
        return OHS_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = (hipStream_t)hip_stream;
    SchedLease lease;
    auto body = [&]() -> int {
        if (b->join_pending) {      // (a deferred call's last convolutions: the EQ state and d_out may be theirs)
            HIP_TRY(hipStreamWaitEvent(st, b->chunk_done[(size_t)b->chunk_done_n - 1], 0));
            b->join_pending = false;
        }
        // the rows' staging slot (the scheduled calls'), each array packed and one behind the other
        const SchedRows ri{dir_idx, idx_stride * K, n_rows, n_segs * K}, rg{obj_gain, gain_stride * K, n_rows, n_segs * K};
        int rc;
        if (blend) {        // the directions, the weights, the gains -- 2 n_dirs planes of one size, the last possibly absent --, then prev
            const int n_dirs = tri ? 3 : 2;
            const size_t plane = n_rows * n_segs * K;
            const SchedRows rj{dir_idx1, idx_stride * K, n_rows, n_segs * K}, rk{dir_idx2, idx_stride * K, n_rows, n_segs * K},
                rw{weight, idx_stride * K, n_rows, n_segs * K}, rv{weight2, idx_stride * K, n_rows, n_segs * K},
                pv{fade ? prev.data() : nullptr, prev.size(), 1, prev.size()};
            const int rcs = sched_stage(b, {&ri, &rj, &rk, &rw, &rv, &rg, &pv}, st, lease);     // (two directions: rk and rv take no room)
            if (rcs) return rcs;
            ConvObjectBlendRows rows;
            rows.rows = lease.slot->d; rows.plane = (int)plane; rows.has_gain = obj_gain != nullptr;
            if (fade) rows.prev = lease.slot->d + (2 * n_dirs - 1) * plane + rg.entries();
            rows.prev_plane = (int)(n_rows * K);
            rows.seg_blocks = (int)seg_blocks; rows.stream_stride = shared ? 0 : (int)(n_segs * K); rows.prev_stride = shared ? 0 : (int)K;
            rows.fade = fade;
            rc = conv_launch_objects_blend(c, b->ctx, d_in, (long long)in_stream_stride, (long long)in_channel_stride, d_out,
                                           (long long)out_stream_stride, (long long)out_channel_stride, (int)n_blocks, b->gain, st, (int)K, n_dirs, rows);
        } else {            // indices, gains, prev_idx, prev_gain
            const SchedRows pi{prev_idx, K, n_rows, K}, pg{prev_gain, K, n_rows, K};
            const int rcs = sched_stage(b, {&ri, &rg, &pi, &pg}, st, lease);
            if (rcs) return rcs;
            ConvObjectRows rows;
            const unsigned *d = lease.slot->d;
            rows.idx = d; d += ri.entries();
            if (obj_gain) rows.gain = d;
            d += rg.entries();
            if (prev_idx) rows.prev_idx = d;
            d += pi.entries();
            if (prev_gain) rows.prev_gain = d;
            rows.seg_blocks = (int)seg_blocks; rows.stream_stride = shared ? 0 : (int)(n_segs * K); rows.prev_stride = shared ? 0 : (int)K;
            rows.fade = fade;
            rc = conv_launch_objects(c, b->ctx, d_in, (long long)in_stream_stride, (long long)in_channel_stride, d_out,
                                     (long long)out_stream_stride, (long long)out_channel_stride, (int)n_blocks, b->gain, st, (int)K, rows);
        }
        if (rc) return rc;
        c.last_obj_fading = fading; c.last_obj_blended = blended; c.last_obj_blended3 = blended3;
        if (b->eq_enable && eq_any_enabled(b->eq))      // EQ(gain * conv(x)): the two ear channels, in place, behind the whole call
            rc = eq_launch(b->eq, d_out, d_out, (long long)out_stream_stride, (long long)out_channel_stride, (long long)frames, st);
        return rc;
    };
    const int rc = body();
    if (rc == OHS_OK || rc == OHS_ERR_INVALID_ARG) return rc;
    return batch_mark_failed(b, rc);
}

extern "C" int ohsint_batch_process_objects(ohs_batch *b, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                                            size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride,
                                            size_t n_objects, size_t seg_blocks, const unsigned *dir_idx, const float *obj_gain,
                                            size_t idx_stride, const unsigned *prev_idx, const float *prev_gain, int switch_mode,
                                            void *hip_stream)
{
    return batch_process_objects_any(b, d_in, d_out, n_blocks, in_stream_stride, in_channel_stride, out_stream_stride, out_channel_stride,
                                     n_objects, seg_blocks, dir_idx, obj_gain, idx_stride, prev_idx, prev_gain, switch_mode, hip_stream,
                                     nullptr, nullptr, nullptr, nullptr);
}

// ---- blended object scenes: two directions and a weight per object (libohs_scene2.so; no entry of ohs_hip.h or ohs_scene.h) ------
// dir_idx1 and weight both NULL: ohsint_batch_process_objects
extern "C" int ohsint_batch_process_objects_blend(ohs_batch *b, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                                                  size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride,
                                                  size_t n_objects, size_t seg_blocks, const unsigned *dir_idx, const float *obj_gain,
                                                  size_t idx_stride, const unsigned *prev_idx, const float *prev_gain, int switch_mode,
                                                  void *hip_stream, const unsigned *dir_idx1, const float *weight,
                                                  const unsigned *prev_idx1, const float *prev_weight)
{
    return batch_process_objects_any(b, d_in, d_out, n_blocks, in_stream_stride, in_channel_stride, out_stream_stride, out_channel_stride,
                                     n_objects, seg_blocks, dir_idx, obj_gain, idx_stride, prev_idx, prev_gain, switch_mode, hip_stream,
                                     dir_idx1, weight, prev_idx1, prev_weight);
}

extern "C" int ohsint_batch_last_objects_blend_launch(const ohs_batch *b, int *n_pairs, int *ranges_per_stream,
                                                      unsigned long long *fading_passes, unsigned long long *blended_passes)
{
    if (!b || !n_pairs || !ranges_per_stream || !fading_passes || !blended_passes) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    *n_pairs = b->conv.last_obj_pairs;
    *ranges_per_stream = b->conv.last_obj_ranges;
    *fading_passes = b->conv.last_obj_fading;
    *blended_passes = b->conv.last_obj_blended;
    return OHS_OK;
}

// ---- three directions and two weights per object (libohs_scene3.so; no entry of ohs_hip.h, ohs_scene.h or ohs_scene2.h) ------------
// dir_idx2 and weight2 both NULL: ohsint_batch_process_objects_blend
extern "C" int ohsint_batch_process_objects_blend3(ohs_batch *b, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                                                   size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride,
                                                   size_t n_objects, size_t seg_blocks, const unsigned *dir_idx, const float *obj_gain,
                                                   size_t idx_stride, const unsigned *prev_idx, const float *prev_gain, int switch_mode,
                                                   void *hip_stream, const unsigned *dir_idx1, const float *weight,
                                                   const unsigned *prev_idx1, const float *prev_weight, const unsigned *dir_idx2,
                                                   const float *weight2, const unsigned *prev_idx2, const float *prev_weight2)
{
    return batch_process_objects_any(b, d_in, d_out, n_blocks, in_stream_stride, in_channel_stride, out_stream_stride, out_channel_stride,
                                     n_objects, seg_blocks, dir_idx, obj_gain, idx_stride, prev_idx, prev_gain, switch_mode, hip_stream,
                                     dir_idx1, weight, prev_idx1, prev_weight, dir_idx2, weight2, prev_idx2, prev_weight2);
}

extern "C" int ohsint_batch_last_objects_blend3_launch(const ohs_batch *b, int *n_pairs, int *ranges_per_stream,
                                                       unsigned long long *fading_passes, unsigned long long *blended_passes,
                                                       unsigned long long *blended3_passes)
{
    if (!b || !n_pairs || !ranges_per_stream || !fading_passes || !blended_passes || !blended3_passes)
        return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    *n_pairs = b->conv.last_obj_pairs;
    *ranges_per_stream = b->conv.last_obj_ranges;
    *fading_passes = b->conv.last_obj_fading;
    *blended_passes = b->conv.last_obj_blended;
    *blended3_passes = b->conv.last_obj_blended3;
    return OHS_OK;
}

int ohs_batch_process_deferred(ohs_batch *b, const float *d_in, float *d_out, size_t n_blocks,
                               size_t stream_stride, size_t channel_stride, void *hip_stream)
{
    return batch_process_impl(b, d_in, d_out, n_blocks, stream_stride, channel_stride, hip_stream, true);
}

// Host-buffer batch call (north_star's offline mode fed from host memory).  The frames are cut into time
// chunks; chunk i + 1 is copied in, chunk i processed and chunk i - 1 copied out at the same time, on three
// streams over three device staging slots, so that both directions of the host link and the kernels
// overlap (the 8 B/frame in + 8 B/frame out over PCIe, not the GPU work, is the bound: DESIGN.md section 5).
// Each chunk is one ohs_batch_process call on its slot, in stream order, so per-stream state chains exactly
// as in a sequence of device calls with the same chunk sizes.
int ohs_batch_process_host(ohs_batch *b, const float *h_in, float *h_out, size_t n_blocks,
                           size_t stream_stride, size_t channel_stride, size_t chunk_blocks)
{
    if (!b || !h_in || !h_out) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    if (n_blocks == 0) return OHS_OK;
    if (n_blocks > (size_t)1 << 24) return fail(OHS_ERR_INVALID_ARG, "n_blocks too large");
    const size_t S = b->conv.S;
    if (!batch_strides_ok(S, stream_stride, channel_stride, n_blocks * BS))
        return fail(OHS_ERR_INVALID_ARG, "strides smaller than the processed region");
    HIP_TRY(hipSetDevice(b->device));
    if (chunk_blocks == 0) {
        // default: ~32 MiB per chunk and direction (0.7 ms of link time; 16 ... 64 MiB measure alike, smaller chunks pay
        // per-copy overhead, larger ones a longer fill and drain), at most an eighth of the call so that small batches
        // pipeline too, at least 16 blocks
        const size_t per_block = S * 2 * BS * sizeof(float);
        chunk_blocks = ((size_t)32 << 20) / per_block;
        chunk_blocks = std::min(chunk_blocks, std::max<size_t>(n_blocks / 8, 1));
        chunk_blocks = std::max<size_t>(chunk_blocks, 16);
    }
    chunk_blocks = std::min(chunk_blocks, n_blocks);
    const size_t cf = chunk_blocks * BS;
    if (!b->st_h2d) {
        // The runtime multiplexes streams onto a few hardware queues per PRIORITY level (4 by default,
        // GPU_MAX_HW_QUEUES), and a stream that shares its queue with a copy stream waits behind every chunk
        // copy: with plain streams the convolution launches of chunk i + 1 sat behind the copy-out of chunk i
        // (rocprofv3 --memory-copy-trace: 2.6 ms per chunk instead of 2.1).  The two copy streams therefore get
        // priority levels of their own, where nothing else of this process lives.
        int pr_least = 0, pr_greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest));
        if (tuning().host_pipe_flat_priorities) pr_least = pr_greatest = 0;     // (experiments: the old behaviour)
        // (the pipeline's compute stream too: which normal-priority stream it would share a queue with depends on how
        // many streams the process has created before -- bench.py measured 21.7 or 25.6 ms depending on its step count)
        HIP_TRY(hipStreamCreateWithPriority(&b->st_h2d, hipStreamNonBlocking, pr_greatest));
        HIP_TRY(hipStreamCreateWithPriority(&b->st_comp, hipStreamNonBlocking, pr_greatest));
        HIP_TRY(hipStreamCreateWithPriority(&b->st_d2h, hipStreamNonBlocking, pr_least != 0 ? pr_least : pr_greatest));
        for (int k = 0; k < ohs_batch::kHostSlots; ++k) {
            HIP_TRY(hipEventCreateWithFlags(&b->ev_h2d[k], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&b->ev_comp[k], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&b->ev_d2h[k], hipEventDisableTiming));
        }
    }
    if (cf > b->slot_frames) {
        DeviceWideSection dws;
        HIP_TRY(hipDeviceSynchronize());
        for (int k = 0; k < ohs_batch::kHostSlots; ++k) {
            if (b->d_slot[k]) hipFree(b->d_slot[k]);
            b->d_slot[k] = nullptr;
        }
        b->slot_frames = 0;
        for (int k = 0; k < ohs_batch::kHostSlots; ++k) HIP_TRY(hipMalloc(&b->d_slot[k], S * 2 * cf * sizeof(float)));
        b->slot_frames = cf;
    }
    // one 2-D copy per chunk when the host rows are equally spaced ([stream][channel] with stream_stride ==
    // 2 * channel_stride, or a single stream); else one 2-D copy per stream
    const bool regular = S == 1 || stream_stride == 2 * channel_stride;
    auto copy = [&](bool to_device, float *dev, size_t off, size_t nf, hipStream_t st) -> int {
        const size_t dpitch = b->slot_frames * sizeof(float), w = nf * sizeof(float);
        if (regular) {
            const size_t hpitch = channel_stride * sizeof(float);
            if (to_device)
                HIP_TRY(hipMemcpy2DAsync(dev, dpitch, h_in + off, hpitch, w, S * 2, hipMemcpyHostToDevice, st));
            else
                HIP_TRY(hipMemcpy2DAsync(h_out + off, hpitch, dev, dpitch, w, S * 2, hipMemcpyDeviceToHost, st));
            return OHS_OK;
        }
        for (size_t s_ = 0; s_ < S; ++s_) {
            const size_t hpitch = channel_stride * sizeof(float);
            float *d = dev + s_ * 2 * b->slot_frames;
            if (to_device)
                HIP_TRY(hipMemcpy2DAsync(d, dpitch, h_in + s_ * stream_stride + off, hpitch, w, 2, hipMemcpyHostToDevice, st));
            else
                HIP_TRY(hipMemcpy2DAsync(h_out + s_ * stream_stride + off, hpitch, d, dpitch, w, 2, hipMemcpyDeviceToHost, st));
        }
        return OHS_OK;
    };
    const size_t n_chunks = (n_blocks + chunk_blocks - 1) / chunk_blocks;
    int rc = OHS_OK;
    // Work the caller queued earlier through ohs_batch_process* touches the same per-stream state.  A pending
    // deferred call is joined here (its convolutions run on the handle's own second stream); work on the CALLER's
    // streams cannot be seen from here: the header asks for ohs_batch_sync first.
    if (b->join_pending) {
        HIP_TRY(hipStreamWaitEvent(b->st_comp, b->chunk_done[(size_t)b->chunk_done_n - 1], 0));
        b->join_pending = false;
    }
    // (experiments build, host_pipe_trace: device timestamps around every stage of every chunk, printed after the call;
    // it adds six event records per chunk)
    const bool trace = tuning().host_pipe_trace != 0;
    std::vector<hipEvent_t> tev;
    auto mark = [&](hipStream_t st) {
        if (!trace) return;
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) == hipSuccess) { hipEventRecord(e, st); tev.push_back(e); }
    };
    const auto host_t0 = std::chrono::steady_clock::now();
    std::vector<double> host_ms;
    // inside the loop a HIP failure must not return: the drain below has to run (the copies already queued write
    // into the caller's buffers)
#define PIPE_TRY(x)                                                                                        \
    {                                                                                                      \
        const hipError_t pe_ = (x);                                                                        \
        if (pe_ != hipSuccess) { rc = fail(OHS_ERR_HIP, std::string(#x ": ") + hipGetErrorString(pe_)); break; } \
    }
    for (size_t i = 0; i < n_chunks && rc == OHS_OK; ++i) {
        const int k = (int)(i % ohs_batch::kHostSlots);
        const size_t blk0 = i * chunk_blocks, nb = std::min(chunk_blocks, n_blocks - blk0);
        const size_t off = blk0 * BS, nf = nb * BS;
        if (i >= (size_t)ohs_batch::kHostSlots) PIPE_TRY(hipStreamWaitEvent(b->st_h2d, b->ev_d2h[k], 0))    // slot free again
        mark(b->st_h2d);
        rc = copy(true, b->d_slot[k], off, nf, b->st_h2d);
        if (rc) break;
        mark(b->st_h2d);
        PIPE_TRY(hipEventRecord(b->ev_h2d[k], b->st_h2d))
        PIPE_TRY(hipStreamWaitEvent(b->st_comp, b->ev_h2d[k], 0))
        mark(b->st_comp);
        rc = batch_process_impl(b, b->d_slot[k], b->d_slot[k], nb, 2 * b->slot_frames, b->slot_frames, b->st_comp, false);
        if (rc) break;
        mark(b->st_comp);
        PIPE_TRY(hipEventRecord(b->ev_comp[k], b->st_comp))
        PIPE_TRY(hipStreamWaitEvent(b->st_d2h, b->ev_comp[k], 0))
        mark(b->st_d2h);
        rc = copy(false, b->d_slot[k], off, nf, b->st_d2h);
        if (rc) break;
        mark(b->st_d2h);
        PIPE_TRY(hipEventRecord(b->ev_d2h[k], b->st_d2h))
        if (trace) host_ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count());
    }
#undef PIPE_TRY
    // blocking call: the outputs are complete on return (also on a failure half-way: nothing may still be
    // writing into the caller's buffers)
    const hipError_t e1 = hipStreamSynchronize(b->st_h2d), e2 = hipStreamSynchronize(b->st_comp),
                     e3 = hipStreamSynchronize(b->st_d2h);
    if (trace && !tev.empty()) {
        fprintf(stderr, "[ohs host pipeline] %zu chunks of %zu blocks; per chunk [ms since the first copy began]: "
                        "h2d begin-end | kernels begin-end | d2h begin-end | host enqueued at\n", n_chunks, chunk_blocks);
        for (size_t i = 0; i + 5 < tev.size(); i += 6) {
            float t[6];
            for (int j = 0; j < 6; ++j) if (hipEventElapsedTime(&t[j], tev[0], tev[i + j]) != hipSuccess) t[j] = -1.f;
            fprintf(stderr, "  %2zu: %6.2f-%6.2f | %6.2f-%6.2f | %6.2f-%6.2f | %6.2f\n", i / 6, t[0], t[1], t[2], t[3], t[4], t[5],
                    i / 6 < host_ms.size() ? host_ms[i / 6] : -1.0);
        }
        for (hipEvent_t e : tev) hipEventDestroy(e);
    }
    // Fail closed (ohs_batch_reset's contract): a copy, an event or a wait that failed with chunks already processed leaves
    // the per-stream state advanced for some chunks only -- exactly like a failure inside ohs_batch_process, which has
    // marked the handle itself.  (Argument errors were found before the loop: nothing was queued.)
    if (rc && rc != OHS_ERR_INVALID_ARG && !b->failed) return batch_mark_failed(b, rc);
    if (rc) return rc;
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
        b->failed = true;
        b->fail_msg = "host pipeline: stream sync failed";
        return fail(OHS_ERR_HIP, b->fail_msg);
    }
    return OHS_OK;
}

int ohs_batch_join(ohs_batch *b, void *hip_stream)
{
    if (!b) return fail(OHS_ERR_INVALID_ARG, "batch is NULL");
    if (!b->join_pending) return OHS_OK;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamWaitEvent((hipStream_t)hip_stream, b->chunk_done[(size_t)b->chunk_done_n - 1], 0));
    b->join_pending = false;
    return OHS_OK;
}

int ohs_batch_set_profiling(ohs_batch *b, int enable)
{
    if (!b) return fail(OHS_ERR_INVALID_ARG, "batch is NULL");
    b->profiling = enable != 0;
    HIP_TRY(hipSetDevice(b->device));
    if (b->profiling && !b->eq.d_stamps) {
        HIP_TRY(hipMalloc(&b->eq.d_stamps, 4 * sizeof(unsigned long long)));
        HIP_TRY(hipMemset(b->eq.d_stamps, 0, 4 * sizeof(unsigned long long)));
    } else if (!b->profiling && b->eq.d_stamps) {
        DeviceWideSection dws;
        HIP_TRY(hipDeviceSynchronize());        // (a launch in flight may still write them)
        hipFree(b->eq.d_stamps);
        b->eq.d_stamps = nullptr;
    }
    return OHS_OK;
}

int ohs_batch_profile_eq_clock(ohs_batch *b, double *shader_ghz, double *wave_us)
{
    if (!b || !shader_ghz || !wave_us) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    *shader_ghz = 0.0; *wave_us = 0.0;
    if (!b->eq.d_stamps) return fail(OHS_ERR_INVALID_ARG, "profiling is off (ohs_batch_set_profiling)");
    HIP_TRY(hipSetDevice(b->device));
    unsigned long long s[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpy(s, b->eq.d_stamps, sizeof(s), hipMemcpyDeviceToHost));     // (synchronous: waits for the device)
    if (s[1] <= s[0] || s[3] <= s[2]) return fail(OHS_ERR_INVALID_ARG, "no ring-form EQ launch has run with profiling on");
    *wave_us = (double)(s[1] - s[0]) / 100.0;                                   // s_memrealtime: 100 MHz
    *shader_ghz = (double)(s[3] - s[2]) / ((double)(s[1] - s[0]) * 10.0);       // shader clocks per 10 ns
    return OHS_OK;
}

int ohs_batch_profile_read(ohs_batch *b, double *eq_ms, double *conv_ms, uint64_t *n_calls,
                           uint64_t *eq_launches, uint64_t *conv_launches)
{
    if (!b || !eq_ms || !conv_ms || !n_calls || !eq_launches || !conv_launches)
        return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(b->device));
    double t[2] = {0.0, 0.0};
    uint64_t cntk[2] = {0, 0};
    hipError_t bad = hipSuccess;
    for (auto &sp : b->spans) {
        cntk[sp.kind]++;
        float ms = 0.f;
        hipError_t e = hipEventSynchronize(sp.b);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, sp.a, sp.b);
        if (e != hipSuccess) {
            // an event that cannot be timed: it does not go back to the pool, and the spans are dropped all the same --
            // one bad span must not make every later read fail
            if (bad == hipSuccess) bad = e;
            hipEventDestroy(sp.a);
            hipEventDestroy(sp.b);
            continue;
        }
        t[sp.kind] += ms;
        b->ev_pool.push_back(sp.a);
        b->ev_pool.push_back(sp.b);
    }
    b->spans.clear();
    if (bad != hipSuccess) {
        b->prof_calls = 0;
        return fail(OHS_ERR_HIP, std::string("profile_read: a span's events could not be timed (") + hipGetErrorString(bad) +
                                     "); the spans recorded so far were dropped");
    }
    *eq_ms = t[0]; *conv_ms = t[1]; *n_calls = b->prof_calls;
    *eq_launches = cntk[0]; *conv_launches = cntk[1];
    b->prof_calls = 0;
    return OHS_OK;
}

int ohs_batch_sync(ohs_batch *b, void *hip_stream)
{
    if (!b) return fail(OHS_ERR_INVALID_ARG, "batch is NULL");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
    if (b->join_pending) {
        HIP_TRY(hipStreamSynchronize(b->st2));
        b->join_pending = false;
    }
    return OHS_OK;
}

int ohs_batch_algorithmic_bytes(const ohs_batch *b, size_t n_blocks, uint64_t *bytes)
{
    if (!b || !bytes) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    // SURVEY.md section 8d / DESIGN.md byte model, per 512-frame block per stream:
    //   audio in 4096 + out 4096, history write 2*4104, history read 2*(P-1)*4104,
    //   overlap read+write 2*(2048+2048), EQ state + coefficients ~520 (if EQ on),
    //   HRIR spectra 4*P*4104 once per block-time, shared by all streams.
    int P = 1;
    for (int p = 0; p < 4; ++p) P = std::max(P, b->conv.P[p]);
    const uint64_t per_stream_block = 4096u + 4096u + 2u * 4104u + 2u * (uint64_t)(P - 1) * 4104u +
                                      2u * (2048u + 2048u) + (b->eq_enable ? 520u : 0u);
    const uint64_t shared_per_block = 4u * (uint64_t)P * 4104u;
    *bytes = (uint64_t)n_blocks * ((uint64_t)b->conv.S * per_stream_block + shared_per_block);
    return OHS_OK;
}

int ohs_batch_kernel_bytes(const ohs_batch *b, size_t n_blocks, uint64_t *eq_bytes, uint64_t *conv_bytes)
{
    if (!b || !eq_bytes || !conv_bytes) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    int P = 1;
    for (int p = 0; p < 4; ++p) P = std::max(P, b->conv.P[p]);
    const uint64_t S = b->conv.S, nbk = n_blocks;
    // DESIGN bytes: what the kernels are built to move through HBM for one call of n_blocks (tables and ring
    // re-reads that are served by L2 are not counted).  This is NOT the SURVEY 8d per-block model
    // (ohs_batch_algorithmic_bytes): the P = 1 kernel keeps overlaps in registers and writes no history.
    //   EQ:             audio in + out, state + coefficients
    //   P = 1, block 512: audio in + out; per stream and chunk boundary the input block in front of it once more (4 KiB;
    //                   where the pre-pass computes the boundary tails, K not in {2, 4, 8, 16}: the tail written and read
    //                   as well) and the four-overlap state (8 KiB in + 8 KiB out)
    //   P > 1 (time-parallel): audio in, ring write, ring read once, W write, W read, audio out
    const uint64_t eq_sb = 4096u + 4096u + 520u;
    *eq_bytes = b->eq_enable ? nbk * S * eq_sb : 0;
    const bool os_plan = P == 1 && b->conv.lazy_ok &&
                         (b->conv.conv_plan == 2 ||
                          (b->conv.conv_plan == 0 && conv_plan_auto_is_os((size_t)S, (long long)nbk, b->eq_enable != 0)));   // (EQ on: in place)
    if (os_plan) {
        // hop-1536 plan: audio in + out; per stream the 512 frames in front of every hop range but the first once more
        // (4 KiB each), the merged overlap in + out and the last input block (3 x 4 KiB)
        const uint64_t K = (uint64_t)conv_os_chunks(b->ctx, (size_t)S, (long long)nbk, b->eq_enable != 0);
        *conv_bytes = nbk * S * 8192u + S * ((K - 1) * 4096u + 3u * 4096u);
    } else if (P == 1) {
        const uint64_t K = (uint64_t)conv_p1_chunks(b->ctx, (size_t)S, (long long)nbk, 0);
        const bool own_tails = conv_p1_waves_per_cu() == 16 && (K == 2 || K == 4 || K == 8 || K == 16);
        // state: per-path overlaps 8 KiB in + 8 KiB out, or (lazy, kernels.h) merged overlap 4 KiB in + 4 KiB out + the
        // last block's input copy 4 KiB
        const uint64_t state = b->conv.lazy_ok ? 3u * 4096u : 2u * 8192u;
        *conv_bytes = nbk * S * 8192u + S * ((K - 1) * (own_tails ? 1u : 3u) * 4096u + state);
    } else if (b->conv.d_xhist && P >= lb_min_p() &&
               (b->conv.conv_plan == 2 || (b->conv.conv_plan == 0 && conv_plan_auto_is_lb((size_t)S, (long long)nbk, P)))) {
        if (!b->eq_enable && conv_plan_auto_is_xb((size_t)S, (long long)nbk, P)) {
            // block-8192 kernel (EQ off: taken to be out of place, as the hop-1536 rule above does): audio in + out; per run of
            // blocks the window's first half once more (64 KiB), with two partitions the carry's window as well; the history append
            const int P2x = (P + 15) / 16;
            const uint64_t n_blk = (nbk * 512u + 8191u) / 8192u;
            const uint64_t run = (uint64_t)conv_xb_run_for((int)S, (int)n_blk, P2x, b->ctx->num_cus);
            *conv_bytes = nbk * S * 8192u + S * ((n_blk + run - 1) / run) * (uint64_t)P2x * 65536u + 2u * S * 2u * (uint64_t)b->conv.xh_len * 4u;
            return OHS_OK;
        }
        // block-2048 plan: audio in, ring write (16 B per frame), ring read once, audio out -- the product never leaves the
        // chip; plus the input history copied once per segment (read + write)
        *conv_bytes = nbk * S * (4096u + 8192u + 8192u + 4096u) + 2u * S * 2u * (uint64_t)b->conv.xh_len * 4u;
    } else {
        *conv_bytes = nbk * S * (4096u + 8192u + 8192u + 8192u + 8192u + 4096u);
    }
    return OHS_OK;
}


int ohs_batch_set_speakers(ohs_batch *b, const ohs_sofa *sofa, float az_l, float el_l, float az_r, float el_r,
                           float radius_m, float fs, unsigned *changed_mask)
{
    if (!b) return fail(OHS_ERR_INVALID_ARG, "batch is NULL");
    return set_speakers_impl(b->conv, sofa, az_l, el_l, az_r, el_r, radius_m, fs, changed_mask,
                             [&](int p, const float *ir, size_t n) { return ohs_batch_set_ir(b, p, ir, n); });
}

}  // extern "C"
