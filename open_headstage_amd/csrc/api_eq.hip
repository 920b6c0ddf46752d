// api_eq.hip -- the EQ table / state of a handle (EqState), ohs_eq_* (StereoParametricEQ, parametric_eq.rs:125-209)
// and ohs_biquad_* (BiquadFilter as a type of its own, parametric_eq.rs:46-123).
#include "api_internal.h"
#include <map>

using namespace ohs;
using namespace ohs_api;
using ohs_host::rbj;

namespace ohs_api {


int eq_init(EqState &e, size_t nb, size_t chains, float fs, hipStream_t st)
{
    if (nb > OHS_MAX_EQ_BANDS) return fail(OHS_ERR_INVALID_ARG, "num_bands > OHS_MAX_EQ_BANDS");
    e.nb = nb; e.chains = chains;
    e.coeffs.assign(nb * 5, 0.0f);
    e.en.assign(nb, 0);
    float c[5];
    int rc = rbj(OHS_FILTER_PEAK, fs, 20.0f, 0.707f, 0.0f, c);   // parametric_eq.rs:63-76
    if (rc) return rc;
    for (size_t b = 0; b < nb; ++b) std::memcpy(&e.coeffs[5 * b], c, sizeof(c));
    const size_t n = chains * (size_t)kEqStateSlots * 2;
    HIP_TRY(hipMalloc(&e.d_state, n * sizeof(float)));
    HIP_TRY(hipMemsetAsync(e.d_state, 0, n * sizeof(float), st));
    return OHS_OK;
}

int eq_reset(EqState &e, hipStream_t st)
{
    const size_t n = e.chains * (size_t)kEqStateSlots * 2;
    HIP_TRY(hipMemsetAsync(e.d_state, 0, n * sizeof(float), st));
    return OHS_OK;
}

// The enabled bands of one table (coeffs [nb][5]; flags en8, or en32 where en8 is NULL) from band `start` on, in cascade order
// and at most `cap` of them, as a pass table; -> how many it holds.  *next (optional): the first band not looked at.
static int eq_compact_pass(size_t nb, const float *coeffs, const unsigned char *en8, const int *en32, size_t start, int cap,
                           EqPassTable &t, size_t *next)
{
    std::memset(&t, 0, sizeof(t));
    int k = 0;
    size_t b = start, last = 0;
    for (; b < nb && k < cap; ++b) {
        if (en8 ? en8[b] == 0 : en32[b] == 0) continue;
        t.slot[k] = (int)b;
        t.b0[k] = coeffs[5 * b + 0]; t.b1[k] = coeffs[5 * b + 1]; t.b2[k] = coeffs[5 * b + 2];
        t.a1[k] = coeffs[5 * b + 3]; t.a2[k] = coeffs[5 * b + 4];
        last = b;
        ++k;
    }
    for (int j = k; j < 16; ++j) t.slot[j] = (int)last;     // unused lanes shadow the last band's slot (never stored)
    if (next) *next = b;
    return k;
}

// the enabled bands, in cascade order, as ONE pass table; returns their number (the caller checks <= 16 / <= 12)
int eq_single_pass_table(const EqState &e, EqPassTable &t)
{
    size_t next = 0;
    int nbp = eq_compact_pass(e.nb, e.coeffs.data(), nullptr, e.en.data(), 0, 16, t, &next);
    for (size_t b = next; b < e.nb; ++b) nbp += e.en[b] != 0;
    return nbp;
}

// the XCDs the EQ's ring launches may use: the handle's (set per call by the batch), or the tuning's override
static std::pair<int, int> eq_xcds(const EqState &e)
{
    if (tuning().eq_xcd_n > 0) return {tuning().eq_xcd_lo, tuning().eq_xcd_n};
    return {e.xcd_lo, e.xcd_n};
}

// the ring forms (one launch for all streams, tables in device memory) may serve these frames
static bool eq_ring_forms_serve(const EqState &e, long long ss, long long cs, long long n)
{
    return !e.exact_specials && !tuning().eq_conveyor && eq_ring_addressable(ss, cs, n);
}

// the scheduled kernels (k_eq_ring_sched, k_eq_ring_sched_streams: the wave ring, 32-bit sample counts per segment) may serve
// n frames of a schedule whose tables have n_bands enabled bands
static bool eq_sched_kernel_serves(const EqState &e, const BatchSchedule &sc, long long ss, long long cs, long long n, size_t n_bands)
{
    return sc.seg_blocks * BS < ((size_t)1 << 30) && eq_pass_takes_wave_ring(ss, cs, n, (int)e.chains, (int)n_bands, e.exact_specials);
}

// identity: the frames of `chains` chains still have to arrive in `out`
static int eq_copy_through(const float *in, float *out, long long ss, long long cs, long long n, size_t chains, hipStream_t st)
{
    if (out == in) return OHS_OK;
    if (chains == 2 || ss == 2 * cs) {
        HIP_TRY(hipMemcpy2DAsync(out, (size_t)cs * sizeof(float), in, (size_t)cs * sizeof(float), (size_t)n * sizeof(float), chains,
                                 hipMemcpyDeviceToDevice, st));
        return OHS_OK;
    }
    for (size_t s = 0; s < chains / 2; ++s)
        HIP_TRY(hipMemcpy2DAsync(out + (long long)s * ss, (size_t)cs * sizeof(float), in + (long long)s * ss, (size_t)cs * sizeof(float),
                                 (size_t)n * sizeof(float), 2, hipMemcpyDeviceToDevice, st));
    return OHS_OK;
}

void eq_free(EqState &e)
{
    if (e.d_state) hipFree(e.d_state);
    if (e.d_stabs) hipFree(e.d_stabs);
    if (e.d_stamps) hipFree(e.d_stamps);
    if (e.d_sched_lanes) hipFree(e.d_sched_lanes);
    if (e.d_sched_stabs) hipFree(e.d_sched_stabs);
    if (e.d_sched_gather) hipFree(e.d_sched_gather);
    e.d_state = nullptr; e.d_stabs = nullptr; e.stabs_passes = 0; e.d_stamps = nullptr; e.d_sched_lanes = nullptr; e.sched_n = 0;
    e.d_sched_stabs = nullptr; e.d_sched_gather = nullptr; e.sched_passes = 0;
}

bool eq_any_enabled(const EqState &e)
{
    if (e.per_stream) {
        for (unsigned char v : e.s_en)
            if (v) return true;
        return false;
    }
    for (size_t i = 0; i < e.nb; ++i)
        if (e.en[i]) return true;
    return false;
}

void eq_set_shared_band(EqState &e, size_t band, const float coeffs[5], int enabled)
{
    std::memcpy(&e.coeffs[5 * band], coeffs, 5 * sizeof(float));
    e.en[band] = enabled != 0;
    if (e.per_stream) {         // the shared call sets the band of EVERY stream
        const size_t S = e.chains / 2;
        for (size_t s = 0; s < S; ++s) {
            std::memcpy(&e.s_coeffs[(s * e.nb + band) * 5], coeffs, 5 * sizeof(float));
            e.s_en[s * e.nb + band] = enabled != 0;
        }
        e.stabs_dirty = true;
    }
}

int eq_set_stream_band(EqState &e, size_t stream, size_t band, const float coeffs[5], int enabled)
{
    const size_t S = e.chains / 2;
    if (stream >= S) return fail(OHS_ERR_INVALID_ARG, "stream index out of range");
    if (band >= e.nb) return OHS_OK;            // parametric_eq.rs:144-164 ignores a band index past the last one
    if (!e.per_stream) {                        // every stream starts from the shared table
        e.s_coeffs.resize(S * e.nb * 5);
        e.s_en.resize(S * e.nb);
        for (size_t s = 0; s < S; ++s) {
            std::memcpy(&e.s_coeffs[s * e.nb * 5], e.coeffs.data(), e.nb * 5 * sizeof(float));
            for (size_t b = 0; b < e.nb; ++b) e.s_en[s * e.nb + b] = e.en[b] != 0;
        }
        e.per_stream = true;
    }
    std::memcpy(&e.s_coeffs[(stream * e.nb + band) * 5], coeffs, 5 * sizeof(float));
    e.s_en[stream * e.nb + band] = enabled != 0;
    e.stabs_dirty = true;
    return OHS_OK;
}

void eq_share_table(EqState &e)
{
    e.per_stream = false;
    e.s_coeffs.clear(); e.s_coeffs.shrink_to_fit();
    e.s_en.clear(); e.s_en.shrink_to_fit();
    e.stabs_dirty = true;
}

// the cascade of ONE table (coeffs [nb][5], en [nb]) over n frames of `chains` chains: enabled bands only, in cascade order,
// 16 per pass; a disabled band is the identity and keeps its state (parametric_eq.rs:118-120), so it is simply not given
// a lane.  ev_start / ev_stop (optional): recorded at the start of the first and the completion of the last pass
static int eq_launch_table(EqState &e, const float *coeffs, const unsigned char *en8, const int *en32, size_t chains,
                           float *d_state, const float *in, float *out, long long ss, long long cs, long long n,
                           hipStream_t st, bool *did_anything, hipEvent_t ev_start, hipEvent_t ev_stop)
{
    const auto [xcd_lo, xcd_n] = eq_xcds(e);
    const float *src = in;
    EqPassTable t, t_next;
    size_t next = 0;
    int nbp = eq_compact_pass(e.nb, coeffs, en8, en32, 0, 16, t, &next);
    if (did_anything) *did_anything = nbp > 0;
    for (bool first = true; nbp > 0; first = false) {
        const int nbp_next = eq_compact_pass(e.nb, coeffs, en8, en32, next, 16, t_next, &next);     // (none: this pass is the last)
        hipError_t err = launch_eq_pass(src, out, ss, cs, n, (int)chains, t, nbp, d_state, st, e.exact_specials, e.fp_mode, xcd_lo, xcd_n,
                                        first ? ev_start : nullptr, nbp_next == 0 ? ev_stop : nullptr, e.d_stamps, &e.last_form);
        if (err != hipSuccess) return fail(OHS_ERR_HIP, std::string("eq launch: ") + hipGetErrorString(err));
        e.last_scheduled = false;
        src = out;
        t = t_next;
        nbp = nbp_next;
    }
    return OHS_OK;
}

// per-stream tables: compact every stream's enabled bands into EqStreamTables of 12 and upload them: pass k of stream s, at
// d_stabs[k * S + s], holds that stream's enabled bands 12 k .. 12 k + 11 (none: nb = 0, the pass hands the samples on).  Not on
// the audio path: it waits for what the stream has queued (a launch in flight may still be reading the old tables) and copies
// synchronously.
static int eq_upload_stream_tables(EqState &e, hipStream_t st)
{
    const size_t S = e.chains / 2;
    size_t mx = 0;
    for (size_t s = 0; s < S; ++s) {
        size_t count = 0;
        for (size_t b = 0; b < e.nb; ++b) count += e.s_en[s * e.nb + b] ? 1 : 0;
        mx = std::max(mx, count);
    }
    const size_t passes = std::max<size_t>(1, (mx + 11) / 12);
    std::vector<EqStreamTable> tabs(passes * S);
    std::memset(tabs.data(), 0, tabs.size() * sizeof(EqStreamTable));
    for (size_t s = 0; s < S; ++s) {
        size_t count = 0;
        for (size_t b = 0; b < e.nb; ++b) {
            if (!e.s_en[s * e.nb + b]) continue;
            EqStreamTable &t = tabs[(count / 12) * S + s];
            const int k = (int)(count % 12);
            const float *c = &e.s_coeffs[(s * e.nb + b) * 5];
            t.b0[k] = c[0]; t.b1[k] = c[1]; t.b2[k] = c[2]; t.a1[k] = c[3]; t.a2[k] = c[4];
            t.slot[k] = (int)b;
            t.nb = k + 1;
            ++count;
        }
        for (size_t pk = 0; pk < passes; ++pk) {        // unused entries repeat the pass's last band's slot (never stored)
            EqStreamTable &t = tabs[pk * S + s];
            for (int j = t.nb; j < 12; ++j) t.slot[j] = t.nb ? t.slot[t.nb - 1] : 0;
        }
    }
    e.max_enabled = mx;
    DeviceWideSection dws;
    HIP_TRY(hipStreamSynchronize(st));
    if (!e.d_stabs || e.stabs_passes < passes) {
        if (e.d_stabs) hipFree(e.d_stabs);
        e.d_stabs = nullptr; e.stabs_passes = 0;
        HIP_TRY(hipMalloc(&e.d_stabs, passes * S * sizeof(EqStreamTable)));
        e.stabs_passes = passes;
    }
    HIP_TRY(hipMemcpy(e.d_stabs, tabs.data(), passes * S * sizeof(EqStreamTable), hipMemcpyHostToDevice));
    e.stabs_dirty = false;
    return OHS_OK;
}

// Stream s of (in, out) alone under the table (coeffs [nb][5], en8 [nb]): the conveyor kernel takes its table as a kernel
// argument, so where the ring forms cannot serve, every stream is a launch sequence of its own (correct for any table; an
// offline job that needs this at scale groups its streams by table and uses one batch per group).  A stream without an enabled
// band is copied through.  *did becomes true where anything was queued.
static int eq_launch_stream(EqState &e, size_t s, const float *coeffs, const unsigned char *en8, const float *in, float *out,
                            long long ss, long long cs, long long n, hipStream_t st, bool *did)
{
    bool launched = false;
    const float *si = in + (long long)s * ss;
    float *so = out + (long long)s * ss;
    int rc = eq_launch_table(e, coeffs, en8, nullptr, 2, e.d_state + s * 2 * (size_t)kEqStateSlots * 2, si, so, ss, cs, n, st, &launched,
                             nullptr, nullptr);
    if (rc == OHS_OK && !launched) rc = eq_copy_through(si, so, ss, cs, n, 2, st);
    if (did) *did = *did || launched || so != si;
    return rc;
}

// run the cascade over n frames of `chains` chains, in place allowed
int eq_launch(EqState &e, const float *in, float *out, long long ss, long long cs, long long n,
              hipStream_t st, bool *did_anything, hipEvent_t ev_start, hipEvent_t ev_stop)
{
    bool did = false;
    int rc = OHS_OK;
    if (!e.per_stream) {
        rc = eq_launch_table(e, e.coeffs.data(), nullptr, e.en.data(), e.chains, e.d_state, in, out, ss, cs, n, st, &did,
                             ev_start, ev_stop);
        if (rc) return rc;
    } else {
        if (e.stabs_dirty) {
            rc = eq_upload_stream_tables(e, st);
            if (rc) return rc;
        }
        if (e.max_enabled == 0) {
            // no stream has an enabled band: identity
        } else if (eq_ring_forms_serve(e, ss, cs, n)) {
            // one launch per 12 bands for all streams: every row reads its own stream's table when its wave starts (a stream with
            // fewer bands than the pass's first hands its samples on -- exact except for -0.0, as the ring form's spare lanes are)
            const auto [xcd_lo, xcd_n] = eq_xcds(e);
            const size_t S = e.chains / 2, passes = (e.max_enabled + 11) / 12;
            for (size_t pk = 0; pk < passes; ++pk) {
                hipError_t err = launch_eq_ring_streams(pk ? out : in, out, ss, cs, n, (int)e.chains, e.d_stabs + pk * S, e.d_state, st,
                                                        e.fp_mode, xcd_lo, xcd_n, pk == 0 ? ev_start : nullptr,
                                                        pk + 1 == passes ? ev_stop : nullptr, &e.last_form);
                e.last_scheduled = false;
                if (err != hipSuccess) return fail(OHS_ERR_HIP, std::string("eq launch (per-stream tables): ") + hipGetErrorString(err));
            }
            did = true;
        } else {
            // The exact-specials mode, strides beyond the ring form's reach: every stream is a launch sequence of its own
            // (eq_launch_stream).
            if (ev_start) HIP_TRY(hipEventRecord(ev_start, st));
            for (size_t s = 0; s < e.chains / 2; ++s) {
                rc = eq_launch_stream(e, s, &e.s_coeffs[s * e.nb * 5], &e.s_en[s * e.nb], in, out, ss, cs, n, st, &did);
                if (rc) return rc;
            }
            if (ev_stop) HIP_TRY(hipEventRecord(ev_stop, st));
            if (did_anything) *did_anything = did;
            return OHS_OK;
        }
    }
    if (!did) {     // no enabled band: the events mark this point of the stream
        if (ev_start) HIP_TRY(hipEventRecord(ev_start, st));
        if (ev_stop) HIP_TRY(hipEventRecord(ev_stop, st));
    }
    if (did_anything) *did_anything = did;
    return OHS_OK;
}

// ---- schedule tables (ohs_batch_set_schedule_tables / ohs_batch_process_scheduled) ------------------------------------------
// Not on the audio path: waits for what the stream has queued (a launch in flight may still read the old lane tables).
int eq_set_schedule_tables(EqState &e, size_t n_tables, const float *coeffs, const uint8_t *enabled, hipStream_t st)
{
    DeviceWideSection dws;
    HIP_TRY(hipDeviceSynchronize());
    if (e.d_sched_lanes) hipFree(e.d_sched_lanes);
    if (e.d_sched_stabs) hipFree(e.d_sched_stabs);
    if (e.d_sched_gather) hipFree(e.d_sched_gather);
    e.d_sched_lanes = nullptr; e.sched_n = 0;
    e.d_sched_stabs = nullptr; e.d_sched_gather = nullptr; e.sched_passes = 0;
    e.sched_coeffs.clear(); e.sched_en.clear(); e.sched_on.clear(); e.sched_class.clear();
    if (n_tables == 0) return OHS_OK;
    e.sched_coeffs.assign(coeffs, coeffs + n_tables * e.nb * 5);
    e.sched_en.assign(enabled, enabled + n_tables * e.nb);
    for (unsigned char &v : e.sched_en) v = v != 0;
    // lane constants per table: lane l is pre lane of enabled band l and post lane of enabled band l - 1 (eq_ring64_body.hpp)
    std::vector<float> lanes(n_tables * 5 * 16);
    for (size_t t = 0; t < n_tables; ++t) {
        float *L = &lanes[t * 5 * 16];
        for (int l = 0; l < 16; ++l) { L[l] = 1.0f; L[16 + l] = 0.0f; L[32 + l] = 0.0f; L[48 + l] = 0.0f; L[64 + l] = 0.0f; }
        std::vector<size_t> on;
        for (size_t b = 0; b < e.nb; ++b)
            if (e.sched_en[t * e.nb + b]) on.push_back(b);
        if (on.empty() || on.size() > 12) continue;
        for (size_t j = 0; j < on.size(); ++j) {
            const float *c = &e.sched_coeffs[(t * e.nb + on[j]) * 5];
            L[j] = c[0]; L[16 + j] = c[1];
            L[32 + j + 1] = c[2]; L[48 + j + 1] = c[3]; L[64 + j + 1] = c[4];
        }
    }
    HIP_TRY(hipMalloc(&e.d_sched_lanes, lanes.size() * sizeof(float)));
    HIP_TRY(hipMemcpy(e.d_sched_lanes, lanes.data(), lanes.size() * sizeof(float), hipMemcpyHostToDevice));
    // for the per-stream scheduled call: band counts, flag classes, and every table as EqStreamTables of 12 bands per pass
    // (eq_upload_stream_tables' compaction, per table instead of per stream)
    e.sched_on.assign(n_tables, 0);
    e.sched_class.assign(n_tables, 0);
    {
        std::map<std::vector<unsigned char>, unsigned> classes;
        size_t mx = 0;
        for (size_t t = 0; t < n_tables; ++t) {
            const std::vector<unsigned char> fl(e.sched_en.begin() + (long)(t * e.nb), e.sched_en.begin() + (long)((t + 1) * e.nb));
            e.sched_class[t] = classes.emplace(fl, (unsigned)classes.size()).first->second;
            size_t on = 0;
            for (unsigned char v : fl) on += v;
            e.sched_on[t] = (unsigned char)on;         // (nb <= OHS_MAX_EQ_BANDS = 64)
            mx = std::max(mx, on);
        }
        const size_t passes = std::max<size_t>(1, (mx + 11) / 12), S = e.chains / 2;
        std::vector<EqStreamTable> tabs(passes * n_tables);
        std::memset(tabs.data(), 0, tabs.size() * sizeof(EqStreamTable));
        for (size_t t = 0; t < n_tables; ++t) {
            size_t count = 0;
            for (size_t b = 0; b < e.nb; ++b) {
                if (!e.sched_en[t * e.nb + b]) continue;
                EqStreamTable &T = tabs[(count / 12) * n_tables + t];
                const int k = (int)(count % 12);
                const float *c = &e.sched_coeffs[(t * e.nb + b) * 5];
                T.b0[k] = c[0]; T.b1[k] = c[1]; T.b2[k] = c[2]; T.a1[k] = c[3]; T.a2[k] = c[4];
                T.slot[k] = (int)b;
                T.nb = k + 1;
                ++count;
            }
            for (size_t pk = 0; pk < passes; ++pk) {        // unused entries repeat the pass's last band's slot (never stored)
                EqStreamTable &T = tabs[pk * n_tables + t];
                for (int j = T.nb; j < 12; ++j) T.slot[j] = T.nb ? T.slot[T.nb - 1] : 0;
            }
        }
        HIP_TRY(hipMalloc(&e.d_sched_stabs, tabs.size() * sizeof(EqStreamTable)));
        HIP_TRY(hipMemcpy(e.d_sched_stabs, tabs.data(), tabs.size() * sizeof(EqStreamTable), hipMemcpyHostToDevice));
        HIP_TRY(hipMalloc(&e.d_sched_gather, passes * S * sizeof(EqStreamTable)));
        HIP_TRY(hipMemset(e.d_sched_gather, 0, passes * S * sizeof(EqStreamTable)));
        e.sched_passes = passes;
    }
    e.sched_n = n_tables;
    (void)st;
    return OHS_OK;
}

bool eq_schedule_table_any_enabled(const EqState &e, size_t table)
{
    for (size_t b = 0; b < e.nb; ++b)
        if (e.sched_en[table * e.nb + b]) return true;
    return false;
}

// Blocks [blk0, blk0 + n_blocks) of a scheduled call.  Consecutive segments with one table index are a RUN.  Consecutive runs
// whose tables have the same enabled flags (1 .. 12 of them) are ONE launch of k_eq_ring_sched where launch_eq_pass would take
// the wave ring for those frames: the coefficients change inside the kernel.  Everything else -- a change of the flags (the
// lanes' roles change; state travels through the state slots, a disabled band's stays frozen in its slot), the row form, the
// conveyor form, more than 12 bands, launches under 8 192 samples -- is one plain launch sequence per run with that run's table,
// exactly what the per-segment call loop launches.  A lone run is the plain call's launch.
int eq_launch_scheduled(EqState &e, const BatchSchedule &sc, size_t blk0, size_t n_blocks, const float *in, float *out,
                        long long ss, long long cs, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop)
{
    struct Run { size_t b0, b1; unsigned tab; };
    std::vector<Run> runs;
    for (size_t blk = blk0; blk < blk0 + n_blocks;) {
        const size_t seg = blk / sc.seg_blocks;
        const size_t end = std::min(blk0 + n_blocks, (seg + 1) * sc.seg_blocks);
        const unsigned t = sc.tab[seg];
        if (!runs.empty() && runs.back().tab == t) runs.back().b1 = end;
        else runs.push_back({blk, end, t});
        blk = end;
    }
    auto same_flags = [&](unsigned a, unsigned b) {
        return std::memcmp(&e.sched_en[a * e.nb], &e.sched_en[b * e.nb], e.nb) == 0;
    };
    auto count_on = [&](unsigned t) {
        size_t k = 0;
        for (size_t b = 0; b < e.nb; ++b) k += e.sched_en[t * e.nb + b];
        return k;
    };
    // groups of runs with equal flags
    struct Group { size_t r0, r1; };
    std::vector<Group> groups;
    for (size_t r = 0; r < runs.size(); ++r) {
        if (!groups.empty() && same_flags(runs[groups.back().r0].tab, runs[r].tab)) groups.back().r1 = r + 1;
        else groups.push_back({r, r + 1});
    }
    // the events ride in the dispatch when the chunk is exactly one kernel launch sequence (as the plain call's); else around
    const bool single = groups.size() == 1 && count_on(runs[0].tab) > 0 &&
                        (groups[0].r1 - groups[0].r0 == 1 ||
                         eq_sched_kernel_serves(e, sc, ss, cs, (long long)n_blocks * BS, count_on(runs[0].tab)));
    if (!single && ev_start) HIP_TRY(hipEventRecord(ev_start, st));
    for (const Group &g : groups) {
        const unsigned t0 = runs[g.r0].tab;
        const size_t on = count_on(t0);
        const size_t gb0 = runs[g.r0].b0, gb1 = runs[g.r1 - 1].b1;
        const long long off = (long long)(gb0 - blk0) * BS, n = (long long)(gb1 - gb0) * BS;
        if (on == 0) {
            int rc = eq_copy_through(in + off, out + off, ss, cs, n, e.chains, st);
            if (rc) return rc;
            continue;
        }
        if (g.r1 - g.r0 > 1 && eq_sched_kernel_serves(e, sc, ss, cs, n, on)) {
            EqPassTable t;      // (at most 12 bands: the wave ring's)
            const int nbp = eq_compact_pass(e.nb, &e.sched_coeffs[(size_t)t0 * e.nb * 5], &e.sched_en[(size_t)t0 * e.nb], nullptr, 0, 12, t, nullptr);
            EqRingSched sch;
            sch.lane_tabs = e.d_sched_lanes; sch.seg_tab = sc.d_tab; sch.n_segs = (int)sc.n_segs;
            sch.seg_len = (int)(sc.seg_blocks * BS);
            sch.seg0 = (int)(gb0 / sc.seg_blocks); sch.off0 = (int)((gb0 % sc.seg_blocks) * BS);
            const auto [xcd_lo, xcd_n] = eq_xcds(e);
            hipError_t err = launch_eq_ring_sched(in + off, out + off, ss, cs, n, (int)e.chains, t, nbp, e.d_state, sch, st, e.fp_mode,
                                                  xcd_lo, xcd_n, single ? ev_start : nullptr, single ? ev_stop : nullptr, e.d_stamps);
            if (err != hipSuccess) return fail(OHS_ERR_HIP, std::string("eq launch (scheduled): ") + hipGetErrorString(err));
            e.last_form = OHS_EQ_FORM_WAVE_RING;
            e.last_scheduled = true;
            continue;
        }
        for (size_t r = g.r0; r < g.r1; ++r) {
            const long long roff = (long long)(runs[r].b0 - blk0) * BS, rn = (long long)(runs[r].b1 - runs[r].b0) * BS;
            const unsigned t = runs[r].tab;
            int rc = eq_launch_table(e, &e.sched_coeffs[(size_t)t * e.nb * 5], &e.sched_en[(size_t)t * e.nb], nullptr, e.chains, e.d_state,
                                     in + roff, out + roff, ss, cs, rn, st, nullptr, single ? ev_start : nullptr,
                                     single ? ev_stop : nullptr);
            if (rc) return rc;
        }
    }
    if (!single && ev_stop) HIP_TRY(hipEventRecord(ev_stop, st));
    return OHS_OK;
}

// ---- a row of table indices per stream (ohs_batch_process_scheduled_streams) -------------------------------------------------
bool eq_schedule_streams_scan(const EqState &e, BatchSchedule &sc)
{
    const size_t S = sc.tab_stride ? e.chains / 2 : 1;
    sc.seg_bits.assign(sc.n_segs, 0);
    sc.seg_max_on.assign(sc.n_segs, 0);
    for (size_t s = 0; s < S; ++s) {
        const unsigned *row = sc.tab + s * sc.tab_stride;
        unsigned prev = 0;
        for (size_t k = 0; k < sc.n_segs; ++k) {
            const unsigned t = row[k];
            if (t >= e.sched_n) return false;
            const unsigned char on = e.sched_on[t];
            unsigned char bits = (on == 0 || on > 12) ? BatchSchedule::kSegNoRing : 0;
            if (k > 0 && prev != t) {
                bits |= BatchSchedule::kSegIdxChange;
                if (e.sched_class[prev] != e.sched_class[t]) bits |= BatchSchedule::kSegFlagsChange;
            }
            prev = t;
            sc.seg_bits[k] |= bits;
            sc.seg_max_on[k] = std::max(sc.seg_max_on[k], on);
        }
    }
    return true;
}

// Blocks [blk0, blk0 + n_blocks) of a per-stream scheduled call.  The frames are cut where ANY stream's enabled flags change (the
// lanes' roles change: state travels through the state slots).  A piece in which every table met has 1 .. 12 enabled bands and for
// whose frames launch_eq_pass would take the wave ring is ONE launch of k_eq_ring_sched_streams: every wave follows its stream's
// row.  Every other piece is cut further where any stream's INDEX changes, and each of those spans is one launch sequence for all
// streams under their own tables -- the per-stream form of eq_launch, its tables gathered on the device from the schedule tables
// (launch_eq_gather_tables; the exact-specials / conveyor forms: one sequence per stream, as there).  The number of launches
// does not grow with the number of streams.
int eq_launch_scheduled_streams(EqState &e, const BatchSchedule &sc, size_t blk0, size_t n_blocks, const float *in, float *out,
                                long long ss, long long cs, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop)
{
    const size_t S = e.chains / 2, blk1 = blk0 + n_blocks;
    const size_t seg_first = blk0 / sc.seg_blocks, seg_last = (blk1 - 1) / sc.seg_blocks;
    auto seg_begin = [&](size_t k) { return std::max(blk0, k * sc.seg_blocks); };
    const auto [xcd_lo, xcd_n] = eq_xcds(e);
    // pieces [k0, k1] of segments without a change of flags
    struct Piece { size_t k0, k1; bool no_ring, idx_change; };
    std::vector<Piece> pieces;
    for (size_t k = seg_first; k <= seg_last; ++k) {
        const unsigned char bits = sc.seg_bits[k];
        if (k == seg_first || (bits & BatchSchedule::kSegFlagsChange)) pieces.push_back({k, k, false, false});
        else if (bits & BatchSchedule::kSegIdxChange) pieces.back().idx_change = true;
        pieces.back().k1 = k;
        if (bits & BatchSchedule::kSegNoRing) pieces.back().no_ring = true;
    }
    auto piece_takes_kernel = [&](const Piece &p) {
        const long long n = (long long)((p.k1 == seg_last ? blk1 : (p.k1 + 1) * sc.seg_blocks) - seg_begin(p.k0)) * BS;
        return !p.no_ring && eq_sched_kernel_serves(e, sc, ss, cs, n, 1);   // (1 .. 12 bands per stream: asked with one)
    };
    // the events ride in the dispatch when the chunk is exactly one launch of the scheduled kernel; else around
    const bool single = pieces.size() == 1 && piece_takes_kernel(pieces[0]);
    if (!single && ev_start) HIP_TRY(hipEventRecord(ev_start, st));
    for (const Piece &p : pieces) {
        const size_t pb0 = seg_begin(p.k0), pb1 = p.k1 == seg_last ? blk1 : (p.k1 + 1) * sc.seg_blocks;
        if (piece_takes_kernel(p)) {
            const long long off = (long long)(pb0 - blk0) * BS, n = (long long)(pb1 - pb0) * BS;
            EqRingSched sch;
            sch.lane_tabs = e.d_sched_lanes; sch.seg_tab = sc.d_tab; sch.n_segs = (int)sc.n_segs;
            sch.seg_len = (int)(sc.seg_blocks * BS);
            sch.seg0 = (int)p.k0; sch.off0 = (int)((pb0 - p.k0 * sc.seg_blocks) * BS);
            hipError_t err = launch_eq_ring_sched_streams(in + off, out + off, ss, cs, n, (int)e.chains, e.d_sched_stabs, e.d_state, sch,
                                                          (long long)sc.tab_stride, st, e.fp_mode, xcd_lo, xcd_n,
                                                          single ? ev_start : nullptr, single ? ev_stop : nullptr);
            if (err != hipSuccess) return fail(OHS_ERR_HIP, std::string("eq launch (per-stream schedule): ") + hipGetErrorString(err));
            e.last_form = OHS_EQ_FORM_WAVE_RING;
            e.last_scheduled = p.idx_change;
            continue;
        }
        // spans [j0, j1] of segments without a change of any stream's index
        for (size_t j0 = p.k0; j0 <= p.k1;) {
            size_t j1 = j0;
            const unsigned char mx = sc.seg_max_on[j0];        // (no index changes inside the span: every segment's is this)
            while (j1 + 1 <= p.k1 && !(sc.seg_bits[j1 + 1] & BatchSchedule::kSegIdxChange)) ++j1;
            const size_t sb0 = seg_begin(j0), sb1 = j1 == seg_last ? blk1 : (j1 + 1) * sc.seg_blocks;
            const long long off = (long long)(sb0 - blk0) * BS, n = (long long)(sb1 - sb0) * BS;
            const float *sin = in + off;
            float *sout = out + off;
            if (mx == 0) {      // identity for every stream
                int rc = eq_copy_through(sin, sout, ss, cs, n, e.chains, st);
                if (rc) return rc;
            } else if (eq_ring_forms_serve(e, ss, cs, n)) {
                const size_t passes = ((size_t)mx + 11) / 12;
                hipError_t err = launch_eq_gather_tables(e.d_sched_gather, e.d_sched_stabs, sc.d_tab + j0, (long long)sc.tab_stride, (int)S,
                                                         (int)e.sched_n, (int)passes, st);
                if (err != hipSuccess) return fail(OHS_ERR_HIP, std::string("eq schedule tables (gather): ") + hipGetErrorString(err));
                for (size_t pk = 0; pk < passes; ++pk) {
                    err = launch_eq_ring_streams(pk ? sout : sin, sout, ss, cs, n, (int)e.chains, e.d_sched_gather + pk * S, e.d_state, st,
                                                 e.fp_mode, xcd_lo, xcd_n, nullptr, nullptr, &e.last_form);
                    e.last_scheduled = false;
                    if (err != hipSuccess) return fail(OHS_ERR_HIP, std::string("eq launch (per-stream schedule, span): ") + hipGetErrorString(err));
                }
            } else {
                for (size_t s = 0; s < S; ++s) {
                    const unsigned t = sc.tab[s * sc.tab_stride + j0];
                    int rc = eq_launch_stream(e, s, &e.sched_coeffs[(size_t)t * e.nb * 5], &e.sched_en[(size_t)t * e.nb], sin, sout, ss, cs,
                                              n, st, nullptr);
                    if (rc) return rc;
                }
            }
            j0 = j1 + 1;
        }
    }
    if (!single && ev_stop) HIP_TRY(hipEventRecord(ev_stop, st));
    return OHS_OK;
}

}  // namespace ohs_api

extern "C" {

// ---- eq --------------------------------------------------------------------------------
int ohs_biquad_coeffs(int filter_type, float fs, float fc, float q, float gain_db, float out[5])
{
    if (!out) return fail(OHS_ERR_INVALID_ARG, "out is NULL");
    return rbj(filter_type, fs, fc, q, gain_db, out);
}

int ohs_eq_create(int device, size_t num_bands, float fs, ohs_eq **out)
{
    if (!out) return fail(OHS_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    DeviceCtx *ctx = nullptr;
    int rc = get_ctx(device, &ctx);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    ohs_eq *q = new (std::nothrow) ohs_eq();
    if (!q) return fail(OHS_ERR_ALLOC, "out of host memory");
    q->device = device; q->ctx = ctx; q->fs = fs;
    if (hipStreamCreateWithFlags(&q->st, hipStreamNonBlocking) != hipSuccess) {
        delete q;
        return fail(OHS_ERR_HIP, "hipStreamCreate failed");
    }
    rc = eq_init(q->eq, num_bands, 2, fs, q->st);
    if (rc == OHS_OK && hipStreamSynchronize(q->st) != hipSuccess) rc = fail(OHS_ERR_HIP, "sync failed");
    if (rc) { ohs_eq_destroy(q); return rc; }
    *out = q;
    return OHS_OK;
}

void ohs_eq_destroy(ohs_eq *q)
{
    if (!q) return;
    hipSetDevice(q->device);
    DeviceWideSection dws;
    if (q->st) hipStreamSynchronize(q->st);
    eq_free(q->eq);
    if (q->d_buf) hipFree(q->d_buf);
    if (q->h_pin) hipHostFree(q->h_pin);
    if (q->d_pinbuf) hipFree(q->d_pinbuf);
    if (q->h_done) hipHostFree(q->h_done);
    if (q->d_counter) hipFree(q->d_counter);
    if (q->st) hipStreamDestroy(q->st);
    delete q;
}

int ohs_eq_update_band(ohs_eq *q, size_t band, float fs, int filter_type, float fc, float qv,
                       float gain_db, int enabled)
{
    if (!q) return fail(OHS_ERR_INVALID_ARG, "eq is NULL");
    if (band >= q->eq.nb) return OHS_OK;    // parametric_eq.rs:145 silently ignored
    float c[5];
    int rc = rbj(filter_type, fs, fc, qv, gain_db, c);
    if (rc) return rc;
    std::memcpy(&q->eq.coeffs[5 * band], c, sizeof(c));
    q->eq.en[band] = enabled != 0;
    return OHS_OK;
}

int ohs_eq_set_band_coeffs(ohs_eq *q, size_t band, const float coeffs[5], int enabled)
{
    if (!q || !coeffs) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    if (band >= q->eq.nb) return OHS_OK;
    std::memcpy(&q->eq.coeffs[5 * band], coeffs, 5 * sizeof(float));
    q->eq.en[band] = enabled != 0;
    return OHS_OK;
}

int ohs_eq_get_band_coeffs(const ohs_eq *q, size_t band, float coeffs[5], int *enabled)
{
    if (!q || !coeffs || band >= q->eq.nb) return fail(OHS_ERR_INVALID_ARG, "bad argument");
    std::memcpy(coeffs, &q->eq.coeffs[5 * band], 5 * sizeof(float));
    if (enabled) *enabled = q->eq.en[band];
    return OHS_OK;
}

int ohs_eq_process_block(ohs_eq *q, float *left, float *right, size_t n)
{
    if (!q) return fail(OHS_ERR_INVALID_ARG, "eq is NULL");
    if (n == 0) return OHS_OK;
    if (!left || !right) return fail(OHS_ERR_INVALID_ARG, "NULL audio pointer");
    HIP_TRY(hipSetDevice(q->device));
    if (n <= 8192) {
        // real-time sized call: copy kernels move the block between pinned, mapped host memory and the
        // device, the EQ runs on device memory -- three launches and one synchronisation, no copy engine.
        // (The EQ kernel does not touch host memory itself: its prefetch runs one 128-sample group = 1.5 us
        // ahead, less than a PCIe read, and its 64-byte stores are a poor fit for the bus.)
        // 1024 frames: 47 us per call (was 260 us with four hipMemcpyAsync of pageable memory).
        if (n > q->pin_cap) {
            DeviceWideSection dws;
            size_t ncap = q->pin_cap ? q->pin_cap : 2048;
            while (ncap < n) ncap *= 2;
            if (q->h_pin) hipHostFree(q->h_pin);
            if (q->d_pinbuf) hipFree(q->d_pinbuf);
            q->h_pin = q->dm_pin = q->d_pinbuf = nullptr; q->pin_cap = 0;
            HIP_TRY(hipHostMalloc((void **)&q->h_pin, 2 * ncap * sizeof(float), hipHostMallocMapped));
            HIP_TRY(hipHostGetDevicePointer((void **)&q->dm_pin, q->h_pin, 0));
            HIP_TRY(hipMalloc(&q->d_pinbuf, 2 * ncap * sizeof(float)));
            q->pin_cap = ncap;
        }
        std::memcpy(q->h_pin, left, n * sizeof(float));
        std::memcpy(q->h_pin + q->pin_cap, right, n * sizeof(float));
        bool any = false;
        for (size_t i = 0; i < q->eq.nb; ++i) any = any || q->eq.en[i];
        if (!any) return OHS_OK;                        // every band disabled: identity
        HIP_TRY(launch_scale_copy(q->dm_pin, q->d_pinbuf, (long long)(q->pin_cap + n), 1.0f, q->st));
        int rc = eq_launch(q->eq, q->d_pinbuf, q->d_pinbuf, 0, (long long)q->pin_cap, (long long)n, q->st);
        if (rc) return rc;
        if (!q->h_done) {
            HIP_TRY(hipHostMalloc((void **)&q->h_done, 64, hipHostMallocMapped));
            HIP_TRY(hipHostGetDevicePointer((void **)&q->dm_done, q->h_done, 0));
            *q->h_done = 0;
            HIP_TRY(hipMalloc((void **)&q->d_counter, sizeof(unsigned)));
            HIP_TRY(hipMemsetAsync(q->d_counter, 0, sizeof(unsigned), q->st));
        }
        const unsigned seq = ++q->call_seq;
        HIP_TRY(launch_scale_copy_done(q->d_pinbuf, q->dm_pin, (long long)(q->pin_cap + n), 1.0f, q->d_counter, q->dm_done, seq, q->st));
        {   // the copy-out kernel's completion word; the stream is the fallback and the error path
            const auto t0 = std::chrono::steady_clock::now();
            unsigned spins = 0;
            while (__atomic_load_n(q->h_done, __ATOMIC_ACQUIRE) != seq) {
                if ((++spins & 255u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5)) {
                    HIP_TRY(hipStreamSynchronize(q->st));
                    break;
                }
            }
        }
        std::memcpy(left, q->h_pin, n * sizeof(float));
        std::memcpy(right, q->h_pin + q->pin_cap, n * sizeof(float));
        return OHS_OK;
    }
    if (n > q->buf_cap) {
        DeviceWideSection dws;
        size_t ncap = q->buf_cap ? q->buf_cap : 4 * BS;
        while (ncap < n) ncap *= 2;
        if (q->d_buf) hipFree(q->d_buf);
        q->d_buf = nullptr; q->buf_cap = 0;
        HIP_TRY(hipMalloc(&q->d_buf, 2 * ncap * sizeof(float)));
        q->buf_cap = ncap;
    }
    HIP_TRY(hipMemcpyAsync(q->d_buf, left, n * sizeof(float), hipMemcpyHostToDevice, q->st));
    HIP_TRY(hipMemcpyAsync(q->d_buf + q->buf_cap, right, n * sizeof(float), hipMemcpyHostToDevice, q->st));
    int rc = eq_launch(q->eq, q->d_buf, q->d_buf, 0, (long long)q->buf_cap, (long long)n, q->st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(left, q->d_buf, n * sizeof(float), hipMemcpyDeviceToHost, q->st));
    HIP_TRY(hipMemcpyAsync(right, q->d_buf + q->buf_cap, n * sizeof(float), hipMemcpyDeviceToHost, q->st));
    HIP_TRY(hipStreamSynchronize(q->st));
    return OHS_OK;
}

#ifdef OHS_EXPERIMENTS
// experiments build only (not declared in include/ohs_hip.h): the same cascade, same state, OUT OF PLACE on the device -- n
// samples per channel of any length from one allocation to another, which the public entry points reach only in whole blocks
// of 512 (the batch).  The output allocation starts from sentinel bits: a sample that no store reached shows.
int ohs_debug_eq_process_block_out_of_place(ohs_eq *q, const float *left, const float *right, float *out_left, float *out_right, size_t n)
{
    if (!q || !left || !right || !out_left || !out_right || n == 0) return fail(OHS_ERR_INVALID_ARG, "bad argument");
    HIP_TRY(hipSetDevice(q->device));
    float *d_in = nullptr, *d_out = nullptr;
    HIP_TRY(hipMalloc(&d_in, 2 * n * sizeof(float)));
    hipError_t e = hipMalloc(&d_out, 2 * n * sizeof(float));
    int rc = OHS_OK;
    if (e == hipSuccess) e = hipMemcpyAsync(d_in, left, n * sizeof(float), hipMemcpyHostToDevice, q->st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_in + n, right, n * sizeof(float), hipMemcpyHostToDevice, q->st);
    if (e == hipSuccess) e = hipMemsetAsync(d_out, 0xA5, 2 * n * sizeof(float), q->st);
    if (e == hipSuccess) rc = eq_launch(q->eq, d_in, d_out, 0, (long long)n, (long long)n, q->st);
    if (e == hipSuccess && rc == OHS_OK) e = hipMemcpyAsync(out_left, d_out, n * sizeof(float), hipMemcpyDeviceToHost, q->st);
    if (e == hipSuccess && rc == OHS_OK) e = hipMemcpyAsync(out_right, d_out + n, n * sizeof(float), hipMemcpyDeviceToHost, q->st);
    const hipError_t es = hipStreamSynchronize(q->st);
    if (e == hipSuccess) e = es;
    if (d_out) hipFree(d_out);
    hipFree(d_in);
    if (rc) return rc;
    if (e != hipSuccess) return fail(OHS_ERR_HIP, hipGetErrorString(e));
    return OHS_OK;
}
#endif

int ohs_eq_set_flush_denormals(ohs_eq *q, int mode)
{
    if (!q) return fail(OHS_ERR_INVALID_ARG, "eq is NULL");
    if (mode < 0 || mode > 2) return fail(OHS_ERR_INVALID_ARG, "mode must be 0 (IEEE), 1 (FTZ) or 2 (FTZ | DAZ)");
    q->eq.fp_mode = mode;
    return OHS_OK;
}

int ohs_eq_set_exact_specials(ohs_eq *q, int enable)
{
    if (!q) return fail(OHS_ERR_INVALID_ARG, "eq is NULL");
    q->eq.exact_specials = enable != 0;
    return OHS_OK;
}

int ohs_eq_reset(ohs_eq *q)
{
    if (!q) return fail(OHS_ERR_INVALID_ARG, "eq is NULL");
    HIP_TRY(hipSetDevice(q->device));
    int rc = eq_reset(q->eq, q->st);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(q->st));
    return OHS_OK;
}

int ohs_eq_frequency_response(const ohs_eq *q, float fs, const float *freqs, size_t n, float *out)
{
    if (!q || (n && (!freqs || !out))) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    if (n == 0) return OHS_OK;
    HIP_TRY(hipSetDevice(q->device));
    const size_t nb = q->eq.nb;
    float *d = nullptr;
    const size_t words = nb * 5 + nb + 2 * n + 8;
    HIP_TRY(hipMalloc(&d, words * sizeof(float)));
    float *d_c = d, *d_f = d + nb * 5 + nb + 4, *d_o = d_f + n;
    int *d_en = (int *)(d + nb * 5);
    hipError_t e = hipSuccess;
    if (nb) {
        e = hipMemcpyAsync(d_c, q->eq.coeffs.data(), nb * 5 * sizeof(float), hipMemcpyHostToDevice, q->st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_en, q->eq.en.data(), nb * sizeof(int), hipMemcpyHostToDevice, q->st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(d_f, freqs, n * sizeof(float), hipMemcpyHostToDevice, q->st);
    if (e == hipSuccess) e = launch_eq_freq_response(d_c, d_en, (int)nb, fs, d_f, (int)n, d_o, q->st);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_o, n * sizeof(float), hipMemcpyDeviceToHost, q->st);
    if (e == hipSuccess) e = hipStreamSynchronize(q->st);
    { DeviceWideSection dws; hipFree(d); }
    if (e != hipSuccess) return fail(OHS_ERR_HIP, hipGetErrorString(e));
    return OHS_OK;
}

// ---- BiquadFilter as a type of its own (parametric_eq.rs:46-123) -------------------------------
int ohs_biquad_create(int device, float initial_sample_rate, ohs_biquad **out)
{
    if (!out) return fail(OHS_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    DeviceCtx *ctx = nullptr;
    int rc = get_ctx(device, &ctx);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    ohs_biquad *f = new (std::nothrow) ohs_biquad();
    if (!f) return fail(OHS_ERR_ALLOC, "out of host memory");
    f->device = device; f->ctx = ctx;
    if (hipStreamCreateWithFlags(&f->st, hipStreamNonBlocking) != hipSuccess) {
        delete f;
        return fail(OHS_ERR_HIP, "hipStreamCreate failed");
    }
    rc = eq_init(f->eq, 1, 1, initial_sample_rate, f->st);        // PeakingEQ 0 dB @ 20 Hz Q 0.707, disabled (:63-76)
    if (rc == OHS_OK && hipStreamSynchronize(f->st) != hipSuccess) rc = fail(OHS_ERR_HIP, "sync failed");
    if (rc) { ohs_biquad_destroy(f); return rc; }
    *out = f;
    return OHS_OK;
}

void ohs_biquad_destroy(ohs_biquad *f)
{
    if (!f) return;
    hipSetDevice(f->device);
    DeviceWideSection dws;
    if (f->st) hipStreamSynchronize(f->st);
    eq_free(f->eq);
    if (f->d_buf) hipFree(f->d_buf);
    if (f->st) hipStreamDestroy(f->st);
    delete f;
}

int ohs_biquad_clone(const ohs_biquad *src, ohs_biquad **out)       // impl Clone :52-60: coefficients, state, enabled
{
    if (!src || !out) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    ohs_biquad *f = nullptr;
    int rc = ohs_biquad_create(src->device, 48000.0f, &f);
    if (rc) return rc;
    f->eq.coeffs = src->eq.coeffs; f->eq.en = src->eq.en;
    f->eq.exact_specials = src->eq.exact_specials; f->eq.fp_mode = src->eq.fp_mode;
    hipStreamSynchronize(src->st);
    if (hipMemcpyAsync(f->eq.d_state, src->eq.d_state, (size_t)kEqStateSlots * 2 * sizeof(float), hipMemcpyDeviceToDevice,
                       f->st) != hipSuccess || hipStreamSynchronize(f->st) != hipSuccess) {
        ohs_biquad_destroy(f);
        return fail(OHS_ERR_HIP, "state copy failed");
    }
    *out = f;
    return OHS_OK;
}

int ohs_biquad_reset_state(ohs_biquad *f)
{
    if (!f) return fail(OHS_ERR_INVALID_ARG, "filter is NULL");
    HIP_TRY(hipSetDevice(f->device));
    int rc = eq_reset(f->eq, f->st);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(f->st));
    return OHS_OK;
}

int ohs_biquad_set_enabled(ohs_biquad *f, int enabled)
{
    if (!f) return fail(OHS_ERR_INVALID_ARG, "filter is NULL");
    f->eq.en[0] = enabled != 0;
    return OHS_OK;
}

int ohs_biquad_update_coeffs(ohs_biquad *f, int filter_type, float sample_rate, float center_freq, float q, float gain_db)
{
    if (!f) return fail(OHS_ERR_INVALID_ARG, "filter is NULL");
    float c[5];
    int rc = rbj(filter_type, sample_rate, center_freq, q, gain_db, c);
    if (rc) return rc;
    std::memcpy(&f->eq.coeffs[0], c, sizeof(c));        // the state is kept (update_coefficients, :112)
    return OHS_OK;
}

int ohs_biquad_set_coeffs(ohs_biquad *f, const float coeffs[5])
{
    if (!f || !coeffs) return fail(OHS_ERR_INVALID_ARG, "NULL argument");
    std::memcpy(&f->eq.coeffs[0], coeffs, 5 * sizeof(float));
    return OHS_OK;
}

int ohs_biquad_process(ohs_biquad *f, float *samples, size_t n)
{
    if (!f) return fail(OHS_ERR_INVALID_ARG, "filter is NULL");
    if (n == 0) return OHS_OK;
    if (!samples) return fail(OHS_ERR_INVALID_ARG, "samples is NULL");
    if (!f->eq.en[0]) return OHS_OK;                    // disabled: the input sample, bit for bit (:118-120)
    HIP_TRY(hipSetDevice(f->device));
    if (n > f->cap) {
        DeviceWideSection dws;
        size_t ncap = f->cap ? f->cap : 4 * BS;
        while (ncap < n) ncap *= 2;
        if (f->d_buf) hipFree(f->d_buf);
        f->d_buf = nullptr; f->cap = 0;
        HIP_TRY(hipMalloc(&f->d_buf, ncap * sizeof(float)));
        f->cap = ncap;
    }
    HIP_TRY(hipMemcpyAsync(f->d_buf, samples, n * sizeof(float), hipMemcpyHostToDevice, f->st));
    int rc = eq_launch(f->eq, f->d_buf, f->d_buf, 0, 0, (long long)n, f->st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(samples, f->d_buf, n * sizeof(float), hipMemcpyDeviceToHost, f->st));
    HIP_TRY(hipStreamSynchronize(f->st));
    return OHS_OK;
}

}  // extern "C"
