// api_conv.hip -- the convolution state of a handle (ConvState: one stream for ohs_engine, S streams for ohs_batch):
// set_ir (convolution.rs:111-139), the ring of input spectra, and conv_launch.  conv_launch serves a call in three steps:
// conv_choose_plan picks the kernel family (the whole rule: it reads the state and tuning() only), one runner per family
// reserves and launches (conv_run_p1, conv_run_os, conv_lb_launch, conv_xb_launch, conv_run_tp, conv_run_sequential), and
// one epilogue advances what every family shares (block counters, last plan, per-family counts, pending tails).
#include "api_internal.h"

using namespace ohs;
using namespace ohs_api;

namespace ohs_api {

// one convolution call: S streams of two channels, n_blocks * 512 frames (strides in floats)
struct ConvCall {
    const float *in; long long in_ss, in_cs;
    float *out; long long out_ss, out_cs;
    int n_blocks; float gain;
    // a gain per segment instead (ConvGains; device memory): frames of block t leave with tab[(off + t) / seg]
    // (gain_stream: stream s reads its row at gain_tab + s * gain_stream; 0 = one row for all)
    const float *gain_tab = nullptr; int gain_seg = 1, gain_off = 0, gain_stream = 0;
    const ConvIrs *irs = nullptr;       // a set of responses per segment and stream (k_conv_p1_irs)
};

// right before the handle is deleted: the buffers only
void conv_free(ConvState &c)
{
    DeviceWideSection dws;      // (frees below: no resident kernel may be in their way)
    for (float2 *h : c.d_H) if (h) hipFree(h);
    for (void *d : std::initializer_list<void *>{c.d_hist, c.d_pre, c.d_tails, c.d_tails_alt, c.d_cd, c.d_chunk_tails, c.d_cdm, c.d_W,
                                                 c.d_W1, c.d_merged, c.d_merged_alt, c.d_last_in, c.d_irt, c.d_cd_os, c.d_irl,
                                                 c.d_xhist, c.d_xhist_alt, c.d_lb_ring, c.d_lb_cd, c.d_lb_ab, c.d_lb_cd_alt,
                                                 c.d_xb_cd, c.d_xb_ab, c.d_ptail, c.d_ptail_alt, c.d_irs_cd, c.d_irs_H, c.d_irs_t,
                                                 c.d_lay_cd, c.d_lay_ov, c.d_lay_ov_alt, c.d_lays_cd, c.d_obj_ah})
        if (d) hipFree(d);
}

int conv_init(ConvState &c, size_t S, hipStream_t st)
{
    c.S = S;
    for (int p = 0; p < 4; ++p) {
        // default path: one all-zero partition (convolution.rs:46-63); FFT(0) == 0
        HIP_TRY(hipMalloc(&c.d_H[p], NF * sizeof(float2)));
        HIP_TRY(hipMemsetAsync(c.d_H[p], 0, NF * sizeof(float2), st));
        c.P[p] = 1;
        c.since[p] = 0;
    }
    c.cap = 1;
    c.cnt = 0;
    HIP_TRY(hipMalloc(&c.d_hist, S * (size_t)c.cap * NF * sizeof(float2)));
    HIP_TRY(hipMemsetAsync(c.d_hist, 0, S * (size_t)c.cap * NF * sizeof(float2), st));
    HIP_TRY(hipMalloc(&c.d_tails, S * 2 * 8 * 64 * sizeof(float2)));
    HIP_TRY(hipMemsetAsync(c.d_tails, 0, S * 2 * 8 * 64 * sizeof(float2), st));
    HIP_TRY(hipMalloc(&c.d_tails_alt, S * 2 * 8 * 64 * sizeof(float2)));
    HIP_TRY(hipMalloc(&c.d_cd, 2 * NF * sizeof(float2)));
    c.cd_valid = false;
    return OHS_OK;
}

// Batch objects let the P = 1 fast path leave its state behind lazily: a k_conv_p1 launch then ends with the merged
// overlap of its last block and a copy of that block's input instead of a k_conv_p1_state launch (9 us + a launch gap
// per call, hidden nowhere when the convolution runs alone); the next fast launch starts from the merged overlap -- which
// also makes a call boundary invisible in the output bits.  (Tuning::p1_lazy_state = 0: the per-path state after every launch.)
int conv_enable_lazy_state(ConvState &c)
{
    if (!tuning().p1_lazy_state) return OHS_OK;
    HIP_TRY(hipMalloc(&c.d_merged, c.S * 8 * 64 * sizeof(float2)));
    HIP_TRY(hipMalloc(&c.d_merged_alt, c.S * 8 * 64 * sizeof(float2)));
    HIP_TRY(hipMalloc(&c.d_last_in, c.S * 2 * BS * sizeof(float)));
    HIP_TRY(hipMalloc(&c.d_irt, 4 * BS * sizeof(float)));
    HIP_TRY(hipMemset(c.d_irt, 0, 4 * BS * sizeof(float)));        // (default paths: one all-zero partition)
    HIP_TRY(hipMalloc(&c.d_cd_os, 2 * NF * sizeof(float4)));
    c.cd_os_valid = false;
    c.lazy_ok = true;
    c.tails_lazy = false;
    return OHS_OK;
}

// the per-path overlaps (d_tails) from the lazy state: whoever reads or edits d_tails calls this first -- a per-path
// set_ir (with the OLD spectra still in place: the overlaps belong to them), the general and the long-IR kernels
// The block-2048 plan leaves no spectra and no overlaps behind: its state is the streams' last input frames (d_xhist).  The
// block-512 state -- the ring's last Pmax spectra and the four per-path overlaps behind the last block -- is what the
// reference's engine would hold after those frames (convolution.rs:258,279-284): replay the last R = min(Pmax, cnt) blocks
// through the sequential kernel from zero overlaps, nothing stored (block t - i of the replay is visible to path p under
// the same `since` rule as ever; what lies further back than R blocks cannot reach the last block's overlap).
static int conv_materialise_from_xhist(ConvState &c, DeviceCtx *ctx, hipStream_t st)
{
    if (!c.lb_lazy) return OHS_OK;
    const long long R = std::min<long long>(std::min<long long>(conv_max_p(c), (long long)c.cnt), c.xh_len / BS);
    if (R > 0) {
        int rc = conv_grow_ring(c, (int)R, st);
        if (rc) return rc;
        {   // the ring of input frames in time order
            hipError_t e = launch_conv_lb_xhist_linearise(c.d_xhist, c.d_xhist_alt, c.xh_len, c.xh_head, (int)c.S, st);
            if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("input history: ") + hipGetErrorString(e));
        }
        ConvGeneralArgs a;
        a.in = c.d_xhist_alt + (c.xh_len - R * BS); a.out = c.d_xhist_alt;     // (nothing is stored: skip_store = R)
        a.in_stream_stride = 2 * c.xh_len; a.in_ch_stride = c.xh_len;
        a.out_stream_stride = 2 * c.xh_len; a.out_ch_stride = c.xh_len;
        a.n_blocks = (int)R;
        for (int p = 0; p < 4; ++p) { a.H[p] = c.d_H[p]; a.P[p] = c.P[p]; a.since[p] = c.since[p] - R; }
        a.hist = c.d_hist; a.cap = c.cap; a.cnt = c.cnt - (unsigned long long)R;
        a.tails = c.d_tails; a.tails_out = c.d_tails;
        a.skip_store = (int)R; a.zero_tails_in = 1;
        a.tw = ctx->d_tw; a.gain = 1.0f; a.fp_mode = c.fp_mode;
        hipError_t e = launch_conv_general(a, (int)c.S, st);
        if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("state replay launch: ") + hipGetErrorString(e));
    } else {
        HIP_TRY(hipMemsetAsync(c.d_tails, 0, c.S * 2 * 8 * 64 * sizeof(float2), st));
    }
    c.lb_lazy = false;
    return OHS_OK;
}

int conv_materialise_state(ConvState &c, DeviceCtx *ctx, hipStream_t st)
{
    if (c.lb_lazy || c.tails_lazy) c.pre_cnt = ~0ull;       // (the ring is about to be rewritten)
    if (c.lb_lazy) {
        const int rc = conv_materialise_from_xhist(c, ctx, st);
        if (rc) return rc;
    }
    if (!c.tails_lazy) return OHS_OK;
    if (!c.tails_both) {        // (else d_tails is current already)
        const int rc = conv_materialise_keep_lazy(c, ctx, st);
        if (rc) return rc;
    }
    c.tails_lazy = false; c.tails_both = false;
    return OHS_OK;
}

// arguments of the state kernels on the lazy state: block 0 of d_last_in -> d_tails
static void conv_state_args(const ConvState &c, const DeviceCtx *ctx, ConvP1Args &a)
{
    std::memset(&a, 0, sizeof(a));
    a.in = c.d_last_in; a.in_stream_stride = 2 * (long long)BS; a.in_ch_stride = (long long)BS;
    a.n_blocks = 1; a.n_streams = (int)c.S;
    for (int p = 0; p < 4; ++p) a.H[p] = c.d_H[p];
    a.tails_out = c.d_tails;
    a.tw = ctx->d_tw; a.fp_mode = c.fp_mode;
    a.xcd_lo = 0; a.xcd_n = 8;
}

int conv_materialise_keep_lazy(ConvState &c, DeviceCtx *ctx, hipStream_t st)
{
    if (!c.tails_lazy || c.tails_both) return OHS_OK;
    ConvP1Args a;
    conv_state_args(c, ctx, a);
    hipError_t e = launch_conv_p1_state(a, st);
    if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("conv_p1_state launch: ") + hipGetErrorString(e));
    c.tails_both = true;
    return OHS_OK;
}

// grow the spectrum ring so that cap >= need, keeping the most recent old_cap blocks
int conv_grow_ring(ConvState &c, int need, hipStream_t st)
{
    if (need <= c.cap) return OHS_OK;
    DeviceWideSection dws;      // (frees / device-wide waits below: no resident kernel may be in their way)
    c.pre_cnt = ~0ull;
    const int ncap = next_pow2(need);
    float2 *nh = nullptr;
    HIP_TRY(hipMalloc(&nh, c.S * (size_t)ncap * NF * sizeof(float2)));
    HIP_TRY(hipMemsetAsync(nh, 0, c.S * (size_t)ncap * NF * sizeof(float2), st));
    for (int i = 0; i < c.cap; ++i) {
        if (c.cnt < (unsigned long long)(i + 1)) break;
        const unsigned long long u = c.cnt - 1 - (unsigned long long)i;
        const size_t so = (size_t)(u & (unsigned long long)(c.cap - 1));
        const size_t sn = (size_t)(u & (unsigned long long)(ncap - 1));
        // one strided copy over all streams
        HIP_TRY(hipMemcpy2DAsync(nh + sn * NF, (size_t)ncap * NF * sizeof(float2),
                                 c.d_hist + so * NF, (size_t)c.cap * NF * sizeof(float2),
                                 NF * sizeof(float2), c.S, hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    hipFree(c.d_hist);
    c.d_hist = nh;
    c.cap = ncap;
    return OHS_OK;
}

// a buffer whose contents may go, reallocated to `bytes`: the stream drained, the old buffer freed, the new one allocated
// (null if that fails).  The caller records the new capacity on success only: a failed reserve leaves capacity 0, and the
// next call tries again.
template <class T> static int conv_realloc(T *&d, size_t bytes, hipStream_t st)
{
    DeviceWideSection dws;      // (frees / device-wide waits below: no resident kernel may be in their way)
    HIP_TRY(hipStreamSynchronize(st));
    if (d) hipFree(d);
    d = nullptr;
    HIP_TRY(hipMalloc(&d, bytes));
    return OHS_OK;
}

// ---- block-2048 plan: the host side of its state (api_internal.h: ConvState) -----------------------------------------
static long long lb_p2pad_for(int Pmax) { return ((((long long)Pmax + 3) / 4) + 3) / 4 * 4; }    // 2048-tap partitions, multiple of 4

// the time-domain copies of the four responses (batch objects): [4][irl_len], zero-padded, grown as needed
static int conv_lb_irl_reserve(ConvState &c, long long need, hipStream_t st)
{
    if (need <= c.irl_len) return OHS_OK;
    DeviceWideSection dws;
    float *n = nullptr;
    HIP_TRY(hipMalloc(&n, 4 * (size_t)need * sizeof(float)));
    hipError_t e = hipMemsetAsync(n, 0, 4 * (size_t)need * sizeof(float), st);
    if (e == hipSuccess && c.d_irl)
        e = hipMemcpy2DAsync(n, (size_t)need * sizeof(float), c.d_irl, (size_t)c.irl_len * sizeof(float),
                             (size_t)c.irl_len * sizeof(float), 4, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { hipFree(n); return fail(OHS_ERR_HIP, std::string("impulse response copy: ") + hipGetErrorString(e)); }
    if (c.d_irl) hipFree(c.d_irl);
    c.d_irl = n; c.irl_len = need;
    c.lb_cd_valid = false; c.lb_tables_gen++;
    return OHS_OK;
}

int conv_lb_store_ir(ConvState &c, int path, const float *d_src, const float *h_src, size_t len, int P, hipStream_t st)
{
    {
        const int rcr = conv_lb_irl_reserve(c, lb_p2pad_for(P) * kLbBlock, st);
        if (rcr) return rcr;
    }
    if (!c.d_irl) return OHS_OK;
    float *dst = c.d_irl + (size_t)path * c.irl_len;
    HIP_TRY(hipMemsetAsync(dst, 0, (size_t)c.irl_len * sizeof(float), st));
    if (len && d_src) HIP_TRY(hipMemcpyAsync(dst, d_src, len * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (len && h_src) HIP_TRY(hipMemcpyAsync(dst, h_src, len * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    c.lb_cd_valid = false; c.lb_tables_gen++;
    return OHS_OK;
}

// after a set_ir has updated P[] and since[]: the input history exists exactly while some response is long enough for the
// block-2048 plan (the one-partition fast path never pays for it); its length follows the longest response
int conv_lb_after_set_ir(ConvState &c, hipStream_t st)
{
    if (!c.lazy_ok) return OHS_OK;
    const int Pmax = conv_max_p(c);
    const long long want = Pmax >= lb_min_p() ? lb_p2pad_for(Pmax) * kLbBlock : 0;
    if (want != c.xh_len) {
        DeviceWideSection dws;
        HIP_TRY(hipStreamSynchronize(st));
        float *n = nullptr, *n2 = nullptr;
        if (want) {
            const size_t bytes = c.S * 2 * (size_t)want * sizeof(float);
            HIP_TRY(hipMalloc(&n, 2 * bytes));      // (a ring of twice the reach)
            if (hipMalloc(&n2, bytes) != hipSuccess) { hipFree(n); return fail(OHS_ERR_HIP, "hipMalloc(input history) failed"); }
            hipError_t e = hipMemsetAsync(n, 0, 2 * bytes, st);
            if (e == hipSuccess && c.d_xhist) {     // keep what is there: the newest frame ends at position `want` of the new ring
                const long long keep = std::min(want, c.xh_len);
                e = launch_conv_lb_xhist_linearise(c.d_xhist, c.d_xhist_alt, c.xh_len, c.xh_head, (int)c.S, st);
                if (e == hipSuccess)
                    e = hipMemcpy2DAsync(n + (want - keep), (size_t)(2 * want) * sizeof(float), c.d_xhist_alt + (c.xh_len - keep),
                                         (size_t)c.xh_len * sizeof(float), (size_t)keep * sizeof(float), c.S * 2,
                                         hipMemcpyDeviceToDevice, st);
            }
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) { hipFree(n); hipFree(n2); return fail(OHS_ERR_HIP, std::string("input history: ") + hipGetErrorString(e)); }
        }
        if (c.d_xhist) hipFree(c.d_xhist);
        if (c.d_xhist_alt) hipFree(c.d_xhist_alt);
        c.d_xhist = n; c.d_xhist_alt = n2;
        c.xh_valid = std::min(c.xh_valid, want);
        c.xh_len = want;
        c.xh_head = want;           // (the kept frames end at position `want`: the next frame goes there)
        c.lb_valid = 0;         // (the ring's depth follows the partition count)
        c.lb_cd_valid = false; c.lb_tables_gen++;
    }
    if (c.d_xhist && conv_since_zero(c)) {
        // every path has forgotten its past (convolution.rs:135-137): so has the input history, and zeros are what every path
        // may see of it
        HIP_TRY(hipMemsetAsync(c.d_xhist, 0, c.S * 2 * (size_t)(2 * c.xh_len) * sizeof(float), st));
        c.xh_valid = c.xh_len;
        c.xh_head = 0;
        c.lb_valid = 0;
    }
    return OHS_OK;
}

// ohs_batch_set_conv_plan(0) for long responses: the block-2048 plan for every call of an object whose longest response has
// lb_min_p() partitions or more.  Its windows sit on the stream's absolute grid, so a call of any length -- the plugin's
// 1024-frame block included -- continues the ring the previous call left (one or two windows to transform, no warm-up), and
// it beats the block-512 kernels at every call length measured (profiles/r05_short_calls_*.jsonl: 64 streams x 16 384 taps,
// 2-block calls 26 vs 35 us even WITH a warm-up per call; 256-block calls 0.138 vs 0.25 ms).
bool conv_plan_auto_is_lb(size_t S, long long n_blocks, int Pmax)
{
    (void)S; (void)n_blocks;
    return Pmax >= lb_min_p();
}

// segment length of a block-2048 launch sequence, in blocks of 2048 (the ring holds a segment's windows: 32 KiB each)
static long long lb_segment_blocks(size_t S)
{
    long long seg = (long long)tuning().lb_seg_windows / (long long)std::max<size_t>(S, 1);
    seg = std::max<long long>(8, std::min<long long>(seg, 256));
    return seg / kLbTile * kLbTile;
}

// tables of the block-2048 plan: the spectra of A = h_lsl + j h_lsr and B = h_rsl + j h_rsr per 2048-tap partition (the forward
// kernel in tables mode, two "streams" of P2pad windows; kept in d_lb_ab), then (C, D).  `a` receives the fields every launch
// of the plan shares.
static int conv_lb_prepare(ConvState &c, DeviceCtx *ctx, hipStream_t st, ConvLbArgs &a)
{
    const int P2pad = (int)(c.xh_len / kLbBlock);
    if (!c.d_lb_cd || c.lb_p2pad != P2pad) {
        c.lb_p2pad = 0; c.lb_cd_valid = false; c.lb_tables_gen++;
        int rc = conv_realloc(c.d_lb_cd, (size_t)P2pad * 2 * kLbBlock * sizeof(float4), st);
        if (rc == OHS_OK) rc = conv_realloc(c.d_lb_ab, (size_t)P2pad * 2 * kLbBlock * sizeof(float4), st);
        if (rc) return rc;
        c.lb_p2pad = P2pad;
    }
    std::memset(&a, 0, sizeof(a));
    a.tw = ctx->d_tw; a.tw4096 = ctx->d_tw4096; a.fp_mode = c.fp_mode; a.P2pad = P2pad;
    a.P2 = std::min(P2pad, (conv_max_p(c) + 3) / 4);        // (the real partitions of 2048 taps: the padding is never multiplied)
#ifdef OHS_EXPERIMENTS
    a.debug_skip = tuning().lb_skip;
#endif
    if (!c.lb_cd_valid) {
        if (c.irl_len < (long long)P2pad * kLbBlock) return fail(OHS_ERR_HIP, "block-2048 plan: impulse responses not stored");
        ConvLbArgs t = a;
        t.in = c.d_irl; t.in_stream_stride = 2 * c.irl_len; t.in_ch_stride = c.irl_len;
        t.out = nullptr; t.n_streams = 2; t.io_frame0 = 0; t.io_frames = c.irl_len;
        t.u0 = 0; t.n_fwd = P2pad; t.ring = c.d_lb_ab; t.ring_cap = P2pad; t.ring_base = 0; t.tables_mode = 1;
        t.fp_mode = 0;      // (tables are built in IEEE arithmetic, like k_ir_spectrum's)
        t.debug_skip = 0;
        hipError_t e = launch_conv_lb_forward(t, st);
        if (e == hipSuccess) e = launch_conv_lb_build_cd(c.d_lb_ab, P2pad, c.d_lb_cd, st);
        if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("block-2048 tables: ") + hipGetErrorString(e));
        c.lb_cd_valid = true;
    }
    return OHS_OK;
}

static int conv_lb_ring_reserve(ConvState &c, int cap_need, hipStream_t st)
{
    if (cap_need <= c.lb_ring_cap) return OHS_OK;
    c.lb_ring_cap = 0; c.lb_valid = 0;
    const int rc = conv_realloc(c.d_lb_ring, c.S * (size_t)cap_need * kLbBlock * sizeof(float4), st);
    if (rc) return rc;
    c.lb_ring_cap = cap_need;
    return OHS_OK;
}

// A per-path set_ir in mid-stream on an object that keeps the input history (convolution.rs:135-138: THAT path forgets its
// past, the others do not).  Instead of gating partitions per path in every kernel that follows, the reset is carried out
// as "every path forgets its past" plus what the frames in front of the reset still owe the output through each path --
// the tails: the input history followed by xh_len frames of silence through the plan's own two kernels, once with the
// L-speaker pair's tables alone (re = the lsl tail, im = the lsr tail) and once with the R-speaker pair's.  The reset path's
// row is dropped, rows still pending from an earlier reset are carried on, and conv_launch adds the rows to the output of
// the calls that follow, whatever plan serves them.  Returns taken = false when the history cannot vouch for every path's
// reach (then the block-512 kernels' per-path gates serve, as before).
static int conv_lb_tail_route(ConvState &c, DeviceCtx *ctx, int path, hipStream_t st, bool *taken)
{
    *taken = false;
    if (!c.lazy_ok || !c.d_xhist) return OHS_OK;
    if (conv_since_zero(c)) return OHS_OK;     // nothing processed since a full reset
    if (!conv_history_covers_paths(c)) return OHS_OK;
    ConvLbArgs a;
    int rc = conv_lb_prepare(c, ctx, st, a);
    if (rc) return rc;
    const int P2pad = a.P2pad;
    const long long Lt = c.xh_len;
    DeviceWideSection dws;
    if (c.lb_cd_alt_p2pad != P2pad) {
        c.lb_cd_alt_p2pad = 0;
        rc = conv_realloc(c.d_lb_cd_alt, (size_t)P2pad * 2 * kLbBlock * sizeof(float4), st);
        if (rc) return rc;
        c.lb_cd_alt_p2pad = P2pad;
    }
    if (c.pt_len != Lt) {       // (a response of another length since the last tails: rows of the old length are re-cut below)
        HIP_TRY(hipStreamSynchronize(st));
        float *n1 = nullptr, *n2 = nullptr;
        const size_t bytes = c.S * 4 * (size_t)Lt * sizeof(float);
        HIP_TRY(hipMalloc(&n1, bytes));
        if (hipMalloc(&n2, bytes) != hipSuccess) { hipFree(n1); return fail(OHS_ERR_HIP, "hipMalloc(pending tails) failed"); }
        hipError_t e = hipMemsetAsync(n1, 0, bytes, st);
        if (e == hipSuccess && c.pt_active && c.d_ptail) {
            // carry the rest of the pending rows over, from position 0 of the new buffer
            const long long rest = std::min(c.pt_len - c.pt_pos, Lt);
            if (rest > 0)
                e = hipMemcpy2DAsync(n1, (size_t)Lt * sizeof(float), c.d_ptail + c.pt_pos, (size_t)c.pt_len * sizeof(float),
                                     (size_t)rest * sizeof(float), c.S * 4, hipMemcpyDeviceToDevice, st);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { hipFree(n1); hipFree(n2); return fail(OHS_ERR_HIP, std::string("pending tails: ") + hipGetErrorString(e)); }
        if (c.d_ptail) hipFree(c.d_ptail);
        if (c.d_ptail_alt) hipFree(c.d_ptail_alt);
        c.d_ptail = n1; c.d_ptail_alt = n2; c.pt_len = Lt; c.pt_pos = 0;
    }
    rc = conv_lb_ring_reserve(c, 2 * P2pad - 1, st);
    if (rc) return rc;
    // windows -(P2pad - 1) .. P2pad - 1 of a segment that starts at the reset: the history, then silence (no buffer frames)
    a.n_streams = (int)c.S; a.gain = 1.0f;
    a.ring = c.d_lb_ring; a.ring_cap = c.lb_ring_cap; a.ring_base = 4ll * c.lb_ring_cap;
    a.in = c.d_xhist; a.io_frame0 = 0; a.io_frames = 0;         // (`in` is never read: no frame lies inside the buffer)
    a.xhist = c.d_xhist; a.xh_append = nullptr; a.xh_len = c.xh_len; a.xh_head = c.xh_head; a.xh_cnt = 0;
    a.u0 = -(P2pad - 1); a.n_fwd = 2 * P2pad - 1;
    a.debug_skip = 0;
    hipError_t e = launch_conv_lb_forward(a, st);
    const int keep = 0xF & ~(1 << path);
    for (int pair = 0; pair < 2 && e == hipSuccess; ++pair) {
        e = launch_conv_lb_build_cd(c.d_lb_ab, P2pad, c.d_lb_cd_alt, st, 1 << pair);
        if (e != hipSuccess) break;
        ConvLbArgs m = a;
        m.cd = c.d_lb_cd_alt; m.n_big = P2pad;
        m.out = c.d_xhist_alt; m.out_stream_stride = 2 * Lt; m.out_ch_stride = Lt;      // [S][2][Lt]: re -> ch 0, im -> ch 1
        m.io_frame0 = 0; m.io_frames = Lt;
        e = launch_conv_lb_mac_inverse(m, st);
        if (e == hipSuccess)
            e = launch_conv_lb_tails_merge(c.pt_active ? c.d_ptail : nullptr, c.pt_pos, c.d_xhist_alt, c.d_ptail_alt, Lt, pair, keep,
                                           (int)c.S, st, c.fp_mode);
    }
    if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("pending tails: ") + hipGetErrorString(e));
    std::swap(c.d_ptail, c.d_ptail_alt);
    c.pt_pos = 0; c.pt_active = true;
    // every path forgets its past: the history, the block-512 ring and overlaps, the window ring
    HIP_TRY(hipMemsetAsync(c.d_xhist, 0, c.S * 2 * (size_t)(2 * c.xh_len) * sizeof(float), st));
    c.xh_head = 0; c.xh_valid = c.xh_len; c.lb_valid = 0; c.lb_lazy = false; c.tails_lazy = false;
    HIP_TRY(hipMemsetAsync(c.d_hist, 0, c.S * (size_t)c.cap * NF * sizeof(float2), st));
    HIP_TRY(hipMemsetAsync(c.d_tails, 0, c.S * 2 * 8 * 64 * sizeof(float2), st));
    for (int p = 0; p < 4; ++p) c.since[p] = 0;
    HIP_TRY(hipStreamSynchronize(st));
    *taken = true;
    return OHS_OK;
}

static int conv_lb_launch(ConvState &c, DeviceCtx *ctx, const ConvCall &k, hipStream_t st, int &ranges)
{
    ConvLbArgs a;
    {
        const int rcp = conv_lb_prepare(c, ctx, st, a);
        if (rcp) return rcp;
    }
    const int P2pad = a.P2pad;
    const long long SEG = lb_segment_blocks(c.S);
    const long long frames_total = (long long)k.n_blocks * BS;
    const long long nbig_total = ((long long)c.cnt * BS + frames_total - 1) / kLbBlock - (long long)c.cnt * BS / kLbBlock + 1;
    const int cap_need = (int)(std::min(SEG, (nbig_total + kLbTile - 1) / kLbTile * kLbTile) + P2pad - 1);
    {
        const int rcr = conv_lb_ring_reserve(c, cap_need, st);
        if (rcr) return rcr;
    }
    a.n_streams = (int)c.S; a.gain = k.gain; a.cd = c.d_lb_cd;
    a.ring = c.d_lb_ring; a.ring_cap = c.lb_ring_cap;
    a.in_stream_stride = k.in_ss; a.in_ch_stride = k.in_cs; a.out_stream_stride = k.out_ss; a.out_ch_stride = k.out_cs;
    a.xh_len = c.xh_len;
    // The call's frames on the stream's absolute grid of 2048-frame blocks: [abs0, absE) touches blocks Ba .. Bl.  Segments of
    // at most SEG blocks; the first may start inside a block (its earlier frames come from the input history and its
    // output frames in front of the call are not stored), the last may end inside one (zeros behind the call; recomputed by
    // the next call).
    const long long abs0 = (long long)c.cnt * BS, absE = abs0 + frames_total;
    const long long Ba = abs0 / kLbBlock, Bl = (absE - 1) / kLbBlock;
    int tiles_last = 0, tile_blocks = kLbTile;
    for (long long Bs = Ba; Bs <= Bl; Bs += SEG) {
        const long long Be = std::min<long long>(Bs + SEG, Bl + 1);
        const int n_big = (int)(Be - Bs);
        const long long f_lo = std::max(abs0, Bs * kLbBlock), f_hi = std::min(absE, Be * kLbBlock);    // the call's frames in this segment
        // does the ring hold the complete windows in front of this segment?
        const bool cont = c.lb_end == Bs && c.lb_valid >= P2pad - 1;
        const int warm = cont ? 0 : P2pad - 1;
        a.in = k.in + (f_lo - abs0); a.out = k.out + (f_lo - abs0);
        a.io_frame0 = f_lo - Bs * kLbBlock; a.io_frames = f_hi - f_lo;
        // (the forward kernel appends the segment's last frames to the input history itself -- before the inverse kernel may
        // overwrite them in place --, into the half of the ring its windows do not read)
        const long long xcnt = std::min<long long>(a.io_frames, c.xh_len);
        a.xhist = c.d_xhist; a.xh_append = c.d_xhist; a.xh_head = c.xh_head; a.xh_cnt = xcnt;
        a.u0 = -warm; a.n_fwd = warm + n_big; a.n_big = n_big;
        a.ring_base = Bs + 4ll * c.lb_ring_cap;
        hipError_t e = launch_conv_lb_forward(a, st);
        if (e == hipSuccess) {
            c.xh_head = (c.xh_head + xcnt) % (2 * c.xh_len);
            e = launch_conv_lb_mac_inverse(a, st, &tile_blocks);
        }
        if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("block-2048 launch: ") + hipGetErrorString(e));
        const long long complete = f_hi / kLbBlock - Bs;          // blocks of this segment whose last frame is known
        c.lb_valid = std::min<long long>((cont ? c.lb_valid : warm) + complete, c.lb_ring_cap - 1);
        c.lb_end = Bs + complete;
        tiles_last = (n_big + tile_blocks - 1) / tile_blocks;
    }
    c.xh_valid = std::min(c.xh_len, c.xh_valid + frames_total);
    c.lb_lazy = true;
    ranges = tiles_last;
    return OHS_OK;
}

// Block 8192 / FFT 16384, one kernel (conv_xb_kernels.hip): long out-of-place calls on responses of at most two 8192-tap
// partitions.  It starts from the input history like the block-2048 plan and leaves the same state behind (the history
// advanced; the block-2048 window ring does not see the call's blocks).
// where the block-8192 kernel pays among the calls the large-block plans serve (out of place only: the caller checks)
bool conv_plan_auto_is_xb(size_t S, long long n_blocks, int Pmax)
{
    const Tuning &tn = tuning();
    const int P2x = (Pmax + 15) / 16;
    return P2x <= 2 && Pmax >= tn.xb_min_p && n_blocks >= tn.xb_min_blocks && (P2x == 1 || (long long)S >= tn.xb_min_streams_p2);
}

static int conv_xb_launch(ConvState &c, DeviceCtx *ctx, const ConvCall &k, int P2, hipStream_t st, int &ranges)
{
    if (c.xb_p2 != P2 || !c.d_xb_cd) {
        c.xb_p2 = 0; c.xb_cd_gen = 0;
        int rc = conv_realloc(c.d_xb_cd, (size_t)P2 * 2 * kXbBlock * sizeof(float4), st);
        if (rc == OHS_OK) rc = conv_realloc(c.d_xb_ab, (size_t)2 * P2 * kXbBlock * sizeof(float4), st);
        if (rc) return rc;
        c.xb_p2 = P2;
    }
    ConvXbArgs a;
    std::memset(&a, 0, sizeof(a));
    a.tw = ctx->d_tw; a.tw16384 = ctx->d_tw16384; a.P2 = P2;
    if (c.xb_cd_gen != c.lb_tables_gen) {
        if (c.irl_len < (long long)P2 * kXbBlock) return fail(OHS_ERR_HIP, "block-8192 plan: impulse responses not stored");
        ConvXbArgs t = a;
        t.in = c.d_irl; t.in_stream_stride = 2 * c.irl_len; t.in_ch_stride = c.irl_len; t.io_frames = c.irl_len;
        t.n_streams = 2; t.n_blk = P2; t.run = 1; t.ab = c.d_xb_ab; t.tables_mode = 1;
        t.fp_mode = 0;      // (tables are built in IEEE arithmetic, like k_ir_spectrum's)
        hipError_t e = launch_conv_xb(t, st);
        if (e == hipSuccess) e = launch_conv_xb_build_cd(reinterpret_cast<const float2 *>(c.d_xb_ab), P2, c.d_xb_cd, st);
        if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("block-8192 tables: ") + hipGetErrorString(e));
        c.xb_cd_gen = c.lb_tables_gen;
    }
    const long long frames = (long long)k.n_blocks * BS;
    a.in = k.in; a.out = k.out;
    a.in_stream_stride = k.in_ss; a.in_ch_stride = k.in_cs; a.out_stream_stride = k.out_ss; a.out_ch_stride = k.out_cs;
    a.xhist = c.d_xhist; a.xh_len = c.xh_len; a.xh_head = c.xh_head;
    a.io_frames = frames; a.n_streams = (int)c.S; a.n_blk = (int)((frames + kXbBlock - 1) / kXbBlock);
    a.run = conv_xb_run_for(a.n_streams, a.n_blk, P2, ctx->num_cus);
    a.cd = c.d_xb_cd; a.gain = k.gain; a.fp_mode = c.fp_mode; a.stagger = tuning().xb_stagger;
    // the call's last frames join the input history: appended by the kernel itself, into the half of the ring it does not read
    const long long xcnt = std::min(frames, c.xh_len);
    a.xh_append = c.d_xhist; a.xh_cnt = xcnt;
#ifdef OHS_EXPERIMENTS
    if (tuning().xb_run > 0) a.run = std::min(tuning().xb_run, a.n_blk);
    a.debug_skip = tuning().xb_skip;
#endif
    hipError_t e = launch_conv_xb(a, st);
    if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("block-8192 launch: ") + hipGetErrorString(e));
    c.xh_head = (c.xh_head + xcnt) % (2 * c.xh_len);
    c.xh_valid = std::min(c.xh_len, c.xh_valid + frames);
    c.lb_valid = 0;             // (the block-2048 window ring has not seen these blocks)
    c.lb_lazy = true;
    ranges = (a.n_blk + a.run - 1) / a.run;
    return OHS_OK;
}

// set_ir (convolution.rs:111-139) for one path; `ir` is a host pointer, or a device pointer on the state's
// device when ir_on_device (the node-level batch hands over what RCCL has just broadcast)
int conv_set_ir(ConvState &c, DeviceCtx *ctx, int path, const float *ir, size_t len, hipStream_t st,
                bool ir_on_device)
{
    if (path < 0 || path > 3) return fail(OHS_ERR_INVALID_ARG, "path must be 0..3");
    if (len && !ir) return fail(OHS_ERR_INVALID_ARG, "ir is NULL");
    if (len > (size_t)1 << 30) return fail(OHS_ERR_INVALID_ARG, "ir too long");
    const int P = len == 0 ? 1 : (int)((len + BS - 1) / BS);
    DeviceWideSection dws;      // (frees / device-wide waits below: no resident kernel may be in their way)
    c.pre_cnt = ~0ull;          // sums computed ahead belong to the old response and the old `since`
    if (c.lazy_ok && !c.d_xhist && c.tails_lazy && c.d_last_in) {
        // The first response of several partitions on an object that has run the one-partition fast path so far: no input
        // history was kept, but one-partition paths reach back 511 frames only, and the fast path's state at rest holds
        // the last block's 512 input frames.  Seeded with those, the history vouches for every path's reach, and the
        // reset below can carry the other paths' past as pending tails.
        int Pmax_after = P;
        for (int p = 0; p < 4; ++p)
            if (p != path) Pmax_after = std::max(Pmax_after, c.P[p]);
        if (conv_max_p(c) == 1 && Pmax_after >= lb_min_p()) {
            const long long want = lb_p2pad_for(Pmax_after) * kLbBlock;
            const size_t bytes = c.S * 2 * (size_t)want * sizeof(float);
            float *n = nullptr, *n2 = nullptr;
            HIP_TRY(hipMalloc(&n, 2 * bytes));
            if (hipMalloc(&n2, bytes) != hipSuccess) { hipFree(n); return fail(OHS_ERR_HIP, "hipMalloc(input history) failed"); }
            hipError_t e = hipMemsetAsync(n, 0, 2 * bytes, st);
            if (e == hipSuccess)        // frames -512 .. -1 at ring positions 0 .. 511, the next frame goes to 512
                e = hipMemcpy2DAsync(n, (size_t)(2 * want) * sizeof(float), c.d_last_in, (size_t)BS * sizeof(float),
                                     (size_t)BS * sizeof(float), c.S * 2, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) { hipFree(n); hipFree(n2); return fail(OHS_ERR_HIP, std::string("input history: ") + hipGetErrorString(e)); }
            c.d_xhist = n; c.d_xhist_alt = n2; c.xh_len = want; c.xh_head = BS; c.xh_valid = BS;
            c.lb_valid = 0; c.lb_cd_valid = false; c.lb_tables_gen++;
            const int rcr = conv_lb_irl_reserve(c, want, st);       // (the tails' tables span the new reach)
            if (rcr) return rcr;
        }
    }
    {   // an object that keeps the input history turns a reset in mid-stream into "all paths forget" + pending tails
        bool taken = false;
        const int rct = conv_lb_tail_route(c, ctx, path, st, &taken);
        if (rct) return rct;
        if (!taken && c.pt_active) {
            // tails still pending from an earlier reset: this path's row is part of the past it now forgets (e.g. the
            // second of four set_ir calls that re-load every path: nothing has been processed since the first)
            HIP_TRY(hipMemset2DAsync(c.d_ptail + (size_t)path * c.pt_len, 4 * (size_t)c.pt_len * sizeof(float), 0,
                                     (size_t)c.pt_len * sizeof(float), c.S, st));
        }
    }
    {   // the overlaps at rest belong to the spectra that are about to be replaced
        const int rcm = conv_materialise_state(c, ctx, st);
        if (rcm) return rcm;
    }
    // every failure path below frees what it allocated: a HIP_TRY inside the lambda returns from the
    // lambda only, the buffers are released after it
    float2 *nH = nullptr;
    float *d_ir = nullptr;
    auto body = [&]() -> int {
        HIP_TRY(hipMalloc(&nH, (size_t)P * NF * sizeof(float2)));
        if (len == 0) {
            HIP_TRY(hipMemsetAsync(nH, 0, NF * sizeof(float2), st));   // :114-118 mute
        } else {
            const float *src = ir;
            if (!ir_on_device) {
                HIP_TRY(hipMalloc(&d_ir, len * sizeof(float)));
                HIP_TRY(hipMemcpyAsync(d_ir, ir, len * sizeof(float), hipMemcpyHostToDevice, st));
                src = d_ir;
            }
            HIP_TRY(launch_ir_spectrum(src, (int)len, P, nH, ctx->d_tw, st));
            if (c.d_irt && P == 1) {        // the overlap-save plan builds its 2048-point tables from the taps themselves
                HIP_TRY(hipMemsetAsync(c.d_irt + path * BS, 0, BS * sizeof(float), st));
                HIP_TRY(hipMemcpyAsync(c.d_irt + path * BS, src, len * sizeof(float), hipMemcpyDeviceToDevice, st));
            }
        }
        if (c.d_irt && len == 0) HIP_TRY(hipMemsetAsync(c.d_irt + path * BS, 0, BS * sizeof(float), st));
        int rc = conv_grow_ring(c, P, st);
        if (rc) return rc;
        // one wait: the spectrum kernel has read d_ir, and nothing queued earlier on `st` still reads the
        // old d_H[path]
        HIP_TRY(hipStreamSynchronize(st));
        return OHS_OK;
    };
    const int rc0 = body();
    if (d_ir) hipFree(d_ir);
    if (rc0) { if (nH) hipFree(nH); return rc0; }
    if (c.lazy_ok) {
        const int rcl = conv_lb_store_ir(c, path, ir_on_device ? ir : nullptr, ir_on_device ? nullptr : ir, len, P, st);
        if (rcl) { hipFree(nH); return rcl; }
    }
    hipFree(c.d_H[path]);
    c.d_H[path] = nH;
    c.P[path] = P;
    c.spk_set[path] = false;
    c.cd_os_valid = false;
    c.cd_valid = false;
    c.cdm_valid = false;
    c.since[path] = 0;      // :135-137 that path's history is "all zero" again
    if (conv_since_zero(c)) {
        // every path has forgotten its past: the ring holds nothing any path may still see.  Zeroing
        // it lets the gate-free time-parallel kernels run right away (all `since` equal).
        HIP_TRY(hipMemsetAsync(c.d_hist, 0, c.S * (size_t)c.cap * NF * sizeof(float2), st));
    }
    {
        const int rcx = conv_lb_after_set_ir(c, st);
        if (rcx) return rcx;
    }
    // :138 that path's overlap := 0.  Tails are (lsl + j lsr) and (rsl + j rsr).
    const int which = path >> 1, comp = path & 1;
    HIP_TRY(launch_zero_tail_component(c.d_tails, (long long)c.S, which, comp, st));
    HIP_TRY(hipStreamSynchronize(st));
    return OHS_OK;
}

// The set table of the IR-scheduled call.  Per set: the four spectra by k_ir_spectrum (all sets' paths in one launch: the padded
// responses lie 512 apart, one "partition" each), (C, D) by k_build_cd -- the kernels set_ir and the plain call use, so that a
// block convolved with set i has the bits of a plain call on a handle that loaded set i --, then the block loop's layout once.
int conv_set_schedule_irs(ConvState &c, DeviceCtx *ctx, size_t n_sets, const float *irs, size_t len, hipStream_t st)
{
    DeviceWideSection dws;      // (frees below)
    for (void *d : std::initializer_list<void *>{c.d_irs_cd, c.d_irs_H, c.d_irs_t})
        if (d) hipFree(d);
    c.d_irs_cd = nullptr; c.d_irs_H = nullptr; c.d_irs_t = nullptr; c.irs_n = 0;
    if (n_sets == 0) return OHS_OK;
    std::vector<float> padded(n_sets * 4 * (size_t)BS, 0.0f);
    for (size_t r = 0; r < n_sets * 4; ++r) std::memcpy(&padded[r * BS], irs + r * len, len * sizeof(float));
    float2 *d_cd = nullptr;     // [n_sets][2][1024] scratch
    auto body = [&]() -> int {
        HIP_TRY(hipMalloc(&c.d_irs_t, padded.size() * sizeof(float)));
        HIP_TRY(hipMalloc(&c.d_irs_H, n_sets * 4 * (size_t)NF * sizeof(float2)));
        HIP_TRY(hipMalloc(&c.d_irs_cd, n_sets * (size_t)NF * sizeof(float4)));
        HIP_TRY(hipMalloc(&d_cd, n_sets * 2 * (size_t)NF * sizeof(float2)));
        HIP_TRY(hipMemcpyAsync(c.d_irs_t, padded.data(), padded.size() * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_TRY(launch_ir_spectrum(c.d_irs_t, (int)padded.size(), (int)(n_sets * 4), c.d_irs_H, ctx->d_tw, st));
        for (size_t i = 0; i < n_sets; ++i) {
            const float2 *h = c.d_irs_H + i * 4 * (size_t)NF;
            HIP_TRY(launch_build_cd(h, h + NF, h + 2 * NF, h + 3 * NF, d_cd + i * 2 * (size_t)NF, st));
        }
        HIP_TRY(launch_irs_tables(d_cd, (int)n_sets, c.d_irs_cd, st));
        HIP_TRY(hipStreamSynchronize(st));
        return OHS_OK;
    };
    int rc = body();
    if (d_cd) hipFree(d_cd);
    // (a shared-row call adopts a set's taps into the time-domain copies the large-transform plans build their tables from)
    if (rc == OHS_OK && c.lazy_ok) rc = conv_lb_irl_reserve(c, lb_p2pad_for(1) * kLbBlock, st);
    if (rc) {
        for (void *d : std::initializer_list<void *>{c.d_irs_cd, c.d_irs_H, c.d_irs_t})
            if (d) hipFree(d);
        c.d_irs_cd = nullptr; c.d_irs_H = nullptr; c.d_irs_t = nullptr;
        return rc;
    }
    c.irs_n = n_sets;
    return OHS_OK;
}

// units "sets" of four responses each -> dst[units][1024] float4.  rows(u, r) is response r (0 .. 3) of unit u, `len` taps, or nullptr
// for an all-zero one.  Built in slices of 1 024 units, host staging and device scratch alike, so that neither grows with the table
// (and k_irs_tables' grid stays small).
template <class Rows>
static int layout_build_tables(DeviceCtx *ctx, size_t units, size_t len, Rows rows, float4 *dst, hipStream_t st)
{
    constexpr size_t kSlice = 1024;
    const size_t slice = std::min(units, kSlice);
    std::vector<float> padded;  // [slice][4][512]
    try {
        padded.resize(slice * 4 * (size_t)BS);
    } catch (const std::bad_alloc &) {
        return fail(OHS_ERR_HIP, "out of host memory for the table's staging");
    }
    float *d_t = nullptr;       // [slice][4][512] scratch
    float2 *d_H = nullptr;      // [slice][4][1024] scratch
    float2 *d_cd = nullptr;     // [slice][2][1024] scratch
    auto body = [&]() -> int {
        HIP_TRY(hipMalloc(&d_t, slice * 4 * (size_t)BS * sizeof(float)));
        HIP_TRY(hipMalloc(&d_H, slice * 4 * (size_t)NF * sizeof(float2)));
        HIP_TRY(hipMalloc(&d_cd, slice * 2 * (size_t)NF * sizeof(float2)));
        for (size_t u0 = 0; u0 < units; u0 += slice) {
            const size_t n = std::min(slice, units - u0);
            std::fill(padded.begin(), padded.end(), 0.0f);
            for (size_t u = 0; u < n; ++u)
                for (size_t r = 0; r < 4; ++r)
                    if (const float *src = rows(u0 + u, r)) std::memcpy(&padded[(u * 4 + r) * BS], src, len * sizeof(float));
            HIP_TRY(hipMemcpyAsync(d_t, padded.data(), n * 4 * (size_t)BS * sizeof(float), hipMemcpyHostToDevice, st));
            HIP_TRY(launch_ir_spectrum(d_t, (int)(n * 4 * (size_t)BS), (int)(n * 4), d_H, ctx->d_tw, st));
            for (size_t p = 0; p < n; ++p) {
                const float2 *h = d_H + p * 4 * (size_t)NF;
                HIP_TRY(launch_build_cd(h, h + NF, h + 2 * NF, h + 3 * NF, d_cd + p * 2 * (size_t)NF, st));
            }
            HIP_TRY(launch_irs_tables(d_cd, (int)n, dst + u0 * (size_t)NF, st, kLayoutTableScale));
            HIP_TRY(hipStreamSynchronize(st));      // (staging and scratch are reused by the next slice)
        }
        return OHS_OK;
    };
    const int rc = body();
    for (void *d : std::initializer_list<void *>{d_t, d_H, d_cd})
        if (d) hipFree(d);
    return rc;
}

// the layout overlap, shared by the single layout, the table of layouts and the scenes' direction table: allocated while any of them
// exists, zeroed by every upload
static int layout_overlap_zeroed(ConvState &c, hipStream_t st)
{
    if (!c.d_lay_ov) HIP_TRY(hipMalloc(&c.d_lay_ov, c.S * 8 * 64 * sizeof(float2)));
    if (!c.d_lay_ov_alt) HIP_TRY(hipMalloc(&c.d_lay_ov_alt, c.S * 8 * 64 * sizeof(float2)));
    HIP_TRY(hipMemsetAsync(c.d_lay_ov, 0, c.S * 8 * 64 * sizeof(float2), st));
    return OHS_OK;
}

static void layout_overlap_release_if_unused(ConvState &c)
{
    if (c.d_lay_cd || c.d_lays_cd || c.d_obj_ah) return;
    for (void *d : std::initializer_list<void *>{c.d_lay_ov, c.d_lay_ov_alt})
        if (d) hipFree(d);
    c.d_lay_ov = nullptr; c.d_lay_ov_alt = nullptr;
}

// One upload for the single layout and the table of layouts alike: `units` sets of four responses (rows, as layout_build_tables reads
// them) into a fresh *d_cd, the layout overlap zeroed.  The caller has freed the old *d_cd; on an error nothing is left behind.
template <class Rows>
static int layout_upload(ConvState &c, DeviceCtx *ctx, size_t units, size_t len, Rows rows, float4 **d_cd, hipStream_t st)
{
    auto body = [&]() -> int {
        HIP_TRY(hipMalloc(d_cd, units * (size_t)NF * sizeof(float4)));
        const int rco = layout_overlap_zeroed(c, st);
        if (rco) return rco;
        const int rct = layout_build_tables(ctx, units, len, rows, *d_cd, st);
        if (rct) return rct;
        HIP_TRY(hipStreamSynchronize(st));
        return OHS_OK;
    };
    const int rc = body();
    if (rc) {
        if (*d_cd) hipFree(*d_cd);
        *d_cd = nullptr;
        layout_overlap_release_if_unused(c);
    }
    return rc;
}

// The speaker layout of ohs_batch_process_layout.  irs[c][e] is row 2 c + e, so the four rows of pair p -- channel 2 p to both ears,
// channel 2 p + 1 to both ears -- are the four paths Lsl, Lsr, Rsl, Rsr of a "set": the spectra by k_ir_spectrum, (C, D) by k_build_cd,
// the block loop's layout by k_irs_tables, exactly as conv_set_schedule_irs builds a set (K = 2: the bits of a plain call on a handle
// that loaded those four responses).  Odd K: the last pair's second channel has two all-zero rows.
int conv_set_layout_irs(ConvState &c, DeviceCtx *ctx, size_t n_channels, const float *irs, size_t len, hipStream_t st)
{
    DeviceWideSection dws;      // (frees below)
    if (c.d_lay_cd) hipFree(c.d_lay_cd);
    c.d_lay_cd = nullptr; c.lay_K = 0; c.lay_len = 0;
    if (n_channels == 0) {
        layout_overlap_release_if_unused(c);
        if (c.d_lay_ov) {       // (a table of layouts keeps the slabs: zeroed, as behind every upload)
            HIP_TRY(hipMemsetAsync(c.d_lay_ov, 0, c.S * 8 * 64 * sizeof(float2), st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        return OHS_OK;
    }
    // (unit p = pair p: rows irs[2 p][0], irs[2 p][1], irs[2 p + 1][0], irs[2 p + 1][1]; an odd last channel has a zero partner)
    auto rows = [&](size_t p, size_t r) -> const float * { return 4 * p + r < 2 * n_channels ? irs + (4 * p + r) * len : nullptr; };
    const int rc = layout_upload(c, ctx, (n_channels + 1) / 2, len, rows, &c.d_lay_cd, st);
    if (rc) return rc;
    c.lay_K = n_channels; c.lay_len = len;
    return OHS_OK;
}

// The table of layouts of ohs_batch_process_layout_scheduled: set j, pair p is "set" j * P + p of the same chain, so a block on set j
// has the bits of ohs_batch_process_layout on a handle that loaded irs[j].
int conv_set_layout_schedule_irs(ConvState &c, DeviceCtx *ctx, size_t n_sets, size_t n_channels, const float *irs, size_t len,
                                 hipStream_t st)
{
    DeviceWideSection dws;      // (frees below)
    if (c.d_lays_cd) hipFree(c.d_lays_cd);
    c.d_lays_cd = nullptr; c.lays_n = 0; c.lays_K = 0; c.lays_len = 0;
    if (n_sets == 0) {
        layout_overlap_release_if_unused(c);
        return OHS_OK;
    }
    const size_t P = (n_channels + 1) / 2;
    auto rows = [&](size_t u, size_t r) -> const float * {      // (unit u = set u / P, pair u % P)
        const size_t j = u / P, q = 4 * (u % P) + r;
        return q < 2 * n_channels ? irs + (j * 2 * n_channels + q) * len : nullptr;
    };
    const int rc = layout_upload(c, ctx, n_sets * P, len, rows, &c.d_lays_cd, st);
    if (rc) return rc;
    c.lays_n = n_sets; c.lays_K = n_channels; c.lays_len = len;
    return OHS_OK;
}

// What the two layout kernels share of a launch: the chunks per stream -- conv_p1_chunks' rule for this kernel's resident waves, capped
// to 1 / 2 / 4 / 8 / 16 as conv_choose_plan caps k_conv_p1_irs (every chunk but the first pays a dry block; there is no pre-pass) --
// and the arguments around the layout's own.  n_blocks > 0.
static ConvP1Args layout_launch_args(const ConvState &c, DeviceCtx *ctx, const float *in, long long in_ss, long long in_cs, float *out,
                                     long long out_ss, long long out_cs, int n_blocks, float gain)
{
    const long long want = conv_p1_chunks(ctx, c.S, n_blocks, 0, 8, conv_layout_waves_per_cu());
    int K = 16;
    while (K > want || K > n_blocks) K >>= 1;
    ConvP1Args a{};
    a.in = in; a.out = out;
    a.in_stream_stride = in_ss; a.in_ch_stride = in_cs;
    a.out_stream_stride = out_ss; a.out_ch_stride = out_cs;
    a.n_blocks = n_blocks; a.n_streams = (int)c.S; a.chunks = K;
    a.tw = ctx->d_tw; a.gain = gain; a.fp_mode = c.fp_mode;
    a.xcd_lo = 0; a.xcd_n = 8;
    for (int g = 0; g < 4; ++g) a.weights[g] = 1;
    a.merged_in = c.d_lay_ov; a.merged_out = c.d_lay_ov_alt;
    a.gain_seg = 1;
    return a;
}

int conv_launch_layout(ConvState &c, DeviceCtx *ctx, const float *in, long long in_ss, long long in_cs,
                       float *out, long long out_ss, long long out_cs, int n_blocks, float gain, hipStream_t st)
{
    if (!c.d_lay_cd || c.lay_K == 0) return fail(OHS_ERR_INVALID_ARG, "no layout uploaded (ohs_batch_set_layout_irs)");
    if (n_blocks <= 0) return OHS_OK;
    const ConvP1Args a = layout_launch_args(c, ctx, in, in_ss, in_cs, out, out_ss, out_cs, n_blocks, gain);
    ConvLayoutArgs l;
    l.cd = c.d_lay_cd; l.n_channels = (int)c.lay_K; l.n_pairs = (int)((c.lay_K + 1) / 2);
    const hipError_t e = launch_conv_p1_layout(a, l, st);
    if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("conv_p1_layout launch: ") + hipGetErrorString(e));
    std::swap(c.d_lay_ov, c.d_lay_ov_alt);
    c.last_lay_pairs = l.n_pairs; c.last_lay_ranges = a.chunks; c.last_lay_scheduled = false;
    return OHS_OK;
}

// The scheduled layout call: conv_launch_layout's plan -- the same chunks per stream, the same overlap slabs --, on the table of layouts
int conv_launch_layout_scheduled(ConvState &c, DeviceCtx *ctx, const float *in, long long in_ss, long long in_cs,
                                 float *out, long long out_ss, long long out_cs, int n_blocks, float gain, hipStream_t st,
                                 const ConvLayoutRows *rows, size_t one_set)
{
    if (!c.d_lays_cd || c.lays_n == 0) return fail(OHS_ERR_INVALID_ARG, "no table uploaded (ohs_batch_set_layout_schedule_irs)");
    if (!rows && one_set >= c.lays_n) return fail(OHS_ERR_INVALID_ARG, "set index out of range");
    if (n_blocks <= 0) return OHS_OK;
    const ConvP1Args a = layout_launch_args(c, ctx, in, in_ss, in_cs, out, out_ss, out_cs, n_blocks, gain);
    const int P = (int)((c.lays_K + 1) / 2);
    hipError_t e;
    if (!rows) {
        ConvLayoutArgs l;
        l.cd = c.d_lays_cd + one_set * (size_t)P * NF; l.n_channels = (int)c.lays_K; l.n_pairs = P;
        e = launch_conv_p1_layout(a, l, st);
    } else {
        ConvLayoutIrArgs l;
        l.cd = c.d_lays_cd; l.n_channels = (int)c.lays_K; l.n_pairs = P;
        l.tab = rows->tab; l.stream = rows->stream_stride; l.seg = rows->seg_blocks;
        l.prev = rows->fade ? rows->prev : nullptr; l.prev_stream = rows->prev_stride; l.fade = rows->fade ? 1 : 0;
        e = launch_conv_p1_layout_irs(a, l, st);
    }
    if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("conv_p1_layout_irs launch: ") + hipGetErrorString(e));
    std::swap(c.d_lay_ov, c.d_lay_ov_alt);
    c.last_lay_pairs = P; c.last_lay_ranges = a.chunks; c.last_lay_scheduled = rows != nullptr;
    return OHS_OK;
}

// The direction table of the object scenes: per direction the two ear spectra by k_ir_spectrum -- the kernel every layout table starts
// from --, then k_object_tables; in slices, as layout_build_tables builds its units, so that staging and scratch do not grow with it.
int conv_set_object_dirs(ConvState &c, DeviceCtx *ctx, size_t n_dirs, const float *irs, size_t len, hipStream_t st)
{
    DeviceWideSection dws;      // (frees below)
    if (c.d_obj_ah) hipFree(c.d_obj_ah);
    c.d_obj_ah = nullptr; c.obj_n = 0; c.obj_len = 0;
    if (n_dirs == 0) {
        layout_overlap_release_if_unused(c);
        if (c.d_lay_ov) {       // (a layout keeps the slabs: zeroed, as behind every upload)
            HIP_TRY(hipMemsetAsync(c.d_lay_ov, 0, c.S * 8 * 64 * sizeof(float2), st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        return OHS_OK;
    }
    constexpr size_t kSlice = 1024;
    const size_t slice = std::min(n_dirs, kSlice);
    std::vector<float> padded;  // [slice][2][512]
    try {
        padded.resize(slice * 2 * (size_t)BS);
    } catch (const std::bad_alloc &) {
        return fail(OHS_ERR_HIP, "out of host memory for the table's staging");
    }
    float *d_t = nullptr;       // [slice][2][512] scratch
    float2 *d_H = nullptr;      // [slice][2][1024] scratch
    auto body = [&]() -> int {
        HIP_TRY(hipMalloc(&c.d_obj_ah, (n_dirs + 1) * (size_t)NF * sizeof(float2)));
        HIP_TRY(hipMemsetAsync(c.d_obj_ah + n_dirs * (size_t)NF, 0, (size_t)NF * sizeof(float2), st));    // (the odd object's partner)
        const int rco = layout_overlap_zeroed(c, st);
        if (rco) return rco;
        HIP_TRY(hipMalloc(&d_t, slice * 2 * (size_t)BS * sizeof(float)));
        HIP_TRY(hipMalloc(&d_H, slice * 2 * (size_t)NF * sizeof(float2)));
        for (size_t u0 = 0; u0 < n_dirs; u0 += slice) {
            const size_t n = std::min(slice, n_dirs - u0);
            std::fill(padded.begin(), padded.end(), 0.0f);
            for (size_t r = 0; r < 2 * n; ++r) std::memcpy(&padded[r * BS], irs + (2 * u0 + r) * len, len * sizeof(float));
            HIP_TRY(hipMemcpyAsync(d_t, padded.data(), n * 2 * (size_t)BS * sizeof(float), hipMemcpyHostToDevice, st));
            HIP_TRY(launch_ir_spectrum(d_t, (int)(n * 2 * (size_t)BS), (int)(n * 2), d_H, ctx->d_tw, st));
            HIP_TRY(launch_object_tables(d_H, (int)n, c.d_obj_ah + u0 * (size_t)NF, st));
            HIP_TRY(hipStreamSynchronize(st));      // (staging and scratch are reused by the next slice)
        }
        return OHS_OK;
    };
    const int rc = body();
    for (void *d : std::initializer_list<void *>{d_t, d_H})
        if (d) hipFree(d);
    if (rc) {
        if (c.d_obj_ah) hipFree(c.d_obj_ah);
        c.d_obj_ah = nullptr;
        layout_overlap_release_if_unused(c);
        return rc;
    }
    c.obj_n = n_dirs; c.obj_len = len;
    return OHS_OK;
}

// The scene call: conv_launch_layout's plan -- the same chunks per stream, the same overlap slabs --, on the direction table
int conv_launch_objects(ConvState &c, DeviceCtx *ctx, const float *in, long long in_ss, long long in_cs, float *out, long long out_ss,
                        long long out_cs, int n_blocks, float gain, hipStream_t st, int n_objects, const ConvObjectRows &rows)
{
    if (!c.d_obj_ah || c.obj_n == 0) return fail(OHS_ERR_INVALID_ARG, "no direction table uploaded (ohs_scene_set_direction_irs)");
    if (n_blocks <= 0) return OHS_OK;
    const ConvP1Args a = layout_launch_args(c, ctx, in, in_ss, in_cs, out, out_ss, out_cs, n_blocks, gain);
    ConvObjectsArgs l;
    l.ahalf = c.d_obj_ah; l.zero_dir = (unsigned)c.obj_n; l.n_objects = n_objects; l.n_pairs = (n_objects + 1) / 2;
    l.idx = rows.idx; l.gain = rows.gain; l.stream = rows.stream_stride; l.seg = rows.seg_blocks;
    l.prev_idx = rows.fade ? rows.prev_idx : nullptr; l.prev_gain = rows.fade ? rows.prev_gain : nullptr;
    l.prev_stream = rows.prev_stride; l.fade = rows.fade ? 1 : 0;
    const hipError_t e = launch_conv_p1_objects(a, l, st);
    if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("conv_p1_objects launch: ") + hipGetErrorString(e));
    std::swap(c.d_lay_ov, c.d_lay_ov_alt);
    c.last_obj_pairs = l.n_pairs; c.last_obj_ranges = a.chunks;
    return OHS_OK;
}

// The blended scene calls: conv_launch_objects's plan on the same table, every object between two directions (n_dirs = 2:
// k_conv_p1_objects_blend) or inside a triangle of three (n_dirs = 3: k_conv_p1_objects_blend3)
int conv_launch_objects_blend(ConvState &c, DeviceCtx *ctx, const float *in, long long in_ss, long long in_cs, float *out, long long out_ss,
                              long long out_cs, int n_blocks, float gain, hipStream_t st, int n_objects, int n_dirs,
                              const ConvObjectBlendRows &rows)
{
    const bool tri = n_dirs == 3;
    if (!c.d_obj_ah || c.obj_n == 0)
        return fail(OHS_ERR_INVALID_ARG, tri ? "no direction table uploaded (ohs_scene3_set_direction_irs)"
                                             : "no direction table uploaded (ohs_scene2_set_direction_irs)");
    if (n_blocks <= 0) return OHS_OK;
    const ConvP1Args a = layout_launch_args(c, ctx, in, in_ss, in_cs, out, out_ss, out_cs, n_blocks, gain);
    ConvObjectsBlendArgs l;
    l.ahalf = c.d_obj_ah; l.zero_dir = (unsigned)c.obj_n; l.n_objects = n_objects; l.n_pairs = (n_objects + 1) / 2;
    l.rows = rows.rows; l.plane = rows.plane; l.has_gain = rows.has_gain ? 1 : 0; l.stream = rows.stream_stride; l.seg = rows.seg_blocks;
    l.prev = rows.fade ? rows.prev : nullptr; l.prev_plane = rows.prev_plane; l.prev_stream = rows.prev_stride; l.fade = rows.fade ? 1 : 0;
    const hipError_t e = tri ? launch_conv_p1_objects_blend3(a, l, st) : launch_conv_p1_objects_blend(a, l, st);
    if (e != hipSuccess)
        return fail(OHS_ERR_HIP, std::string(tri ? "conv_p1_objects_blend3 launch: " : "conv_p1_objects_blend launch: ") + hipGetErrorString(e));
    std::swap(c.d_lay_ov, c.d_lay_ov_alt);
    c.last_obj_pairs = l.n_pairs; c.last_obj_ranges = a.chunks;
    return OHS_OK;
}

// What four set_ir calls would load, without their resets: spectra, time-domain copies, every derived table invalid.
int conv_adopt_schedule_set(ConvState &c, size_t set, hipStream_t st)
{
    if (set >= c.irs_n || conv_max_p(c) != 1) return fail(OHS_ERR_INVALID_ARG, "no such set, or a response longer than one partition");
    c.pre_cnt = ~0ull;
    for (int p = 0; p < 4; ++p) {
        const size_t row = set * 4 + (size_t)p;
        HIP_TRY(hipMemcpyAsync(c.d_H[p], c.d_irs_H + row * NF, NF * sizeof(float2), hipMemcpyDeviceToDevice, st));
        if (c.d_irt) HIP_TRY(hipMemcpyAsync(c.d_irt + p * BS, c.d_irs_t + row * BS, BS * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (c.d_irl && c.irl_len >= BS) {
            HIP_TRY(hipMemsetAsync(c.d_irl + (size_t)p * c.irl_len, 0, (size_t)c.irl_len * sizeof(float), st));
            HIP_TRY(hipMemcpyAsync(c.d_irl + (size_t)p * c.irl_len, c.d_irs_t + row * BS, BS * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
        c.spk_set[p] = false;
    }
    c.cd_valid = false; c.cd_os_valid = false; c.cdm_valid = false;
    c.lb_cd_valid = false; c.lb_tables_gen++;
    return OHS_OK;
}

// Chunks per stream of the P = 1 kernel: at least ONE round of resident waves (CUs x 16), and a wave count S * K that
// FILLS its last round -- all waves of a launch take the same time, so 2.13 rounds cost 3 (1024 and 2048 streams with
// K = ceil(2 R / S) ran at 71 % for that reason).  K is the smallest value from ceil(R / S) upwards whose last round is
// >= 97 % full.  (Rounds 1 and 2 asked for two rounds; since the chunk lengths follow the waves' age ranks one exact
// round is the faster plan -- config 3 without EQ: 4096 waves 0.537-0.541 ms, 8192 waves 0.549-0.555, 3840 0.563,
// 4352 0.81 -- and the pre-pass has half the boundary tails to compute.  Tuning::p1_rounds = 2 restores the old rule.)
// waves_per_cu == 0: k_conv_p1 and its kin, whose resident waves per CU follow the tuning (16 by default).  waves_per_cu > 0 is
// the rule for ANOTHER kernel of the family with that many resident waves per CU -- k_conv_p1_layout, 12 -- and changes three
// things: the round R = CUs x waves_per_cu; the one-chunk -> two-chunk rule below is off (it belongs to k_conv_p1's deal of
// chunks over age ranks); and a short launch always prices 2 / 4 / 8 / 16 chunks as computing their own boundary tails,
// because such a kernel has no pre-pass at all.
long long conv_p1_chunks(const DeviceCtx *ctx, size_t S, long long n_blocks, long long target_override, int xcd_n, int waves_per_cu)
{
    const int wpc = waves_per_cu > 0 ? waves_per_cu : conv_p1_waves_per_cu();
    const long long R = (long long)ctx->num_cus * xcd_n / 8 * wpc;
    long long K;
    if (target_override > 0) {
        K = (target_override + (long long)S - 1) / (long long)S;
    } else {
        const long long rounds = tuning().p1_rounds;
        const long long k0 = std::max<long long>(1, (rounds * R + (long long)S - 1) / (long long)S);
        K = k0;
        double best = 0.0;
        for (long long k = k0; k < k0 + 32; ++k) {
            const double rd = (double)((long long)S * k) / (double)R;
            const double eff = rd / std::ceil(rd - 1e-9);
            if (eff > best + 1e-9) { best = eff; K = k; }
            if (eff >= 0.97) break;
        }
    }
    // One chunk per stream (4096 streams and more) leaves the age ranks nothing to balance: two chunks, dealt out over
    // ranks {0, 3} / {1, 2} (conv_kernels.hip: p1_wave_job), cost a second round but end together -- 4096 streams: 8.9 ->
    // 8.0 ms of convolution per step.
    if (K == 1 && n_blocks >= 16 && target_override <= 0 && wpc == 16) K = 2;
    if (n_blocks < 4 * K && target_override <= 0) {
        // A short launch (the last, 2 % time chunk of an overlapped batch step: 19 blocks), a few blocks per wave at
        // best: every chunk boundary costs the pre-pass a block's work, and a wave count just above a round starts a second,
        // almost empty one.  Cost in block times: rounds x blocks per wave for the main kernel + rounds for the boundary
        // tails (one more block per wave where the chunks' own waves compute them -- K = 2, 4, 8, 16 --, else a pre-pass
        // launch: its rounds + about a block time of launch); the smallest K of minimal cost (19 blocks x 256 streams:
        // K = 16, one round of at most 2 + 1 blocks, no pre-pass).
        const bool own_ok = wpc == 16 || waves_per_cu > 0;    // (the layout kernel's chunks always compute their own)
        long long best_k = std::min(K, n_blocks), best_cost = -1;
        for (long long k = 1; k <= std::min(K, n_blocks); ++k) {
            const long long rounds_main = ((long long)S * k + R - 1) / R, per_wave = (n_blocks + k - 1) / k;
            long long cost;
            if (k == 1) cost = rounds_main * per_wave;
            else if (own_ok && (k == 2 || k == 4 || k == 8 || k == 16)) cost = rounds_main * (per_wave + 1);
            else cost = rounds_main * per_wave + ((long long)S * (k - 1) + R - 1) / R + 1;
            if (best_cost < 0 || cost < best_cost) { best_cost = cost; best_k = k; }
        }
        K = best_k;
    }
    if (K > n_blocks) K = n_blocks;
    if (K < 1) K = 1;
    return K;
}

// ohs_batch_set_conv_plan(0): which P = 1 plan the library picks by itself
// The hop-1536 plan does a quarter less work per frame at three waves per SIMD and wins wherever the convolution's time
// is exposed and the launch can fill the chip (profiles/r04_conv_plan_ab_run3.txt, _run4.txt):
//   out of place (the call's hop ranges are independent: any count per stream): 0.944 x the block-512 plan's time at 256
//     streams, 0.87-0.89 x from 384 on; a tie at 128 and below
//   in place (a stream's ranges share a workgroup: 1, 2, 3, 4, 6 or 12 of them): 0.93 x at 512 streams, 0.87-0.92 x beyond;
//     a tie at 384.  The batch's EQ || convolution path is in place: at 256 streams with the EQ on -- BASELINE configs[2] --
//     the convolution hides under the EQ's serial chain either way (1.000-1.004 x), and the block-512 plan keeps its two
//     properties there: output bits that do not depend on where the calls cut the signal, and the recorded golden hash.
// Short calls stay with the block-512 plan as well (a wave's first and last hops run the guarded form of the hop).
bool conv_plan_auto_is_os(size_t S, long long n_blocks, bool in_place)
{
    return n_blocks >= 48 && S >= (in_place ? 512u : 256u);
}

// hop ranges per stream of the hop-1536 plan: rounds of resident waves x hops per wave (+ 1: the tables and the first
// window), the smallest count of minimal cost.  In place all of a stream's ranges must share a workgroup
// (launch_conv_p1_os): a divisor of its wave count; out of place any count goes, and few streams still fill the chip
// (64 streams x 48 ranges).
int conv_os_chunks(const DeviceCtx *ctx, size_t S, long long n_blocks, bool in_place)
{
    const long long R = (long long)ctx->num_cus * conv_os_waves_per_cu();
    const long long H = (n_blocks * BS + 1535) / 1536;
    int K = 1;
    long long best = -1;
    for (int k = 1; k <= (in_place ? conv_os_waves_per_cu() : 96) && k <= H; ++k) {
        if (in_place && conv_os_waves_per_cu() % k) continue;
        const long long cost = (((long long)S * k + R - 1) / R) * ((H + k - 1) / k + 1);
        if (best < 0 || cost < best) { best = cost; K = k; }
    }
    return K;
}

// What conv_choose_plan decides for a call: the kernel family, and what is decided along with it
struct ConvPlan {
    int kernel = OHS_CONV_KERNEL_NONE;  // OHS_CONV_KERNEL_*
    int K = 0;                  // one partition: time chunks (block 512) or hop ranges (hop 1536) per stream
    int xcd_lo = 0, xcd_n = 8;  // block 512, one partition: the XCDs its launches may use
    int P2x = 0;                // block 8192: partitions of 8192 taps
    bool gated = false;         // time-parallel block 512: after a per-path set_ir (k_conv_tp_old)
    long long SEG = 0;          // time-parallel block 512: blocks per segment
};

// The plan rule: which kernel family serves the call `k`.  It reads the state and tuning() only.
static ConvPlan conv_choose_plan(const ConvState &c, const DeviceCtx *ctx, const ConvCall &k, bool allow_fast)
{
    const Tuning &tn = tuning();
    const int Pmax = conv_max_p(c);
    ConvPlan plan;
    if (Pmax == 1 && allow_fast) {
        // every path has one partition: time-parallel single-FFT-pair kernel
        // Two plans for this case (ohs_batch_set_conv_plan): block 512 / FFT 1024 overlap-add (k_conv_p1: the plan whose
        // output bits tests/golden/p1_output_sha256.txt holds) and hop 1536 / FFT 2048 overlap-save (k_conv_p1_os: a third
        // less transform and product work per frame; batch objects only -- it hands the lazy state over).
        const bool os_ok = c.lazy_ok && c.d_irt && k.n_blocks >= 3 && c.xcd_n == 8 && tn.p1_xcd_n == 0 &&
                           ((k.in_ss | k.in_cs | k.out_ss | k.out_cs) & 1) == 0 &&
                           ((reinterpret_cast<uintptr_t>(k.in) | reinterpret_cast<uintptr_t>(k.out)) & 7) == 0 &&
                           (unsigned long long)k.n_blocks * BS + 1536ull < (1ull << 31);
        // (a schedule of impulse responses is always the block-512 family's: the hop-1536 windows straddle segment boundaries)
        if (!k.irs && os_ok && (c.conv_plan == 2 || (c.conv_plan == 0 && conv_plan_auto_is_os(c.S, k.n_blocks, k.in == k.out)))) {
            plan.kernel = OHS_CONV_KERNEL_HOP1536_P1;
            plan.K = conv_os_chunks(ctx, c.S, k.n_blocks, k.in == k.out);
            return plan;
        }
        plan.kernel = OHS_CONV_KERNEL_BLOCK512_P1;
        plan.xcd_lo = c.xcd_lo; plan.xcd_n = c.xcd_n;
        if (tn.p1_xcd_n > 0) { plan.xcd_lo = tn.p1_xcd_lo; plan.xcd_n = tn.p1_xcd_n; }
        plan.K = (int)conv_p1_chunks(ctx, c.S, k.n_blocks, tn.p1_target_waves, plan.xcd_n);
        if (k.irs) {    // k_conv_p1_irs has no pre-pass: 1 chunk, or 2 / 4 / 8 / 16 that compute their own boundary tails
            int K = 16;
            while (K > plan.K) K >>= 1;
            plan.K = K;
        }
        return plan;
    }
    if (allow_fast && c.d_xhist && Pmax >= lb_min_p()) {
        // Block 2048 / FFT 4096 (conv_lb_kernels.hip).  It convolves the input history itself, so every path must be
        // allowed to see all of its own response's reach of it (conv_history_covers_paths).
        const bool lb_ok = conv_history_covers_paths(c) && ((k.in_ss | k.in_cs | k.out_ss | k.out_cs) & 3) == 0 &&
                           ((reinterpret_cast<uintptr_t>(k.in) | reinterpret_cast<uintptr_t>(k.out)) & 15) == 0;
        if (lb_ok && (c.conv_plan == 2 || (c.conv_plan == 0 && conv_plan_auto_is_lb(c.S, k.n_blocks, Pmax)))) {
            // Long out-of-place calls on responses of at most two 8192-tap partitions: block 8192 / FFT 16384, one kernel (the
            // buffers must not overlap at all: a run's first windows read frames in front of its own blocks).  Where it pays
            // (profiles/r05_xb_vs_lb_shapes.txt): calls of 128 blocks or more; with two partitions, on 32 streams or more.
            const int P2x = (Pmax + 15) / 16;
            const long long call_frames = (long long)k.n_blocks * BS;
            const float *in_end = k.in + (c.S - 1) * k.in_ss + k.in_cs + call_frames;
            const float *out_end = k.out + (c.S - 1) * k.out_ss + k.out_cs + call_frames;
            const bool apart = in_end <= k.out || out_end <= k.in;
            const bool xb = apart && conv_plan_auto_is_xb(c.S, k.n_blocks, Pmax) &&
                            c.xh_len >= (long long)P2x * kXbBlock && call_frames < (1ll << 29);
            plan.kernel = xb ? OHS_CONV_KERNEL_BLOCK8192 : OHS_CONV_KERNEL_BLOCK2048;
            plan.P2x = P2x;
            return plan;
        }
    }
    bool since_old = true;
    for (int p = 0; p < 4; ++p) since_old = since_old && c.since[p] >= c.P[p] - 1;
    // gate-free condition of the time-parallel kernels: no path may have blocks in the ring that
    // it must not see (either every path is older than its own IR -- path p reads P[p] - 1 blocks back --, or all
    // were reset together: conv_set_ir zeroed the ring then)
    const bool gate_free = since_old || conv_since_equal(c);
    // Otherwise -- a per-path set_ir in mid-stream -- the same three kernels run on a ring whose old blocks they
    // cannot reach (the call starts Ppad - 1 zeroed slots further on) and k_conv_tp_old adds what each path may
    // still see of them to the first Pmax - 1 blocks.  The first segment must reach beyond every old block
    // (n_blocks >= Pmax): the state it leaves behind is computed gate-free.  Shorter calls take the general kernel
    // (one wave per stream, blocks in sequence: 290 x slower on BASELINE config 4, which is why long calls do not).
    // (calls of 1 .. 3 blocks too: until round 5 they went through the sequential kernel -- one wave per stream, 93 us per
    // block on BASELINE config 4's shape, whatever the number of streams: profiles/r05_short_calls_before.jsonl)
    plan.gated = allow_fast && !gate_free && k.n_blocks >= Pmax;
    if (!allow_fast || !(gate_free || plan.gated)) {
        plan.kernel = OHS_CONV_KERNEL_SEQUENTIAL;
        return plan;
    }
    plan.kernel = OHS_CONV_KERNEL_BLOCK512_TP;
    // segment size: keep the MAC scratch around 128 MiB
    plan.SEG = std::max<long long>(8, std::min<long long>(16384 / (long long)c.S, 1024));
    if (plan.gated) plan.SEG = std::max<long long>(plan.SEG, Pmax);
    return plan;
}

// the (C, D) tables of k_conv_p1, kept current ahead of either one-partition plan
static int conv_p1_build_cd(ConvState &c, hipStream_t st)
{
    if (c.cd_valid) return OHS_OK;
    hipError_t e = launch_build_cd(c.d_H[0], c.d_H[1], c.d_H[2], c.d_H[3], c.d_cd, st);
    if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("build_cd: ") + hipGetErrorString(e));
    c.cd_valid = true;
    return OHS_OK;
}

// block 512 / FFT 1024, one partition (k_conv_p1); the events ride in its dispatch
static int conv_run_p1(ConvState &c, DeviceCtx *ctx, const ConvCall &k, const ConvPlan &plan, hipStream_t st,
                       hipEvent_t ev_start, hipEvent_t ev_stop, int &ranges)
{
    int rc = k.irs ? OHS_OK : conv_p1_build_cd(c, st);
    if (rc) return rc;
    if (k.irs && (!c.lazy_ok || !c.d_irs_cd)) return fail(OHS_ERR_HIP, "IR-scheduled launch without the lazy state or the set table");
    const Tuning &tn = tuning();
    const int K = plan.K;
    if ((size_t)K > c.chunk_tails_cap) {
        c.chunk_tails_cap = 0;
        rc = conv_realloc(c.d_chunk_tails, c.S * (size_t)K * 512 * sizeof(float2), st);
        if (rc) return rc;
        c.chunk_tails_cap = (size_t)K;
    }
    ConvP1Args a;
    a.in = k.in; a.out = k.out;
    a.in_stream_stride = k.in_ss; a.in_ch_stride = k.in_cs;
    a.out_stream_stride = k.out_ss; a.out_ch_stride = k.out_cs;
    a.n_blocks = k.n_blocks; a.n_streams = (int)c.S; a.chunks = K;
    a.CD = c.d_cd;
    for (int p = 0; p < 4; ++p) a.H[p] = c.d_H[p];
    a.tails = c.d_tails; a.tails_out = c.d_tails_alt; a.chunk_tails = c.d_chunk_tails;
    a.merged_in = c.tails_lazy ? c.d_merged : nullptr;
    a.merged_out = c.lazy_ok ? c.d_merged_alt : nullptr;
    a.last_in = c.lazy_ok ? c.d_last_in : nullptr;
    a.tw = ctx->d_tw; a.gain = k.gain; a.fp_mode = c.fp_mode;
    a.gain_tab = k.gain_tab; a.gain_seg = k.gain_seg; a.gain_off = k.gain_off; a.gain_stream = k.gain_stream;     // (k_conv_p1_gains looks the gain up itself)
    a.xcd_lo = plan.xcd_lo; a.xcd_n = plan.xcd_n;
    {   // boundary tails by the chunks' own waves where a stream's chunks share a workgroup (else: the pre-pass)
        const bool allowed = conv_p1_waves_per_cu() == 16 && (K == 2 || K == 4 || K == 8 || K == 16);
        a.own_tails = (allowed && (tn.p1_own_tails || k.irs)) ? 1 : 0;
    }
    a.stagger = tn.p1_stagger;
    a.prio_mode = tn.p1_prio;
    // Chunk lengths by the age rank of the wave that runs a chunk (p1_chunk_begin), equal lengths when chunks are
    // short.  In the plans that do not spread a stream's chunks over the ranks, ALL of a stream's chunks can sit on
    // heavy ranks: its shortest chunk is then n * wmin / (K * wmax) blocks, and that one must keep >= 2 blocks (a
    // chunk of zero blocks would make the boundary-tail code index block b0 - 1 = -1).
    const int *kw = tn.p1_weights;
    const int wmin = std::min(std::min(kw[0], kw[1]), std::min(kw[2], kw[3]));
    const int wmax = std::max(std::max(kw[0], kw[1]), std::max(kw[2], kw[3]));
    const bool weighted = (long long)k.n_blocks * wmin >= 2ll * K * wmax;
    for (int g = 0; g < 4; ++g) a.weights[g] = weighted ? kw[g] : 1;
    hipError_t e;
    if (k.irs) {
        ConvIrXfArgs i;
        i.cd = c.d_irs_cd; i.H = c.d_irs_H; i.tab = k.irs->tab;
        i.seg = k.irs->seg_blocks; i.off = k.irs->blk_off; i.stream = k.irs->stream_stride; i.cut = k.irs->cut ? 1 : 0;
        i.prev = k.irs->prev; i.prev_stream = k.irs->prev_stride;
        e = k.irs->xfade ? launch_conv_p1_irs_xf(a, i, st, ev_start, ev_stop) : launch_conv_p1_irs(a, i, st, ev_start, ev_stop);
    } else {
        e = launch_conv_p1(a, st, ev_start, ev_stop);
    }
    if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("conv_p1 launch: ") + hipGetErrorString(e));
    if (c.lazy_ok) {
        std::swap(c.d_merged, c.d_merged_alt);
        c.tails_lazy = true;
    } else {
        std::swap(c.d_tails, c.d_tails_alt);
    }
    ranges = K;
    return OHS_OK;
}

// hop 1536 / FFT 2048, one partition (k_conv_p1_os); the events ride in its dispatch
static int conv_run_os(ConvState &c, DeviceCtx *ctx, const ConvCall &k, int K, hipStream_t st, hipEvent_t ev_start,
                       hipEvent_t ev_stop, int &ranges)
{
    const int rc = conv_p1_build_cd(c, st);
    if (rc) return rc;
    if (!c.cd_os_valid) {
        hipError_t e = launch_os_tables(c.d_irt, ctx->d_tw, ctx->d_tw2048, c.d_cd_os, st);
        if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("os tables: ") + hipGetErrorString(e));
        c.cd_os_valid = true;
    }
    ConvOsArgs o;
    o.in = k.in; o.out = k.out;
    o.in_stream_stride = k.in_ss; o.in_ch_stride = k.in_cs; o.out_stream_stride = k.out_ss; o.out_ch_stride = k.out_cs;
    o.n_blocks = k.n_blocks; o.n_streams = (int)c.S; o.chunks = K;
    o.CD = c.d_cd_os; o.tw2048 = ctx->d_tw2048;
    o.tails = c.d_tails; o.merged_in = c.tails_lazy ? c.d_merged : nullptr;
    o.merged_out = c.d_merged_alt; o.last_in = c.d_last_in;
    o.tw = ctx->d_tw; o.gain = k.gain; o.fp_mode = c.fp_mode;
    hipError_t e = launch_conv_p1_os(o, st, ev_start, ev_stop);
    if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("conv_p1_os launch: ") + hipGetErrorString(e));
    std::swap(c.d_merged, c.d_merged_alt);
    c.tails_lazy = true;
    ranges = K;
    return OHS_OK;
}

// The call's frames join the input history of the block-2048 plan (what it starts from when a later call takes it): the
// time-parallel forward kernel appends them itself, the sequential kernel's calls get a launch for it (`append`) -- in front
// of anything that overwrites them in place.  Then the history's head moves past the call.
static int conv_xh_follow(ConvState &c, const ConvCall &k, bool append, hipStream_t st)
{
    if (!c.d_xhist) return OHS_OK;
    const long long frames = (long long)k.n_blocks * BS;
    if (append) {
        if (((k.in_ss | k.in_cs) & 3) != 0 || (reinterpret_cast<uintptr_t>(k.in) & 15) != 0) {
            c.xh_valid = 0;     // (buffers the 16-byte copy cannot read: the history no longer follows the stream)
            return OHS_OK;
        }
        hipError_t e = launch_conv_lb_xhist_append(k.in, k.in_ss, k.in_cs, c.d_xhist, c.xh_len, c.xh_head, frames, (int)c.S, st);
        if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("input history update: ") + hipGetErrorString(e));
    }
    c.xh_head = (c.xh_head + std::min(frames, c.xh_len)) % (2 * c.xh_len);
    c.xh_valid = std::min(c.xh_len, c.xh_valid + frames);
    return OHS_OK;
}

// block 512, several partitions, one wave per stream and the blocks in sequence (k_conv_general)
static int conv_run_sequential(ConvState &c, DeviceCtx *ctx, const ConvCall &k, hipStream_t st, int &ranges)
{
    int rc = conv_materialise_state(c, ctx, st);        // (this kernel reads and writes the per-path overlaps)
    if (rc) return rc;
    c.lb_valid = 0;         // (the block-2048 ring does not see the blocks of this call)
    rc = conv_xh_follow(c, k, true, st);
    if (rc) return rc;
    ConvGeneralArgs a;
    a.in = k.in; a.out = k.out;
    a.in_stream_stride = k.in_ss; a.in_ch_stride = k.in_cs;
    a.out_stream_stride = k.out_ss; a.out_ch_stride = k.out_cs;
    a.n_blocks = k.n_blocks;
    for (int p = 0; p < 4; ++p) { a.H[p] = c.d_H[p]; a.P[p] = c.P[p]; a.since[p] = c.since[p]; }
    a.hist = c.d_hist; a.cap = c.cap; a.cnt = c.cnt;
    a.tails = c.d_tails; a.tails_out = c.d_tails;
    a.skip_store = 0; a.zero_tails_in = 0;
    a.tw = ctx->d_tw; a.gain = k.gain; a.fp_mode = c.fp_mode;
    hipError_t e = launch_conv_general(a, (int)c.S, st);
    if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("conv launch: ") + hipGetErrorString(e));
    ranges = 1;
    return OHS_OK;
}

// block 512, several partitions, time-parallel: k_conv_tp_forward / _mac / _inverse per segment of plan.SEG blocks; gated
// (after a per-path set_ir) behind a zeroed gap in the ring, with k_conv_tp_old in the first segment
static int conv_run_tp(ConvState &c, DeviceCtx *ctx, const ConvCall &k, const ConvPlan &plan, hipStream_t st, int &ranges)
{
    int rc = conv_materialise_state(c, ctx, st);        // (these kernels read and write the per-path overlaps)
    if (rc) return rc;
    c.lb_valid = 0;         // (the block-2048 ring does not see the blocks of this call)
    const int Pmax = conv_max_p(c);
    const long long seg_max = std::min<long long>(plan.SEG, k.n_blocks);
    const int Ppad = Ppad_for_ring(Pmax);
    // (gated: old blocks + the zeroed gap + the segment live in the ring together)
    rc = conv_grow_ring(c, (int)(seg_max + (plan.gated ? 2 : 1) * (Ppad - 1) + (plan.gated ? Pmax : 0)), st);
    if (rc) return rc;
    const unsigned long long cnt_old = c.cnt;
    if (plan.gated) {
        // the zeroed gap: ring slots cnt .. cnt + Ppad - 2 of every stream (two strided memsets when it wraps)
        const unsigned long long gap = (unsigned long long)(Ppad - 1), cap = (unsigned long long)c.cap;
        const unsigned long long s0 = c.cnt & (cap - 1), n0 = std::min(gap, cap - s0);
        const size_t pitch = (size_t)c.cap * NF * sizeof(float2);
        HIP_TRY(hipMemset2DAsync(c.d_hist + s0 * NF, pitch, 0, (size_t)n0 * NF * sizeof(float2), c.S, st));
        if (n0 < gap)
            HIP_TRY(hipMemset2DAsync(c.d_hist, pitch, 0, (size_t)(gap - n0) * NF * sizeof(float2), c.S, st));
        c.cnt += gap;
    }
    if (!c.d_cdm || c.cdm_ppad != Ppad) {       // (a set_ir that keeps Ppad re-uses the buffer: no wait, no malloc)
        c.cdm_valid = false;
        rc = conv_realloc(c.d_cdm, (size_t)Ppad * 2 * NF * sizeof(float2), st);
        if (rc) return rc;
        c.cdm_ppad = Ppad;
    }
    if (!c.cdm_valid) {
        hipError_t e = launch_build_cd_multi(c.d_H[0], c.d_H[1], c.d_H[2], c.d_H[3], c.P[0], c.P[1],
                                             c.P[2], c.P[3], Ppad, c.d_cdm, st);
        if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("build_cd_multi: ") + hipGetErrorString(e));
        c.cdm_ppad = Ppad; c.cdm_valid = true;
    }
    if ((size_t)seg_max > c.w_blocks) {
        c.w_blocks = 0;
        rc = conv_realloc(c.d_W, c.S * (size_t)seg_max * NF * sizeof(float2), st);
        if (rc) return rc;
        c.w_blocks = (size_t)seg_max;
    }
    if (!c.d_W1) HIP_TRY(hipMalloc(&c.d_W1, c.S * (size_t)NF * sizeof(float2)));
    const long long call_frames = (long long)k.n_blocks * BS;
    const long long xh_cnt = c.d_xhist ? std::min(call_frames, c.xh_len) : 0;
    long long done = 0;
    while (done < k.n_blocks) {
        const int seg = (int)std::min<long long>(plan.SEG, k.n_blocks - done);
        ConvTpArgs a;
        a.in = k.in + done * BS; a.out = k.out + done * BS;
        a.in_stream_stride = k.in_ss; a.in_ch_stride = k.in_cs;
        a.out_stream_stride = k.out_ss; a.out_ch_stride = k.out_cs;
        a.n_streams = (int)c.S; a.seg_blocks = seg; a.n_mac = seg; a.Ppad = Ppad; a.Pmax = Pmax;
        a.CD = c.d_cdm; a.hist = c.d_hist; a.cap = c.cap; a.cnt = c.cnt + (unsigned long long)done;
        a.W = c.d_W; a.W1 = c.d_W1; a.tails = c.d_tails; a.tails_out = c.d_tails_alt;
        a.pairs = ctx->d_pairs; a.n_pairs = ctx->n_pairs;
        a.tw = ctx->d_tw; a.gain = k.gain; a.fp_mode = c.fp_mode;
        // (frame i of the segment is frame done * 512 + i of the call; the call's last xh_cnt frames are appended)
        a.xh_ring = c.d_xhist; a.xh_len = c.xh_len; a.xh_head = c.xh_head;
        a.xh_frame0 = done * BS - (call_frames - xh_cnt);
        hipError_t e = launch_conv_tp_forward(a, st);
        if (e == hipSuccess) e = launch_conv_tp_mac(a, st);
        if (e == hipSuccess && plan.gated && done == 0 && Pmax > 1) {
            ConvTpOldArgs o;
            o.n_streams = (int)c.S; o.n_old = Pmax - 1; o.Pmax = Pmax;
            for (int p = 0; p < 4; ++p) { o.H[p] = c.d_H[p]; o.P[p] = c.P[p]; o.since[p] = c.since[p]; }
            o.hist = c.d_hist; o.cap = c.cap; o.cnt_old = cnt_old;
            o.W = c.d_W; o.n_mac = seg; o.fp_mode = c.fp_mode;
            e = launch_conv_tp_old(o, st);
        }
        if (e == hipSuccess) e = launch_conv_tp_inverse(a, st);   // block 0 reads the OLD state; new state -> the other slab
        if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("conv_tp: ") + hipGetErrorString(e));
        std::swap(c.d_tails, c.d_tails_alt);
        done += seg;
        ranges = seg;
    }
    return conv_xh_follow(c, k, false, st);
}

int conv_launch(ConvState &c, DeviceCtx *ctx, const float *in, long long in_ss, long long in_cs,
                float *out, long long out_ss, long long out_cs, int n_blocks, float gain, hipStream_t st,
                bool allow_fast, hipEvent_t ev_start, hipEvent_t ev_stop, const ConvGains *gains, const ConvIrs *irs)
{
    // (ev_start / ev_stop: recorded at the start / completion of the call's launches)
    if (n_blocks <= 0) {                    // nothing to do (the pre-pass would index block -1)
        if (ev_start) HIP_TRY(hipEventRecord(ev_start, st));
        if (ev_stop) HIP_TRY(hipEventRecord(ev_stop, st));
        return OHS_OK;
    }
    // A gain per segment (ohs_batch_process_scheduled): k_conv_p1 looks it up at its store; every other family runs with gain 1
    // and is followed by k_scale_segments (x * 1.0f is exact: the same bits, except where the pending-tails add below folds the
    // gain in -- there (a + b) * g instead of a * g + b * g).  The plan is chosen exactly as for the plain call.
    const bool seg_gains = gains != nullptr && gains->tab != nullptr;
    ConvCall k{in, in_ss, in_cs, out, out_ss, out_cs, n_blocks, seg_gains ? 1.0f : gain};
    if (irs && irs->tab) {
        if (conv_max_p(c) != 1 || !allow_fast || c.pt_active || seg_gains)
            return fail(OHS_ERR_INVALID_ARG, "a schedule of impulse responses needs one-partition responses, no pending tails and no gain schedule");
        k.irs = irs;
    }
    const ConvPlan plan = conv_choose_plan(c, ctx, k, allow_fast);
    int ranges = 0, rc;
    if (plan.kernel == OHS_CONV_KERNEL_BLOCK512_P1) {
        if (seg_gains && !c.pt_active) { k.gain_tab = gains->tab; k.gain_seg = gains->seg_blocks; k.gain_off = gains->blk_off; k.gain_stream = gains->stream_stride; }
        rc = conv_run_p1(c, ctx, k, plan, st, ev_start, ev_stop, ranges);
    } else if (plan.kernel == OHS_CONV_KERNEL_HOP1536_P1) {
        rc = conv_run_os(c, ctx, k, plan.K, st, ev_start, ev_stop, ranges);
    } else {
        struct EvScope {    // the plans that do not carry the events in a dispatch: recorded around their launches
            hipStream_t st; hipEvent_t stop;
            ~EvScope() { if (stop) hipEventRecord(stop, st); }
        };
        if (ev_start) HIP_TRY(hipEventRecord(ev_start, st));
        const EvScope ev_scope{st, ev_stop};
        switch (plan.kernel) {
        case OHS_CONV_KERNEL_BLOCK2048: rc = conv_lb_launch(c, ctx, k, st, ranges); break;
        case OHS_CONV_KERNEL_BLOCK8192: rc = conv_xb_launch(c, ctx, k, plan.P2x, st, ranges); break;
        case OHS_CONV_KERNEL_BLOCK512_TP: rc = conv_run_tp(c, ctx, k, plan, st, ranges); break;
        default: rc = conv_run_sequential(c, ctx, k, st, ranges); break;
        }
    }
    if (rc) return rc;
    // the epilogue of every plan
    c.cnt += (unsigned long long)n_blocks;
    for (int p = 0; p < 4; ++p) c.since[p] += n_blocks;
    c.last_kernel = plan.kernel; c.last_ranges = ranges;
    c.kernel_calls[plan.kernel]++;
    c.last_ir_scheduled = k.irs != nullptr;
    c.last_ir_crossfaded = k.irs != nullptr && k.irs->xfade;
    c.tails_both = false;       // (d_tails belongs to the state in front of this launch)
    if (k.irs && (k.irs->per_stream_state || k.irs->faded_end) && k.irs->blk_off + n_blocks == k.irs->call_blocks) {
        // the call's last block has left the lazy state; the per-path overlaps under every stream's own last set, now, while the rows
        // are at hand (conv_materialise_state would take the handle's spectra) -- and, where that block faded, as the sum of both
        // halves of the fade (the last input through ONE set is not what it left)
        ConvP1Args a;
        conv_state_args(c, ctx, a);
        ConvIrXfArgs i;
        i.cd = c.d_irs_cd; i.H = c.d_irs_H; i.tab = k.irs->tab;
        i.seg = k.irs->seg_blocks; i.off = k.irs->call_blocks - 1; i.stream = k.irs->stream_stride; i.cut = 0;
        i.prev = k.irs->prev; i.prev_stream = k.irs->prev_stride;
        hipError_t e = k.irs->xfade ? launch_conv_p1_state_irs_xf(a, i, st) : launch_conv_p1_state_irs(a, i, st);
        if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("conv_p1_state_irs launch: ") + hipGetErrorString(e));
        c.tails_both = true;
    }
    if (c.pt_active) {
        // what the frames in front of a per-path set_ir still owe these frames (conv_lb_tail_route)
        const long long n = (long long)n_blocks * BS;
        // (with a gain table in k_conv_p1: tail * gain[segment] is not what this launch computes -- it adds with gain 1 in front of
        // the scale pass below, so such a call takes the scale pass for the tails' sake)
        hipError_t e = launch_conv_lb_tails_add(out, out_ss, out_cs, n, c.d_ptail, c.pt_len, c.pt_pos, k.gain, (int)c.S, st, c.fp_mode);
        if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("pending tails: ") + hipGetErrorString(e));
        c.pt_pos += n;
        if (c.pt_pos >= c.pt_len) c.pt_active = false;
    }
    if (seg_gains && !k.gain_tab) {
        hipError_t e = launch_scale_segments(out, out_ss, out_cs, n_blocks, (int)c.S, gains->tab, gains->seg_blocks, gains->blk_off, st,
                                             c.fp_mode, gains->stream_stride);
        if (e != hipSuccess) return fail(OHS_ERR_HIP, std::string("segment gains: ") + hipGetErrorString(e));
    }
    return OHS_OK;
}

}  // namespace ohs_api
