// api_internal.h -- what the translation units of the C-ABI implementation share: error reporting, the per-device
// context, the convolution / EQ state of a handle with the functions that drive it, the handle structs themselves.
// Internal to open_headstage_amd/csrc; nothing here crosses the C ABI (include/ohs_hip.h).
//   api_core.hip    error state, device context, library-wide entry points (version, device count, ohs_rt_configure, debug)
//   api_conv.hip    ConvState: set_ir, the launch plans of the convolution (conv_launch)
//   api_eq.hip      EqState + ohs_eq_* + ohs_biquad_*
//   api_engine.hip  ohs_engine_* (FIFO adapter, launch per call, resident real-time kernel and its mailbox), ohs_chain_process
//   api_batch.hip   ohs_batch_* (EQ || convolution over time chunks, host pipeline, profiling)
#pragma once
#include "../../include/ohs_hip.h"
#include "kernels.h"
#include "wave_fft.hpp"
#include "host_internal.h"
#include "tuning.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

namespace ohs_api {
using namespace ohs;

constexpr int BS = OHS_BLOCK_SIZE;
constexpr int NF = OHS_FFT_SIZE;

extern thread_local std::string g_err;
#ifdef OHS_EXPERIMENTS
// experiments build: the k-th chunk launch sequence of ohs_batch_process from now fails as if HIP had refused it
// (ohs_debug_inject_batch_failure); the product build has no such path
extern std::atomic<int> g_inject_batch_failure;
#endif

int fail(int status, const std::string &msg);

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            return fail(OHS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));      \
    } while (0)

// ---- per-device context: the master twiddle table ------------------------------
struct DeviceCtx {
    int device = -1;
    float2 *d_tw = nullptr;
    float2 *d_tw2048 = nullptr; // k_conv_p1_os: w2048^bin in the paired layout
    float2 *d_tw4096 = nullptr; // k_conv_lb_*: w4096^(n1 c), [3][1024]
    float2 *d_tw16384 = nullptr;// k_conv_xb: w16384^(n1 c), [15][1024]
    int *d_pairs = nullptr;     // k_conv_tp_mac: leaders of the spectrum position pairs {b, mirror(b)}
    int n_pairs = 0;
    int num_cus = 256;
};
int get_ctx(int device, DeviceCtx **out);

// the MAC's register windows read up to Ppad - 1 blocks back (C/D are zero beyond the real partition count, and those
// partitions are skipped, never multiplied: ConvTpArgs::Pmax)
inline int Ppad_for_ring(int Pmax) { return (Pmax + 15) / 16 * 16; }

inline int next_pow2(int v)
{
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// ---- resident real-time kernels vs. device-wide waits ------------------------------------------------------
// hipFree, hipDeviceSynchronize and hipHostFree wait for EVERY kernel on the device -- a resident real-time kernel
// (k_engine_resident) of some other engine included, which only leaves when its owner stops it or after ~2 s without
// a call.  Library code that is about to make such a wait opens a DeviceWideSection: it asks every resident kernel of
// the device to leave (the `stop` word of its mailbox; the kernel is gone a microsecond later, and its owner restarts
// it on its next call exactly as after an idle exit) and keeps new ones from starting until the section ends (rt_start
// answers OHS_RT_NO_SLOT meanwhile: that call is served launch per call, like an engine beyond the device's cap).
// Only the mailbox word of a foreign engine is touched, under the registry's mutex, which an engine's destruction
// takes before its mailbox is freed.
constexpr int kMaxDevices = 64;
struct RtRegistry {
    std::mutex mu;
    std::vector<ohs_engine *> running;     // engines whose resident kernel has been launched and not yet reaped
    int hold = 0;                           // open DeviceWideSections
};
extern RtRegistry g_rt_reg[kMaxDevices];
void rt_request_stop_locked(ohs_engine *e);      // (api_engine.hip, with the mailbox protocol)
struct DeviceWideSection {
    int dev = 0;
    DeviceWideSection()
    {
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
        RtRegistry &r = g_rt_reg[dev % kMaxDevices];
        std::lock_guard<std::mutex> lk(r.mu);
        ++r.hold;
        for (ohs_engine *e : r.running) rt_request_stop_locked(e);
    }
    ~DeviceWideSection()
    {
        RtRegistry &r = g_rt_reg[dev % kMaxDevices];
        std::lock_guard<std::mutex> lk(r.mu);
        --r.hold;
    }
    DeviceWideSection(const DeviceWideSection &) = delete;
    DeviceWideSection &operator=(const DeviceWideSection &) = delete;
};

// ---- convolution state shared by the engine (1 stream) and batch (S streams); api_conv.hip ----
struct ConvState {
    size_t S = 1;
    float2 *d_H[4] = {nullptr, nullptr, nullptr, nullptr};
    int P[4] = {1, 1, 1, 1};
    long long since[4] = {0, 0, 0, 0};
    float2 *d_hist = nullptr;       // [S][cap][1024]
    int cap = 1;
    unsigned long long cnt = 0;
    float2 *d_tails = nullptr;      // [S][2][8][64]
    // P = 1 fast path
    float2 *d_tails_alt = nullptr;  // second state slab (k_conv_p1 writes its new tails here)
    float2 *d_cd = nullptr;         // [2][1024] combined spectra C, D
    bool cd_valid = false;
    float2 *d_chunk_tails = nullptr;
    size_t chunk_tails_cap = 0;     // in chunks per stream
    // time-parallel long-IR path
    float2 *d_cdm = nullptr;        // [Ppad][2][1024] combined spectra per partition
    int cdm_ppad = 0;
    bool cdm_valid = false;
    float2 *d_W = nullptr;          // [S][w_blocks][1024] MAC output scratch
    size_t w_blocks = 0;
    float2 *d_W1 = nullptr;         // [S][1024]
    int fp_mode = 0;                // denormal handling of every launch on this state (kernels.h: ohs_set_fp_mode)
    int xcd_lo = 0, xcd_n = 8;      // XCDs the P = 1 kernels may use (kernels.h: xcd_grid); set per call by the batch
    // Lazy state of the P = 1 fast path (batch objects; kernels.h: ConvP1Args::merged_out).  While tails_lazy, d_tails is
    // stale and the state is {d_merged, d_last_in}; conv_materialise_state turns it back into the per-path overlaps.
    bool lazy_ok = false, tails_lazy = false;
    float2 *d_merged = nullptr, *d_merged_alt = nullptr;    // [S][8][64]
    float *d_last_in = nullptr;                             // [S][2][512]
    // overlap-save plan of the P = 1 path (conv_os_kernels.hip; batch objects): the impulse responses in the time domain
    // (512 floats per path, zero-padded; valid while that path has one partition) and the (C, D) tables built from them
    float *d_irt = nullptr;         // [4][512]
    float4 *d_cd_os = nullptr;      // [2][1024]
    bool cd_os_valid = false;
    int conv_plan = 0;              // ohs_batch_set_conv_plan: 0 = the library's choice, 1 = block 512 / FFT 1024, 2 = the large-transform
                                    // plans (one partition: hop 1536 / FFT 2048; longer responses: block 2048 / FFT 4096)
    // Block-2048 plan for long impulse responses (conv_lb_kernels.hip; batch objects with a response of lb_min_p() partitions
    // or more).  It is overlap-save on the INPUT: the state it needs and leaves is the last xh_len input frames of every
    // stream (d_xhist; every P > 1 launch of such an object keeps it current), not spectra and overlaps.  While lb_lazy,
    // d_hist / d_tails are stale; conv_materialise_state rebuilds them from d_xhist when another plan needs them.
    float *d_irl = nullptr;         // [4][irl_len] the impulse responses in the time domain, zero-padded
    long long irl_len = 0;
    float *d_xhist = nullptr;       // [S][2][2 xh_len], a ring of twice its reach: the frame k <= xh_len frames in front of the next
                                    // one at (xh_head - k) mod 2 xh_len (the forward kernels append into the half nobody reads)
    float *d_xhist_alt = nullptr;   // [S][2][xh_len] scratch: the history in time order, when the block-512 state is rebuilt from it
    long long xh_len = 0;           // the reach = P2pad * 2048
    long long xh_head = 0;          // where the next frame goes (a multiple of 512, < 2 xh_len)
    long long xh_valid = 0;         // trailing frames of d_xhist that are what every path may see of the past (zeros after a reset of all paths count)
    bool lb_lazy = false;
    float4 *d_lb_ring = nullptr;    // [S][lb_ring_cap][2048] window spectra, pair layout
    int lb_ring_cap = 0;
    // The windows sit on the stream's ABSOLUTE grid (block B = frames [2048 B, 2048 B + 2048) counted from the last reset):
    // window B lives in ring slot (B + 4 lb_ring_cap) % lb_ring_cap.  A call may start and end anywhere on the 512 grid: the
    // block it starts in is recomputed (its earlier frames come from the input history), the block it ends in is computed
    // with zeros for the frames to come and recomputed by the next call -- only windows of COMPLETE blocks stay valid.
    long long lb_end = 0;           // windows lb_end - lb_valid .. lb_end - 1 (complete blocks) are in the ring
    long long lb_valid = 0;
    float4 *d_lb_cd = nullptr, *d_lb_ab = nullptr;          // [P2pad][2][2048] tables; [2][P2pad][2048] scratch for building them
    int lb_p2pad = 0;               // what d_lb_cd / d_lb_ab are allocated for
    bool lb_cd_valid = false;
    // Pending tails (conv_lb_tail_route): a per-path set_ir on an object that keeps the input history is carried out as "every
    // path forgets its past" + what the frames in front of the reset still owe the output through the SURVIVING paths,
    // computed once ([S][4 paths][pt_len], a row per path so that a later reset of that path can drop it) and added to the
    // output of the calls that follow, whatever plan serves them.  No kernel of such an object ever needs a per-path gate.
    float *d_ptail = nullptr, *d_ptail_alt = nullptr;
    long long pt_len = 0, pt_pos = 0;
    bool pt_active = false;
    float4 *d_lb_cd_alt = nullptr;  // tables of one speaker pair alone (the tails' two runs)
    int lb_cd_alt_p2pad = 0;
    // block 8192 / FFT 16384 (conv_xb_kernels.hip): tables of the response's one or two 8192-tap partitions; valid with lb_cd_valid's
    // generation (every place that invalidates the block-2048 tables bumps lb_tables_gen)
    float4 *d_xb_cd = nullptr, *d_xb_ab = nullptr;
    int xb_p2 = 0;
    unsigned long long lb_tables_gen = 1, xb_cd_gen = 0;
    // Engines (one stream) with a response of more than one partition: the next call's sums over the partitions behind it
    // (kernels.h: ConvGeneralArgs::pre), computed by the kernel that served the previous call.  They belong to the state
    // with block counter pre_cnt; anything else that touches the state (set_ir, reset, a ring that moved, another kernel
    // that processes blocks) leaves pre_cnt != cnt or sets it to ~0 here.
    float2 *d_pre = nullptr;        // [8][2][1024]
    unsigned long long pre_cnt = ~0ull;
    int pre_n = 0;
    // what served the last convolution launch (ohs_batch_last_conv_plan): OHS_CONV_KERNEL_*, and its ranges per stream
    int last_kernel = 0, last_ranges = 0;
    unsigned long long kernel_calls[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // conv_launch calls served per family (ohs_batch_conv_plan_counts)
    // The set table of the IR-scheduled call (ohs_batch_set_schedule_irs): irs_n sets of four one-partition responses, as the (C, D)
    // tables k_conv_p1_irs reads, as the four path spectra per set (the state kernel; what a shared-row call adopts into d_H) and in
    // the time domain, zero-padded to 512 (what it adopts into d_irt / d_irl)
    size_t irs_n = 0;
    float4 *d_irs_cd = nullptr;     // [irs_n][1024]
    float2 *d_irs_H = nullptr;      // [irs_n][4][1024]
    float *d_irs_t = nullptr;       // [irs_n][4][512]
    // tails_lazy && tails_both: d_tails holds the per-path overlaps too (computed behind an IR-scheduled call with a row per stream,
    // where d_H could not rebuild them); the next launch clears it
    bool tails_both = false;
    bool last_ir_scheduled = false; // the last conv_launch looked the set up per block (ohs_batch_last_conv_ir_scheduled)
    bool last_ir_crossfaded = false;    // ... with the crossfading kernel k_conv_p1_irs_xf (the query then reports 2)
    // The speaker layout of ohs_batch_process_layout (ohs_batch_set_layout_irs): lay_K channels of two responses each (at most 512 taps),
    // as the (C, D) table of every PAIR of channels that k_conv_p1_layout reads, and the layout's own merged overlap -- two slabs, the
    // launch reads d_lay_ov and writes d_lay_ov_alt, then they swap.  Independent of everything above: the stereo calls never touch it.
    size_t lay_K = 0, lay_len = 0;
    float4 *d_lay_cd = nullptr;     // [ceil(lay_K / 2)][1024]
    float2 *d_lay_ov = nullptr, *d_lay_ov_alt = nullptr;    // [S][8][64]
    int last_lay_pairs = 0, last_lay_ranges = 0;    // the most recent layout launch (ohs_batch_last_layout_launch)
    // The table of layouts of ohs_batch_process_layout_scheduled (ohs_batch_set_layout_schedule_irs): lays_n sets of lays_K channels,
    // the (C, D) table of every (set, pair) that k_conv_p1_layout_irs reads.  Independent of the single layout above -- either may
    // exist without the other --, but both calls continue ONE overlap: d_lay_ov / d_lay_ov_alt live while either exists.
    size_t lays_n = 0, lays_K = 0, lays_len = 0;
    float4 *d_lays_cd = nullptr;    // [lays_n][ceil(lays_K / 2)][1024]
    bool last_lay_scheduled = false;    // k_conv_p1_layout_irs served the most recent layout launch (ohs_batch_last_layout_scheduled)
    // The direction table of the object scenes (ohs_scene_set_direction_irs; no entry of ohs_hip.h reaches it): obj_n directions of two
    // responses each, as the half-sums k_conv_p1_objects combines per pass, and one all-zero row behind them.  The scene call continues
    // the layout overlap: d_lay_ov / d_lay_ov_alt live while any of the three tables exists.
    size_t obj_n = 0, obj_len = 0;
    float2 *d_obj_ah = nullptr;     // [obj_n + 1][1024]
    int last_obj_pairs = 0, last_obj_ranges = 0;    // the most recent scene launch (ohs_scene_last_launch)
    unsigned long long last_obj_fading = 0;         // ... and its passes through old directions, summed over the streams
    unsigned long long last_obj_blended = 0;        // ... and its passes that load four rows (0 behind a plain scene call)
    unsigned long long last_obj_blended3 = 0;       // ... and its passes that load six rows (0 behind a one- or two-direction call)
    // ohs_*_set_speakers: what it last loaded into each path (a set_ir from anywhere else forgets it), so that a
    // change of the speaker angles re-loads only the paths whose impulse response really changed
    std::vector<float> spk_ir[4];
    bool spk_set[4] = {false, false, false, false};
};

void conv_free(ConvState &c);
inline int conv_max_p(const ConvState &c) { return std::max(std::max(c.P[0], c.P[1]), std::max(c.P[2], c.P[3])); }
inline bool conv_since_equal(const ConvState &c) { return c.since[0] == c.since[1] && c.since[1] == c.since[2] && c.since[2] == c.since[3]; }
inline bool conv_since_zero(const ConvState &c) { return conv_since_equal(c) && c.since[0] == 0; }     // every path reset since the last block
// the input history holds all of every path's own response's reach of the past that the path may see: each path older than
// its response (and the history that deep), or all reset together with the others (the history was zeroed then)
inline bool conv_history_covers_paths(const ConvState &c)
{
    bool deep = true;
    for (int p = 0; p < 4; ++p) deep = deep && c.since[p] >= c.P[p] && c.xh_valid >= (long long)c.P[p] * OHS_BLOCK_SIZE;
    return deep || (conv_since_equal(c) && c.xh_valid >= c.xh_len);
}
// the `pre` fields of an engine kernel's arguments for a call that completes k blocks (<= 8)
inline void conv_pre_args(const ConvState &c, ConvGeneralArgs &a, int k)
{
    const bool on = c.d_pre != nullptr && conv_max_p(c) > 1;
    a.pre = on ? c.d_pre : nullptr;
    a.pre_n = (on && c.pre_cnt == c.cnt) ? c.pre_n : 0;
    a.pre_next = on ? k : 0;
}
// ... and the host's mirror of what the kernel left behind (after c.cnt has been advanced by k)
inline void conv_pre_served(ConvState &c, int k)
{
    if (k <= 0) return;             // no block completed: the sums found stay what they are
    const bool on = c.d_pre != nullptr && conv_max_p(c) > 1;
    c.pre_cnt = on ? c.cnt : ~0ull;
    c.pre_n = on ? k : 0;
}
int conv_init(ConvState &c, size_t S, hipStream_t st);
int conv_enable_lazy_state(ConvState &c);
int conv_materialise_state(ConvState &c, DeviceCtx *ctx, hipStream_t st);
int conv_grow_ring(ConvState &c, int need, hipStream_t st);
int conv_set_ir(ConvState &c, DeviceCtx *ctx, int path, const float *ir, size_t len, hipStream_t st,
                bool ir_on_device = false);
bool conv_plan_auto_is_os(size_t S, long long n_blocks, bool in_place);
inline int lb_min_p() { return tuning().lb_min_p; }     // 512-tap partitions from which the block-2048 plan is considered (2: taps > 512)
bool conv_plan_auto_is_lb(size_t S, long long n_blocks, int Pmax);
bool conv_plan_auto_is_xb(size_t S, long long n_blocks, int Pmax);      // ... and among those, the block-8192 kernel (out-of-place calls)
int conv_os_chunks(const DeviceCtx *ctx, size_t S, long long n_blocks, bool in_place);
// time chunks per stream of the one-partition kernel's launch plan (also what ohs_batch_kernel_bytes prices)
long long conv_p1_chunks(const DeviceCtx *ctx, size_t S, long long n_blocks, long long target_override, int xcd_n = 8,
                         int waves_per_cu = 0);      // (0: k_conv_p1's; k_conv_p1_layout passes its own)
// a gain per segment of seg_blocks blocks (device memory): block t of the launch, block blk_off + t of the call, leaves with
// tab[(blk_off + t) / seg_blocks].  NULL (or tab == NULL): the scalar `gain`.
// stream_stride: stream s reads its row at tab + s * stream_stride (0: one row for all streams).
struct ConvGains {
    const float *tab = nullptr;
    int seg_blocks = 1, blk_off = 0;
    int stream_stride = 0;
};
// a set of impulse responses per segment and stream (device rows of indices into the handle's set table): block t of the launch,
// block blk_off + t of a call of call_blocks blocks, is convolved with set tab[s * stream_stride + (blk_off + t) / seg_blocks].
// cut: OHS_IR_SWITCH_CUT.  per_stream_state: behind the call's last block the per-path overlaps are computed from every stream's
// own last set (rows per stream: d_H cannot rebuild them later).  Needs every path at one partition, the lazy state, no pending tails
// (the batch entry point checks); always served by the block-512 family.
// xfade: ohs_batch_process_ir_crossfaded -- k_conv_p1_irs_xf serves the launches; prev (device memory, or nullptr): the set in front
// of the call's first block, stream s reads prev[s * prev_stride].  faded_end: the call's last block fades in at least one stream,
// so the per-path overlaps are computed behind it whatever the rows (neither d_H nor one set per stream could rebuild them).
struct ConvIrs {
    const unsigned *tab = nullptr;
    int seg_blocks = 1, blk_off = 0, stream_stride = 0, call_blocks = 0;
    bool cut = false, per_stream_state = false;
    bool xfade = false, faded_end = false;
    const unsigned *prev = nullptr;
    int prev_stride = 0;
};
int conv_launch(ConvState &c, DeviceCtx *ctx, const float *in, long long in_ss, long long in_cs,
                float *out, long long out_ss, long long out_cs, int n_blocks, float gain, hipStream_t st,
                bool allow_fast = true, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr,
                const ConvGains *gains = nullptr, const ConvIrs *irs = nullptr);
// the set table (host array irs[n_sets][4][len], 1 <= len <= 512; n_sets == 0 frees it); the caller has drained the device
int conv_set_schedule_irs(ConvState &c, DeviceCtx *ctx, size_t n_sets, const float *irs, size_t len, hipStream_t st);
// the speaker layout (host array irs[n_channels][2][len], 1 <= len <= 512; n_channels == 0 frees it) and its zeroed overlap; the
// caller has drained the device
int conv_set_layout_irs(ConvState &c, DeviceCtx *ctx, size_t n_channels, const float *irs, size_t len, hipStream_t st);
// n_blocks of every stream's lay_K channels -> two ears, times gain; out of place (the caller checks), asynchronous on st
int conv_launch_layout(ConvState &c, DeviceCtx *ctx, const float *in, long long in_ss, long long in_cs,
                       float *out, long long out_ss, long long out_cs, int n_blocks, float gain, hipStream_t st);
// the table of layouts (host array irs[n_sets][n_channels][2][len], 1 <= len <= 512; n_sets == 0 frees it); zeroes the layout overlap;
// the caller has drained the device
int conv_set_layout_schedule_irs(ConvState &c, DeviceCtx *ctx, size_t n_sets, size_t n_channels, const float *irs, size_t len,
                                 hipStream_t st);
// rows of set indices into that table (device memory; validated by the caller): block t uses set tab[s * stream_stride + t / seg_blocks];
// fade: the crossfade over the first block of a segment whose set differs from the one in front (prev: in front of the call's
// first block, stream s reads prev[s * prev_stride]; nullptr: no boundary there)
struct ConvLayoutRows {
    const unsigned *tab = nullptr;
    int seg_blocks = 1, stream_stride = 0;
    const unsigned *prev = nullptr;
    int prev_stride = 0;
    bool fade = false;
};
// n_blocks of every stream's lays_K channels -> two ears, times gain.  rows == nullptr: set `one_set` throughout, served by
// k_conv_p1_layout on that set's slice of the table; else one launch of k_conv_p1_layout_irs.  Out of place, asynchronous on st
int conv_launch_layout_scheduled(ConvState &c, DeviceCtx *ctx, const float *in, long long in_ss, long long in_cs,
                                 float *out, long long out_ss, long long out_cs, int n_blocks, float gain, hipStream_t st,
                                 const ConvLayoutRows *rows, size_t one_set);
// the direction table of the object scenes (host array irs[n_dirs][2][len], 1 <= len <= 512; n_dirs == 0 frees it); zeroes the layout
// overlap; the caller has drained the device
int conv_set_object_dirs(ConvState &c, DeviceCtx *ctx, size_t n_dirs, const float *irs, size_t len, hipStream_t st);
// rows of direction indices and gains per object (device memory; validated by the caller), as ConvObjectsArgs reads them
struct ConvObjectRows {
    const unsigned *idx = nullptr, *gain = nullptr, *prev_idx = nullptr, *prev_gain = nullptr;
    int seg_blocks = 1, stream_stride = 0, prev_stride = 0;
    bool fade = false;
};
// n_blocks of every stream's n_objects channels -> two ears, times gain: one launch of k_conv_p1_objects.  Out of place, asynchronous on st
int conv_launch_objects(ConvState &c, DeviceCtx *ctx, const float *in, long long in_ss, long long in_cs, float *out, long long out_ss,
                        long long out_cs, int n_blocks, float gain, hipStream_t st, int n_objects, const ConvObjectRows &rows);
// the blended scene calls' rows (device memory; validated by the caller), as ConvObjectsBlendArgs reads them: 2 n_dirs planes -- the
// n_dirs directions, the n_dirs - 1 weights, the gain (if has_gain) -- `plane` entries apart, and in front of the call as many planes
// of [row][n_objects], `prev_plane` apart (all staged whenever fade is set)
struct ConvObjectBlendRows {
    const unsigned *rows = nullptr, *prev = nullptr;
    int plane = 0, prev_plane = 0, seg_blocks = 1, stream_stride = 0, prev_stride = 0;
    bool has_gain = false, fade = false;
};
// conv_launch_objects with n_dirs = 2 directions and a weight per object (one launch of k_conv_p1_objects_blend) or n_dirs = 3
// directions and two weights (k_conv_p1_objects_blend3)
int conv_launch_objects_blend(ConvState &c, DeviceCtx *ctx, const float *in, long long in_ss, long long in_cs, float *out, long long out_ss,
                              long long out_cs, int n_blocks, float gain, hipStream_t st, int n_objects, int n_dirs,
                              const ConvObjectBlendRows &rows);
// the handle's four responses become set `set` of the table, overlaps and history untouched (asynchronous on st)
int conv_adopt_schedule_set(ConvState &c, size_t set, hipStream_t st);
// the per-path overlaps from the lazy state with the CURRENT spectra, the lazy state kept valid beside them (tails_both)
int conv_materialise_keep_lazy(ConvState &c, DeviceCtx *ctx, hipStream_t st);

// ---- speaker angles -> four set_ir (the wiring the reference leaves open; speakers.cpp) ---------
template <class SetIr>
int set_speakers_impl(ConvState &c, const ohs_sofa *sofa, float az_l, float el_l, float az_r, float el_r, float radius_m,
                      float fs, unsigned *changed_mask, SetIr set_ir)
{
    if (changed_mask) *changed_mask = 0;
    if (!sofa) return fail(OHS_ERR_INVALID_ARG, "sofa is NULL");
    std::vector<float> irs[4];
    int rc = ohs_host::speaker_irs(sofa, az_l, el_l, az_r, el_r, radius_m, fs, irs);
    if (rc) return rc;
    for (int p = 0; p < 4; ++p) {
        if (c.spk_set[p] && c.spk_ir[p] == irs[p]) continue;        // same nearest measurement as before: nothing to do
        rc = set_ir(p, irs[p].data(), irs[p].size());
        if (rc) return rc;
        c.spk_ir[p].swap(irs[p]);
        c.spk_set[p] = true;
        if (changed_mask) *changed_mask |= 1u << p;
    }
    return OHS_OK;
}

// ---- EQ table / state shared by ohs_eq (1 stream) and ohs_batch -------------------
struct EqState {
    size_t nb = 0;
    size_t chains = 2;
    std::vector<float> coeffs;   // nb * 5  {b0,b1,b2,a1,a2}
    std::vector<int> en;         // nb
    float *d_state = nullptr;    // [chains][kEqStateSlots][2], indexed by band
    bool exact_specials = false; // ohs_*_set_eq_exact_specials: conveyor kernel, exact for -0.0 / around non-finite input
    int fp_mode = 0;             // denormal handling (kernels.h: ohs_set_fp_mode)
    int xcd_lo = 0, xcd_n = 8;   // XCDs the ring kernel's launches may use (kernels.h: xcd_grid); set per call by the batch
    // Per-stream tables (ohs_batch_set_stream_eq_band_coeffs): every stream owns its bands, as every plugin instance of the
    // reference does (parametric_eq.rs:125-129).  Host copy [streams][nb] of coefficients and enable flags, created from the
    // shared table by the first per-stream edit; the compacted device tables are uploaded by the next launch.
    bool per_stream = false;
    std::vector<float> s_coeffs;         // streams * nb * 5
    std::vector<unsigned char> s_en;     // streams * nb
    EqStreamTable *d_stabs = nullptr;    // [passes][streams]: pass k = every stream's enabled bands 12 k .. 12 k + 11
    size_t stabs_passes = 0;
    bool stabs_dirty = true;
    size_t max_enabled = 0;              // largest number of enabled bands of any stream (as of the last upload scan)
    unsigned long long *d_stamps = nullptr;     // [4] clock stamps of the last ring launch's wave 0 (ohs_batch_set_profiling)
    // what served the last EQ launch (ohs_batch_last_eq_form): OHS_EQ_FORM_*, and whether it was k_eq_ring_sched
    int last_form = 0;
    bool last_scheduled = false;
    // Schedule tables (ohs_batch_set_schedule_tables): host copies [n][nb][5] / [n][nb], and for the scheduled wave ring every
    // table's lane constants, compacted by its own enabled flags (kernels.h: EqRingSched::lane_tabs, [n][5][16]; a table with
    // no or more than 12 enabled bands never reaches that kernel, its entry is the pass-on lane's constants)
    size_t sched_n = 0;
    std::vector<float> sched_coeffs;
    std::vector<unsigned char> sched_en;
    float *d_sched_lanes = nullptr;
    // for the per-stream scheduled call: every schedule table as EqStreamTables, compacted by its own flags, 12 bands per pass --
    // d_sched_stabs[pass * sched_n + table] (pass 0 is what k_eq_ring_sched_streams reads); sched_on = enabled bands per table,
    // sched_class = a number per distinct set of enabled flags (two tables have equal flags iff equal class);
    // d_sched_gather [sched_passes][streams]: the per-stream tables of the span a fallback launch serves, filled in stream order
    // right in front of that launch (launch_eq_gather_tables)
    ohs::EqStreamTable *d_sched_stabs = nullptr, *d_sched_gather = nullptr;
    size_t sched_passes = 0;
    std::vector<unsigned char> sched_on;
    std::vector<unsigned> sched_class;
};

// One scheduled batch call, as the launches see it: segment k = blocks [k seg_blocks, (k + 1) seg_blocks) of the call.  tab / gain
// are the caller's host arrays (either may be NULL: the handle's table / gain throughout), d_tab / d_gain their device copies.
struct BatchSchedule {
    size_t seg_blocks = 1, n_segs = 0;
    const unsigned *tab = nullptr;
    const float *gain = nullptr;
    const unsigned *d_tab = nullptr;
    const float *d_gain = nullptr;
    // ohs_batch_process_scheduled_streams: a row per stream -- stream s reads tab / d_tab at s * tab_stride and gain / d_gain at
    // s * gain_stride (0: one row for all streams; else >= n_segs).  seg_bits[k], over ALL streams: kSegIdxChange -- some stream's
    // index differs from segment k - 1's; kSegFlagsChange -- some stream's enabled flags do; kSegNoRing -- some stream's table has
    // no or more than 12 enabled bands.  seg_max_on[k]: the largest number of enabled bands of any stream's table in segment k.
    bool streams = false;
    size_t tab_stride = 0, gain_stride = 0;
    static constexpr unsigned char kSegIdxChange = 1, kSegFlagsChange = 2, kSegNoRing = 4;
    std::vector<unsigned char> seg_bits, seg_max_on;
};


int eq_init(EqState &e, size_t nb, size_t chains, float fs, hipStream_t st);
int eq_reset(EqState &e, hipStream_t st);
int eq_single_pass_table(const EqState &e, EqPassTable &t);
bool eq_any_enabled(const EqState &e);      // some band of the shared table, or of any stream's own table, is enabled
int eq_set_stream_band(EqState &e, size_t stream, size_t band, const float coeffs[5], int enabled);
void eq_set_shared_band(EqState &e, size_t band, const float coeffs[5], int enabled);   // ... and of every stream's own table
void eq_share_table(EqState &e);            // back to the one shared table
void eq_free(EqState &e);
int eq_launch(EqState &e, const float *in, float *out, long long ss, long long cs, long long n,
              hipStream_t st, bool *did_anything = nullptr, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
int eq_set_schedule_tables(EqState &e, size_t n_tables, const float *coeffs, const uint8_t *enabled, hipStream_t st);
bool eq_schedule_table_any_enabled(const EqState &e, size_t table);
// the cascade over blocks [blk0, blk0 + n_blocks) of a scheduled call (shared table only; sc.tab != NULL); in / out point at blk0
int eq_launch_scheduled(EqState &e, const BatchSchedule &sc, size_t blk0, size_t n_blocks, const float *in, float *out,
                        long long ss, long long cs, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop);
// the same with a row of table indices per stream (sc.streams, sc.tab != NULL).  First, one pass over the rows (sc.tab, tab_stride,
// n_segs set) that fills sc.seg_bits / seg_max_on; false: an index is out of range (nothing else is to be trusted then)
bool eq_schedule_streams_scan(const EqState &e, BatchSchedule &sc);
int eq_launch_scheduled_streams(EqState &e, const BatchSchedule &sc, size_t blk0, size_t n_blocks, const float *in, float *out,
                                long long ss, long long cs, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop);

// ---- growable planar device FIFO [2][cap] (api_engine.hip) -----------------------------
struct DevFifo {
    float *d = nullptr;
    size_t cap = 0, len = 0;
};

}  // namespace ohs_api

using ohs_api::ConvState;
using ohs_api::DevFifo;
using ohs_api::DeviceCtx;
using ohs_api::EqState;
using ohs::RtMailbox;

// =======================================================================================
// handles
// =======================================================================================
struct ohs_engine {
    int device = 0;
    DeviceCtx *ctx = nullptr;
    hipStream_t st = nullptr;
    ConvState conv;
    DevFifo in, out, scratch;
    float *d_stage = nullptr;   // [2][stage_cap] pop staging (gain applied here)
    size_t stage_cap = 0;
    // single-launch call path (f2): pinned host staging mapped into the device + EQ output buffer
    float *h_in = nullptr, *h_out = nullptr;      // host [2][hcap]
    float *dm_in = nullptr, *dm_out = nullptr;    // the same memory, device addresses
    float *d_eqbuf = nullptr;                     // device [2][hcap]
    unsigned *h_done = nullptr, *dm_done = nullptr;   // completion word of the single-launch call (pinned; host / device address)
    unsigned call_seq = 0;
    size_t hcap = 0;
    uint64_t silent_frames = 0;                   // frames answered with the zero fill of convolution.rs:176-181
    // resident real-time kernel (ohs_engine_set_realtime): mailbox in pinned mapped memory, its own stream
    bool rt_enabled = false, rt_running = false, rt_slot = false;   // rt_slot: counted in the device's resident-kernel cap
    bool rt_wedged = false;         // a resident kernel did not leave within 5 s of its stop request and may still be alive:
                                    // it holds pointers to this engine's state, its mailbox and its stream (rt_stop)
    RtMailbox *mb = nullptr, *mb_dev = nullptr;
    hipStream_t rt_st = nullptr;
    unsigned rt_seq = 0;
    unsigned rt_eq_version = 0;     // version of the EQ block in the mailbox (bumped whenever its content changes)
};

struct ohs_eq {
    int device = 0;
    DeviceCtx *ctx = nullptr;
    hipStream_t st = nullptr;
    EqState eq;
    float fs = 48000.0f;
    float *d_buf = nullptr;     // [2][buf_cap]
    size_t buf_cap = 0;
    float *h_pin = nullptr;     // [2][pin_cap] pinned + mapped host staging for real-time sized calls
    float *dm_pin = nullptr;    // its device address
    float *d_pinbuf = nullptr;  // [2][pin_cap] device side
    unsigned *h_done = nullptr, *dm_done = nullptr, *d_counter = nullptr;   // completion word (pinned) + its workgroup counter
    unsigned call_seq = 0;
    size_t pin_cap = 0;
};

struct ohs_biquad {          // BiquadFilter (parametric_eq.rs:46-123): one DF2T section, one (mono) chain
    int device = 0;
    DeviceCtx *ctx = nullptr;
    hipStream_t st = nullptr;
    EqState eq;                 // one band, one chain
    float *d_buf = nullptr;
    size_t cap = 0;
};

struct ohs_batch {
    int device = 0;
    DeviceCtx *ctx = nullptr;
    hipStream_t st = nullptr;   // for set-up work only
    ConvState conv;
    EqState eq;
    int eq_enable = 0;
    float gain = 1.0f;
    // A HIP failure in the middle of a processing call leaves the per-stream state advanced for some time chunks only:
    // the handle is marked failed and every later processing call is refused until ohs_batch_reset (which zeroes the
    // state) -- never a continuation on half-advanced state.
    bool failed = false;
    std::string fail_msg;
    hipStream_t st2 = nullptr;  // convolution of time chunk i runs here while the EQ of chunk i+1 runs on the caller's stream
    bool overlap = true;
    int xcd_split = 0;          // x > 0: overlapped calls run the EQ on XCDs [0, x) and the convolution on [x, 8)
    // optional per-kernel timing: (begin, end, kind) event pairs; kind 0 = EQ, 1 = convolution
    bool profiling = false;
    struct Span { hipEvent_t a, b; int kind; };
    std::vector<Span> spans;
    uint64_t prof_calls = 0;
    std::vector<hipEvent_t> ev_pool;
    std::vector<hipEvent_t> ev_inflight;   // ordering events of the current / previous calls
    // ohs_batch_process_deferred: the convolutions of the previous call may still be running on st2
    std::vector<hipEvent_t> chunk_done;    // one persistent event per time chunk, re-recorded on st2 by every such call
    int chunk_done_n = 0;                  // chunks of the pending call
    bool join_pending = false;
    const float *pend_out = nullptr;       // geometry of the pending call: per-chunk waits only if the next one matches
    size_t pend_blocks = 0, pend_ss = 0, pend_cs = 0;
    // ohs_batch_process_host: three staging slots [S][2][slot_frames], copy-in / compute / copy-out streams
    static constexpr int kHostSlots = 3;
    float *d_slot[kHostSlots] = {nullptr, nullptr, nullptr};
    size_t slot_frames = 0;
    hipStream_t st_h2d = nullptr, st_comp = nullptr, st_d2h = nullptr;
    hipEvent_t ev_h2d[kHostSlots] = {nullptr, nullptr, nullptr}, ev_comp[kHostSlots] = {nullptr, nullptr, nullptr},
               ev_d2h[kHostSlots] = {nullptr, nullptr, nullptr};
    // The scheduled calls: a call's rows (table indices, gains, set indices, prev_idx) travel through one of kSchedSlots staging
    // slots -- pinned host memory and its device copy, `cap` 32-bit entries each, the call's arrays packed one behind the other
    // and copied in one go; `done` is recorded behind the call that used the slot and waited for before the slot is filled
    // again (api_batch.hip: SchedLease)
    static constexpr int kSchedSlots = 4;
    struct SchedSlot {
        unsigned *h = nullptr, *d = nullptr;
        size_t cap = 0;
        hipEvent_t done = nullptr;
        bool in_use = false;
    };
    SchedSlot sched_slot[kSchedSlots];
    int sched_next = 0;
};
