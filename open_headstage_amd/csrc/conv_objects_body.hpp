// conv_objects_body.hpp -- what the three object-scene kernels share: k_conv_p1_objects (conv_objects_kernels.hip, one direction per
// object), k_conv_p1_objects_blend (conv_objects_blend_kernels.hip, two) and k_conv_p1_objects_blend3 (conv_objects_blend3_kernels.hip,
// three).  Each kernel stays in a translation unit of its own -- all three sit at the edge of the 168 VGPRs that three waves per SIMD
// leave, and a kernel beside another one changed how hipcc allocates it -- but the helpers, the three passes and the launch stand here
// once, and so does the block loop of the two- and the three-direction kernel: a promise that one call has another call's bits
// (SCENES.md) is a promise about one function instantiated twice.  k_conv_p1_objects keeps a block loop of its own
// (conv_objects_kernels.hip says why) over the same helpers, two-row pass and launch.  Built with the FFT kernels' flags
// (-fno-slp-vectorize -ffp-contract=off): every operation rounds by itself.  The order of the loads and of the operands below is what
// holds the kernels at their register figures (libohs_hip.resources.json; DESIGN.md sections 4.5h, 4.5i, 4.5k): recompile and compare
// after every change.
#pragma once
#include "kernels.h"
#include "wave_fft.hpp"

#include <atomic>

namespace ohs {

constexpr int kObjWaves = OHS_LAYOUT_WAVES;                 // the layout kernels' workgroup shape (kernels.h)
constexpr int kObjWavesPerSimd = OHS_LAYOUT_WAVES_PER_SIMD;
constexpr size_t kObjLdsBytes = (kTabComplex + kObjWaves * kWaveLdsComplex) * sizeof(float2);
constexpr bool kObjLdsPlanFits = kObjLdsBytes * (4 * kObjWavesPerSimd / kObjWaves) <= 160 * 1024;
// (conv_kernels.hip's: the audio is read once and written once)
#define OHS_P1_LD(p) __builtin_nontemporal_load(p)
#define OHS_P1_ST(p, v) __builtin_nontemporal_store((v), (p))
// table loads in flight: the two-row pass has groups of four positions of two rows (16 VGPRs); the four-row pass a rolling window of
// OHS_P1_BLEND_DEPTH half-positions of two rows each (12 VGPRs at depth 3: what fits without scratch -- depth 4 cost 40 B / lane);
// the six-row pass a rolling window of OHS_P1_BLEND3_ROWS single rows (8 VGPRs at 4 rows: 5 rows cost 8 B / lane, 6 rows
// 16 B / lane, and whole half-positions of three rows fit at depth 1 only)
#ifndef OHS_P1_IRS_GROUP
#define OHS_P1_IRS_GROUP 4
#endif
#ifndef OHS_P1_BLEND_DEPTH
#define OHS_P1_BLEND_DEPTH 3
#endif
#ifndef OHS_P1_BLEND3_ROWS
#define OHS_P1_BLEND3_ROWS 4
#endif
#ifndef OHS_P1_BLEND_FENCE
#define OHS_P1_BLEND_FENCE __builtin_amdgcn_sched_barrier(0);
#endif
#ifndef OHS_P1_IRS_FENCE
#define OHS_P1_IRS_FENCE __builtin_amdgcn_sched_barrier(0);
#endif

// > 64 KiB of dynamic LDS needs an opt-in function attribute, per device.
static hipError_t objects_allow_large_lds(const void *fn, size_t bytes, std::atomic<unsigned long long> &done_mask)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (done_mask.load(std::memory_order_acquire) & bit) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) done_mask.fetch_or(bit, std::memory_order_release);
    return e;
}

// workgroup index inside the launch's XCD set, or -1 for a workgroup on another XCD (kernels.h: xcd_grid)
__device__ __forceinline__ long long objects_xcd_block(const ConvP1Args &A)
{
    unsigned bid = blockIdx.x;
    if (A.xcd_n != 8) {
        const unsigned x = (bid & 7u) - (unsigned)A.xcd_lo;
        if (x >= (unsigned)A.xcd_n) return -1;
        bid = (bid >> 3) * (unsigned)A.xcd_n + x;
    }
    return (long long)bid;
}

// A wave-uniform 32-bit entry of a row that nobody writes while the kernel runs, read through the constant address space: with a
// uniform address hipcc makes it a scalar load (a plain load + readfirstlane was a vector load and a full memory wait per entry:
// four round trips in series in front of every pass).
__device__ __forceinline__ unsigned uniform_entry(const unsigned *p)
{
    return *(const __attribute__((address_space(4))) unsigned *)(p);
}

// ---- the rows of a launch, as the launch checks them ------------------------------------------------------------------------------
//   ConvObjectsArgs       one direction per object; index rows and gain rows behind pointers of their own, every one but idx nullable
//   ConvObjectsBlendArgs  NDIR = 2 or 3 directions per object in 2 NDIR planes of one shape, `plane` entries apart -- NDIR direction
//                         indices, NDIR - 1 weights, the gain (only if has_gain; else 1.0f) --, and in front of the call's first block
//                         as many planes of [n_objects], `prev_plane` apart (under CROSSFADE the host always stages them)
static bool objects_rows_ok(const ConvObjectsArgs &l) { return l.idx && l.seg >= 1 && l.stream >= 0 && l.prev_stream >= 0; }
static bool objects_rows_ok(const ConvObjectsBlendArgs &l)
{
    return l.rows && l.plane >= 1 && l.seg >= 1 && l.stream >= 0 && l.prev_stream >= 0 && !(l.fade && (!l.prev || l.prev_plane < 1));
}

// ---- the three passes ---------------------------------------------------------------------------------------------------------------
// What ends every pass: position i's rows a, b of the pair's two objects -> the pair's (C, D), c = (a.x + b.y, a.y - b.x),
// d = (a.x - b.y, a.y + b.x), then the expression of p1_spectral_product_paired_global (_add), operation for operation.  Within the
// normal range 0.5 u + 0.5 v has the bits of 0.5 (u + v), so c and d are what k_build_cd -> k_irs_tables(kLayoutTableScale) put into a
// layout table for the same four responses.
template <bool ADD>
__device__ __forceinline__ void objects_pair_product(const float2 (&z)[16], float2 (&w)[16], int i, float2 a, float2 b, bool lane32)
{
    const float2 zz = z[i], m = paired_mirror(z, i >> 2, i & 3, lane32);
    const float2 c = make_float2(a.x + b.y, a.y - b.x), d = make_float2(a.x - b.y, a.y + b.x);
    const float wx = fmaf(m.y, d.y, fmaf(m.x, d.x, fmaf(-zz.y, c.y, zz.x * c.x)));
    const float wy = fmaf(-m.y, d.x, fmaf(m.x, d.y, fmaf(zz.y, c.x, zz.x * c.y)));
    if (ADD) { w[i].x += wx; w[i].y += wy; }
    else { w[i].x = wx; w[i].y = wy; }
}

// the two-row pass: one row per object.  Two 8-byte loads per position where the layout kernels have one 16-byte load, and four additions.
template <bool ADD>
__device__ __forceinline__ void objects_pass_rows2(const float2 (&z)[16], float2 (&w)[16], const float2 *ap, const float2 *bp, int lane)
{
    constexpr int G = OHS_P1_IRS_GROUP;
    const bool lane32 = lane == 32;
#pragma unroll
    for (int g = 0; g < 16 / G; ++g) {
        float2 qa[G], qb[G];
        OHS_P1_IRS_FENCE
#pragma unroll
        for (int j = 0; j < G; ++j) { qa[j] = ap[(G * g + j) * 64]; qb[j] = bp[(G * g + j) * 64]; }
#pragma unroll
        for (int j = 0; j < G; ++j) objects_pair_product<ADD>(z, w, G * g + j, qa[j], qb[j], lane32);
    }
}

// The rows of the four- and the six-row pass are read through ONE buffer descriptor over the whole table with the row as the scalar
// offset and the lane's 8 bytes as the only per-lane address: four 64-bit pointers would be eight VGPRs, which these kernels do not
// have (three waves per SIMD, no scratch).
typedef float objects_v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float2 objects_row_load(__amdgpu_buffer_rsrc_t table, int off, int row_bytes, int i)
{
    const objects_v2f q = __builtin_bit_cast(objects_v2f, __builtin_amdgcn_raw_buffer_load_b64(table, off, row_bytes + i * 64 * (int)sizeof(float2), 0));
    return make_float2(q.x, q.y);
}

// the four-row pass: each object's row is u A[d0] + w A[d1] per component -- two multiplications and one addition, each rounded by
// itself --, u = 1 - w formed once per pass by the caller.  w = 0 gives 1 A[d0] + 0 A[d1] = A[d0] and w = 1 gives A[d1] for finite rows.
template <bool ADD>
__device__ __forceinline__ void objects_pass_rows4(const float2 (&z)[16], float2 (&w)[16], __amdgpu_buffer_rsrc_t table, int ra0, int ra1,
                                                   int rb0, int rb1, int off, float ua, float wa, float ub, float wb, int lane)
{
    const bool lane32 = lane == 32;
    // A rolling window over the pass's 32 half-positions (position i's two rows of object a, then its two rows of object b): three
    // halves -- six loads, 12 VGPRs -- are in flight at any time, and the slot a half leaves is refilled at once, so the window
    // never drains between positions the way a load group does between groups.
    constexpr int D = OHS_P1_BLEND_DEPTH;
    float2 q0[D], q1[D];
    auto issue = [&](int h) {
        const int i = h >> 1;
        q0[h % D] = objects_row_load(table, off, (h & 1) ? rb0 : ra0, i);
        q1[h % D] = objects_row_load(table, off, (h & 1) ? rb1 : ra1, i);
    };
#pragma unroll
    for (int h = 0; h < D; ++h) issue(h);
    float2 a = make_float2(0.0f, 0.0f);
#pragma unroll
    for (int h = 0; h < 32; ++h) {
        OHS_P1_BLEND_FENCE
        const float us = (h & 1) ? ub : ua, ws = (h & 1) ? wb : wa;
        const float2 r = make_float2(us * q0[h % D].x + ws * q1[h % D].x, us * q0[h % D].y + ws * q1[h % D].y);
        if (h + D < 32) issue(h + D);
        if (!(h & 1)) { a = r; continue; }
        objects_pair_product<ADD>(z, w, h >> 1, a, r, lane32);
    }
}

// the six-row pass: each object's row is (u A[d0] + w1 A[d1]) + w2 A[d2] per component -- three multiplications and two additions,
// each rounded by itself, in that order --, u = (1 - w1) - w2 formed once per pass by the caller.  The window holds OHS_P1_BLEND3_ROWS
// single rows, consumed in the order of the sum.  ra / rb: the byte offsets of object a's / b's three rows; ka / kb: their (u, w1, w2).
template <bool ADD>
__device__ __forceinline__ void objects_pass_rows6(const float2 (&z)[16], float2 (&w)[16], __amdgpu_buffer_rsrc_t table, const int (&ra)[3],
                                                   const int (&rb)[3], int off, const float (&ka)[3], const float (&kb)[3], int lane)
{
    const bool lane32 = lane == 32;
    // A rolling window over the pass's 96 row loads (half-position h's three rows, in the order of the sum): R are in flight, and the
    // slot a row leaves is refilled at once.
    constexpr int R = OHS_P1_BLEND3_ROWS;
    float2 q[R];
    auto issue = [&](int n) {
        const int h = n / 3, j = n % 3;
        q[n % R] = objects_row_load(table, off, (h & 1) ? rb[j] : ra[j], h >> 1);
    };
#pragma unroll
    for (int n = 0; n < R; ++n) issue(n);
    float2 a = make_float2(0.0f, 0.0f);
#pragma unroll
    for (int h = 0; h < 32; ++h) {
        OHS_P1_BLEND_FENCE
        float2 r = make_float2(0.0f, 0.0f);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int n = 3 * h + j;
            const float ks = (h & 1) ? kb[j] : ka[j];
            const float2 t = make_float2(ks * q[n % R].x, ks * q[n % R].y);
            r = j == 0 ? t : make_float2(r.x + t.x, r.y + t.y);       // (u A[d0] + w1 A[d1]) + w2 A[d2]
            if (n + R < 96) issue(n + R);
        }
        if (!(h & 1)) { a = r; continue; }
        objects_pair_product<ADD>(z, w, h >> 1, a, r, lane32);
    }
}

// ---- the block loop -----------------------------------------------------------------------------------------------------------------
// k_conv_p1_layout_irs (conv_kernels.hip) for K independently moving sources:
//   result = gain * sum over objects c of conv(u_c h[d0_c] + w1_c h[d1_c] + w2_c h[d2_c], x_c gain_c),  u = (1 - w1) - w2,
// with two or three of the terms (NDIR); `old` is the previous segment's entry, what stands in front of the call's first block there.  The table holds one row per DIRECTION, ahalf[dir][i] = 0.5 (Hl + j Hr) in
// the paired layout, and a pass forms its pair's (C, D) from the two objects' rows (objects_pair_product).  An odd last object pairs
// with the table's all-zero row, and its partner's weights count as +0.0.
// Every object has its own entries per segment (wave-uniform: read per pass, not kept -- K may be 64).  A wave-uniform three-way
// choice per pass:
//   both objects' w1 and w2 have the bits of +0.0:  two rows -- k_conv_p1_objects's only pass, the same function;
//   otherwise both w2 have the bits of +0.0:        four rows, d2 never read -- with two directions, every other pass;
//   otherwise:                                      six rows.
// So a pass of the three-direction kernel with w2 = +0.0 IS the two-direction kernel's pass: the same function.
// Under CROSSFADE an object changes in the first block of a segment by the rule at `changes` below, and a pair fades when either of its objects
// changes: one vector load of the rows and a ballot give the block's 64 change bits, computed in front of the previous block's
// inverse transform so that the prefetch knows the first pair.  Passes of a block: for every fading pair, p ascending,
// (x gain_old) g[n] through the OLD entries; then for every pair, p ascending, (x gain_cur) f[n] through the current ones if the
// pair fades, x gain_cur if not.  One accumulator, one inverse transform.  No change and gains 1.0: k_conv_p1_layout's block; every
// pair fading and gains 1.0: k_conv_p1_layout_irs's fading block -- pass for pass (x * 1.0f is exact).  Workgroup shape, LDS plan,
// chunks with a dry block, address idiom, tail, store and merged_out are k_conv_p1_layout_irs's.
template <int NDIR>
__device__ __forceinline__ void objects_block_loop(const ConvP1Args &A, const ConvObjectsBlendArgs &L)
{
    constexpr bool TRI = NDIR == 3;
    static_assert(NDIR == 2 || NDIR == 3, "two or three directions per object (k_conv_p1_objects has a loop of its own)");
    constexpr int PW1 = NDIR, PW2 = NDIR + 1, PG = 2 * NDIR - 1;        // the planes of w1, of w2 (three directions) and of the gain
    const long long wg = objects_xcd_block(A);
    if (wg < 0) return;
    ohs_set_fp_mode(A.fp_mode);
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    float2 *tab = smem;
    fill_twiddle_tables(tab, A.tw, threadIdx.x, 64 * kObjWaves);
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const unsigned ul = (unsigned)lane;
    float2 *lds = smem + kTabComplex + wave * kWaveLdsComplex;
    const long long gw = wg * kObjWaves + wave;
    if (gw >= (long long)A.n_streams * A.chunks) return;
    const int s = __builtin_amdgcn_readfirstlane((int)(gw / A.chunks));
    const int ck = __builtin_amdgcn_readfirstlane((int)(gw % A.chunks));
    const int b0 = __builtin_amdgcn_readfirstlane((int)((long long)ck * A.n_blocks / A.chunks));
    const int b1 = __builtin_amdgcn_readfirstlane((int)((long long)(ck + 1) * A.n_blocks / A.chunks));
    if (b0 >= b1) return;
    const int t_first = ck > 0 ? b0 - 1 : b0;
    const int P = L.n_pairs, K = L.n_objects;

    const float *in_s = A.in + (size_t)s * A.in_stream_stride;
    float *ql = A.out + (size_t)s * A.out_stream_stride + (size_t)t_first * kBlock;

    const unsigned kOne = 0x3f800000u;
    // the stream's rows: 2 NDIR planes of one shape, L.plane entries apart, and in front of the call's first block as many planes of
    // [n_objects], L.prev_plane apart
    const unsigned *rows = L.rows + (size_t)s * (size_t)L.stream;
    const unsigned *prev = L.prev ? L.prev + (size_t)s * (size_t)L.prev_stream : nullptr;
    const size_t plane = (size_t)L.plane, pplane = (size_t)L.prev_plane;
    const bool has_gain = L.has_gain != 0;
    // plane 0 of segment k's entries, of the ones in front of them, and the plane stride that goes with each
    auto cur_of = [&](int k) { return rows + (size_t)k * (size_t)K; };
    auto old_of = [&](int k) { return k > 0 ? cur_of(k - 1) : prev ? prev : cur_of(0); };
    auto old_plane = [&](int k) { return k > 0 || !prev ? plane : pplane; };
    // bit c: object c changes in block (segment k, position r): when d0, the bits of w1, w2 or the gain differ from the entry in front,
    // or d1 does beside a w1 that is not +0.0 on both sides, or d2 beside such a w2 (a second / third index beside a weight of +0.0
    // before and after takes no part in any pass: no change of the object)
    auto changes = [&](int k, int r) -> unsigned long long {
        if (!L.fade || r != 0) return 0ull;
        const unsigned *c = cur_of(k), *o = old_of(k);
        const size_t op = old_plane(k);
        bool ch = false;
        if (lane < K) {
            const unsigned cw1 = c[PW1 * plane + lane], ow1 = o[PW1 * op + lane], cw2 = TRI ? c[PW2 * plane + lane] : 0u, ow2 = TRI ? o[PW2 * op + lane] : 0u;
            ch = c[lane] != o[lane] || cw1 != ow1 || cw2 != ow2 || ((cw1 | ow1) != 0u && c[plane + lane] != o[op + lane]) ||
                 ((cw2 | ow2) != 0u && c[2 * plane + lane] != o[2 * op + lane]);
            if (has_gain) ch = ch || c[PG * plane + lane] != o[PG * op + lane];
        }
        return __builtin_amdgcn_ballot_w64(ch);
    };
    auto first_pair = [](unsigned long long chg) { return chg ? (int)(__builtin_ctzll(chg) >> 1) : 0; };
    int lay_k = __builtin_amdgcn_readfirstlane(t_first / L.seg);
    int lay_r = __builtin_amdgcn_readfirstlane(t_first - lay_k * L.seg);

    float2 tail[8];
    if (ck == 0) {
        const float2 *mt = A.merged_in + (size_t)s * (8 * 64);
#pragma unroll
        for (int a = 0; a < 8; ++a) tail[a] = mt[a * 64 + ul];
    } else {
#pragma unroll
        for (int a = 0; a < 8; ++a) tail[a] = make_float2(0.0f, 0.0f);
    }
    float xa[8], xb[8];
    auto request = [&](int t, int p) {
        unsigned u = ul;
        asm volatile("" : "+v"(u));
        const float *pa = in_s + (size_t)(2 * p) * A.in_ch_stride + (size_t)t * kBlock + u;
#pragma unroll
        for (int a = 0; a < 8; ++a) xa[a] = OHS_P1_LD(&pa[64 * a]);
        if (2 * p + 1 < K) {
            const float *pb = pa + A.in_ch_stride;
#pragma unroll
            for (int a = 0; a < 8; ++a) xb[a] = OHS_P1_LD(&pb[64 * a]);
        } else {
#pragma unroll
            for (int a = 0; a < 8; ++a) xb[a] = 0.0f;
        }
    };
    unsigned long long chg = changes(lay_k, lay_r);
    request(t_first, first_pair(chg));
    const PairedPlan plan = paired_plan(lane);
    // the whole direction table, zero row included, for the four- and six-row passes' loads (wave-uniform; a load past it would read 0)
    const __amdgpu_buffer_rsrc_t table = __builtin_amdgcn_make_buffer_rsrc(const_cast<float2 *>(L.ahalf), 0,
                                                                            (int)((L.zero_dir + 1u) * (unsigned)(kFft * sizeof(float2))), 0x00020000);
    for (int t = t_first; t < b1; ++t) {
        const bool dry = t < b0;
        float2 w[16];
        bool old_half = chg != 0ull;    // the passes through the old directions come first
        int p = first_pair(chg);
        bool first = true;
        for (;;) {
            const bool fading = ((chg >> (2 * p)) & 3ull) != 0ull;
            // this pass's entries: the old ones in the old half of a fade (directions, weights and gain alike), the segment's own elsewhere
            const unsigned *re = (old_half ? old_of(lay_k) : cur_of(lay_k)) + 2 * p;
            const size_t rp = old_half ? old_plane(lay_k) : plane;
            const bool partner = 2 * p + 1 < K;
            const unsigned da = uniform_entry(re), db = partner ? uniform_entry(re + 1) : L.zero_dir;
            const unsigned wa_bits = uniform_entry(re + PW1 * rp), wb_bits = partner ? uniform_entry(re + PW1 * rp + 1) : 0u;
            const unsigned wa2_bits = TRI ? uniform_entry(re + PW2 * rp) : 0u, wb2_bits = TRI && partner ? uniform_entry(re + PW2 * rp + 1) : 0u;
            const float ga = __uint_as_float(has_gain ? uniform_entry(re + PG * rp) : kOne);
            const float gb = __uint_as_float(has_gain && partner ? uniform_entry(re + PG * rp + 1) : kOne);
            float2 v[16];
            if (fading) {
                float n = (float)lane;
                asm volatile("" : "+v"(n));     // (the ramp values are not worth registers across the transforms)
                const float sn = old_half ? -n : n, c0 = old_half ? (float)kBlock : 0.0f, c64 = old_half ? -64.0f : 64.0f;
#pragma unroll
                for (int a = 0; a < 8; ++a) {
                    const float ramp = ((c0 + c64 * (float)a) + sn) * (1.0f / (float)kBlock);     // g, then f: exact
                    v[a] = make_float2((xa[a] * ga) * ramp, (xb[a] * gb) * ramp);
                }
            } else {
#pragma unroll
                for (int a = 0; a < 8; ++a) v[a] = make_float2(xa[a] * ga, xb[a] * gb);
            }
#pragma unroll
            for (int a = 0; a < 8; ++a) v[a + 8] = make_float2(0.0f, 0.0f);
            // the pass behind this one: the next fading pair of the old half, then pairs 0 .. P - 1 of the current one
            bool n_old = old_half, more = true;
            int n_p = p + 1;
            if (old_half) {
                const unsigned long long m = n_p < 32 ? chg >> (2 * n_p) : 0ull;
                if (m) n_p += (int)(__builtin_ctzll(m) >> 1);
                else { n_old = false; n_p = 0; }
            } else {
                more = n_p < P;
            }
            if (more) request(t, n_p);
            wave_fft_fwd_paired(v, lds, tab, lane, plan);
            unsigned u = ul;
            asm volatile("" : "+v"(u));
            constexpr int kRowBytes = kFft * (int)sizeof(float2);    // (65 537 rows of 8 KiB: below 2^31)
            if ((wa_bits | wb_bits | wa2_bits | wb2_bits) == 0u) {        // wave-uniform
                const float2 *ap = L.ahalf + (size_t)da * kFft + u, *bp = L.ahalf + (size_t)db * kFft + u;
                if (first) objects_pass_rows2<false>(v, w, ap, bp, lane);
                else objects_pass_rows2<true>(v, w, ap, bp, lane);
            } else {
                if ((wa2_bits | wb2_bits) == 0u) {                          // d2 is not read
                    const unsigned da1 = uniform_entry(re + rp), db1 = partner ? uniform_entry(re + rp + 1) : L.zero_dir;
                    const float wa = __uint_as_float(wa_bits), wb = __uint_as_float(wb_bits);
                    const float ua = 1.0f - wa, ub = 1.0f - wb;
                    const int off = (int)(ul * (unsigned)sizeof(float2));
                    if (first) objects_pass_rows4<false>(v, w, table, (int)da * kRowBytes, (int)da1 * kRowBytes, (int)db * kRowBytes,
                                                         (int)db1 * kRowBytes, off, ua, wa, ub, wb, lane);
                    else objects_pass_rows4<true>(v, w, table, (int)da * kRowBytes, (int)da1 * kRowBytes, (int)db * kRowBytes,
                                                  (int)db1 * kRowBytes, off, ua, wa, ub, wb, lane);
                } else if constexpr (NDIR == 3) {
                    const unsigned da1 = uniform_entry(re + rp), db1 = partner ? uniform_entry(re + rp + 1) : L.zero_dir;
                    const unsigned da2 = uniform_entry(re + 2 * rp), db2 = partner ? uniform_entry(re + 2 * rp + 1) : L.zero_dir;
                    const float wa = __uint_as_float(wa_bits), wb = __uint_as_float(wb_bits);
                    const float wa2 = __uint_as_float(wa2_bits), wb2 = __uint_as_float(wb2_bits);
                    const float ka[3] = {(1.0f - wa) - wa2, wa, wa2}, kb[3] = {(1.0f - wb) - wb2, wb, wb2};
                    const int ra[3] = {(int)da * kRowBytes, (int)da1 * kRowBytes, (int)da2 * kRowBytes};
                    const int rb[3] = {(int)db * kRowBytes, (int)db1 * kRowBytes, (int)db2 * kRowBytes};
                    const int off = (int)(ul * (unsigned)sizeof(float2));
                    if (first) objects_pass_rows6<false>(v, w, table, ra, rb, off, ka, kb, lane);
                    else objects_pass_rows6<true>(v, w, table, ra, rb, off, ka, kb, lane);
                }
            }
            first = false;
            if (!more) break;
            old_half = n_old; p = n_p;
        }
        if (++lay_r == L.seg) { lay_r = 0; ++lay_k; }
        // the next block's changes, in front of the prefetch of its first pair; behind the launch's last block the prefetch re-reads
        // that block (its own frames: in bounds; the values are never used)
        chg = t + 1 < b1 ? changes(lay_k, lay_r) : 0ull;
        request(t + 1 < A.n_blocks ? t + 1 : t, t + 1 < b1 ? first_pair(chg) : 0);
        wave_fft_inv_paired(w, lds, tab, lane, plan);
        if (!dry) {
            unsigned u = ul;
            asm volatile("" : "+v"(u));
            float *pl = ql + u, *pr = pl + A.out_ch_stride;
#pragma unroll
            for (int a = 0; a < 8; ++a) {
                OHS_P1_ST(&pl[64 * a], (w[a].x + tail[a].x) * A.gain);
                OHS_P1_ST(&pr[64 * a], (w[a].y + tail[a].y) * A.gain);
            }
        }
#pragma unroll
        for (int a = 0; a < 8; ++a) tail[a] = w[a + 8];
        ql += kBlock;
    }
    if (b1 == A.n_blocks) {         // the overlap the call leaves behind
        float2 *mo = A.merged_out + (size_t)s * (8 * 64);
#pragma unroll
        for (int a = 0; a < 8; ++a) mo[a * 64 + ul] = tail[a];
    }
}

// ---- the launch: launch_conv_p1_layout's checks and shape, plus the rows' -----------------------------------------------------------
// a.chunks as for launch_conv_p1_layout; the host has checked every index against the table and every weight against its range
template <class Args>
static hipError_t launch_objects_kernel(void (*kernel)(const ConvP1Args, const Args), const ConvP1Args &args, const Args &l, hipStream_t st)
{
    ConvP1Args a = args;
    a.gain = args.gain * (1.0f / kLayoutTableScale);        // the inverse transform's 1/N: the direction table comes without it
    if (a.n_blocks <= 0 || a.n_streams <= 0 || a.chunks > a.n_blocks) return hipErrorInvalidValue;
    if (!(a.chunks == 1 || a.chunks == 2 || a.chunks == 4 || a.chunks == 8 || a.chunks == 16)) return hipErrorInvalidValue;
    if (a.xcd_n < 1 || a.xcd_n > 8 || a.xcd_lo < 0 || a.xcd_lo + a.xcd_n > 8) return hipErrorInvalidValue;
    if (!a.in || !a.out || !a.merged_in || !a.merged_out || a.merged_in == a.merged_out || !a.tw) return hipErrorInvalidValue;
    if (!l.ahalf || l.n_objects < 1 || l.n_objects > 64 || l.n_pairs != (l.n_objects + 1) / 2) return hipErrorInvalidValue;
    if (!objects_rows_ok(l)) return hipErrorInvalidValue;
    static std::atomic<unsigned long long> lds_ok{0};       // (one kernel per translation unit, and this function is local to it)
    hipError_t e = objects_allow_large_lds(reinterpret_cast<const void *>(kernel), kObjLdsBytes, lds_ok);
    if (e != hipSuccess) return e;
    const long long waves = (long long)a.n_streams * a.chunks;
    const dim3 grid(xcd_grid((unsigned)((waves + kObjWaves - 1) / kObjWaves), a.xcd_n));
    hipLaunchKernelGGL(kernel, grid, dim3(64 * kObjWaves), kObjLdsBytes, st, a, l);
    return hipGetLastError();
}

}  // namespace ohs
