// conv_objects_kernels.hip -- k_conv_p1_objects: K independently moving sources per stream -> two ears in one kernel
// (ohs_scene_process, include/ohs_scene.h; kernels.h: ConvObjectsArgs), and the direction table it reads.
//
// A sibling of k_conv_p1_layout_irs (conv_kernels.hip) in a translation unit of its own: with this kernel inside conv_kernels.hip
// hipcc allocated six of that file's other kernels differently (k_conv_p1 107 instead of 108 VGPRs, k_conv_p1_edges 103 instead of
// 115, ...), and the kernels every earlier measurement was taken on are to stay the code they were.  The price is three small
// helpers restated here (the launch's XCD map, the large-LDS opt-in, the load / store macros), as conv_os_kernels.hip restates its own.
// Built with the FFT kernels' flags (-fno-slp-vectorize -ffp-contract=off): every operation rounds by itself, as in the layout kernels.
#include "kernels.h"
#include "wave_fft.hpp"

#include <atomic>

namespace ohs {

constexpr int kLayoutWaves = OHS_LAYOUT_WAVES;              // the layout kernels' workgroup shape (kernels.h)
constexpr int kLayoutWavesPerSimd = OHS_LAYOUT_WAVES_PER_SIMD;
static_assert((kTabComplex + kLayoutWaves * kWaveLdsComplex) * sizeof(float2) * (4 * kLayoutWavesPerSimd / kLayoutWaves) <= 160 * 1024,
              "k_conv_p1_objects: LDS plan");
// (conv_kernels.hip's: the audio is read once and written once; four table loads in flight per group)
#define OHS_P1_LD(p) __builtin_nontemporal_load(p)
#define OHS_P1_ST(p, v) __builtin_nontemporal_store((v), (p))
#ifndef OHS_P1_IRS_GROUP
#define OHS_P1_IRS_GROUP 4
#endif
#ifndef OHS_P1_IRS_FENCE
#define OHS_P1_IRS_FENCE __builtin_amdgcn_sched_barrier(0);
#endif

// > 64 KiB of dynamic LDS needs an opt-in function attribute, per device.
static hipError_t obj_allow_large_lds(const void *fn, size_t bytes, std::atomic<unsigned long long> &done_mask)
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
__device__ __forceinline__ long long p1_xcd_block(const ConvP1Args &A)
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

// k_conv_p1_objects: k_conv_p1_layout_irs (conv_kernels.hip) for K independently moving sources.  Two
// things differ from that kernel.
// The table holds one row per DIRECTION, ahalf[dir][i] = 0.5 (Hl + j Hr) in the paired layout, and a pass forms its pair's (C, D) from
// the two objects' rows: c = (a.x + b.y, a.y - b.x), d = (a.x - b.y, a.y + b.x), then the expression of p1_spectral_product_paired_global
// (_add), operation for operation.  Within the normal range 0.5 u + 0.5 v has the bits of 0.5 (u + v), so c and d are what k_build_cd ->
// k_irs_tables(kLayoutTableScale) put into a layout table for the same four responses.  Two 8-byte loads per position where the layout
// kernels have one 16-byte load, and four additions.  An odd last object pairs with the table's all-zero row.
// Every object has its own direction index and gain per segment (rows [segment][K] of 32-bit entries, wave-uniform: read per pass,
// not kept -- K may be 64).  `old` is the previous segment's entry, the caller's prev_* in front of the call's first block, the
// block's own where there is none.  Under CROSSFADE an object changes in the first block of a segment when its index or its gain's
// bits differ from old, and a pair fades when either of its objects changes: one vector load of both rows and a ballot give the
// block's 64 change bits, computed in front of the previous block's inverse transform so that the prefetch knows the first pair.
// Passes of a block: for every fading pair, p ascending, (x gain_old) g[n] through the OLD directions; then for every pair, p
// ascending, (x gain_cur) f[n] through the current ones if the pair fades, x gain_cur if not.  One accumulator, one inverse transform.
// No change and gains 1.0: k_conv_p1_layout's block; every pair fading and gains 1.0: k_conv_p1_layout_irs's fading block -- pass for
// pass (x * 1.0f is exact).  Workgroup shape, LDS plan, chunks with a dry block, address idiom, tail, store and merged_out are
// k_conv_p1_layout_irs's.  What the build gives (hipcc, gfx950; libohs_hip.resources.json): 165 VGPRs of the
// 168 that three waves per SIMD leave, 86 SGPRs, no scratch, three waves per SIMD -- with the load group of four as it is.
template <bool ADD>
__device__ __forceinline__ void p1_spectral_product_objects(const float2 (&z)[16], float2 (&w)[16], const float2 *ap, const float2 *bp, int lane)
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
        for (int j = 0; j < G; ++j) {
            const int i = G * g + j;
            const float2 zz = z[i], m = paired_mirror(z, i >> 2, i & 3, lane32);
            const float2 a = qa[j], b = qb[j];
            const float2 c = make_float2(a.x + b.y, a.y - b.x), d = make_float2(a.x - b.y, a.y + b.x);
            const float wx = fmaf(m.y, d.y, fmaf(m.x, d.x, fmaf(-zz.y, c.y, zz.x * c.x)));
            const float wy = fmaf(-m.y, d.x, fmaf(m.x, d.y, fmaf(zz.y, c.x, zz.x * c.y)));
            if (ADD) { w[i].x += wx; w[i].y += wy; }
            else { w[i].x = wx; w[i].y = wy; }
        }
    }
}

__global__ __launch_bounds__(64 * kLayoutWaves, kLayoutWavesPerSimd) void k_conv_p1_objects(const ConvP1Args A, const ConvObjectsArgs L)
{
    const long long wg = p1_xcd_block(A);
    if (wg < 0) return;
    ohs_set_fp_mode(A.fp_mode);
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    float2 *tab = smem;
    fill_twiddle_tables(tab, A.tw, threadIdx.x, 64 * kLayoutWaves);
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const unsigned ul = (unsigned)lane;
    float2 *lds = smem + kTabComplex + wave * kWaveLdsComplex;
    const long long gw = wg * kLayoutWaves + wave;
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

    // the stream's rows; a gain row that does not exist reads as 1.0f
    const unsigned kOne = 0x3f800000u;
    const unsigned *idx_row = L.idx + (size_t)s * (size_t)L.stream;
    const unsigned *gain_row = L.gain ? L.gain + (size_t)s * (size_t)L.stream : nullptr;
    const unsigned *pidx = L.prev_idx ? L.prev_idx + (size_t)s * (size_t)L.prev_stream : nullptr;
    const unsigned *pgain = L.prev_gain ? L.prev_gain + (size_t)s * (size_t)L.prev_stream : nullptr;
    // segment k's entries and the ones in front of them (k == 0 without prev_*: the segment's own, so nothing changes there)
    auto cur_idx = [&](int k) { return idx_row + (size_t)k * (size_t)K; };
    auto cur_gain = [&](int k) { return gain_row ? gain_row + (size_t)k * (size_t)K : nullptr; };
    auto old_idx = [&](int k) { return k > 0 ? cur_idx(k - 1) : pidx ? pidx : cur_idx(0); };
    auto old_gain = [&](int k) { return k > 0 ? cur_gain(k - 1) : pgain ? pgain : cur_gain(0); };
    // bit c: object c changes in block (segment k, position r)
    auto changes = [&](int k, int r) -> unsigned long long {
        if (!L.fade || r != 0) return 0ull;
        const unsigned *ci = cur_idx(k), *oi = old_idx(k), *cg = cur_gain(k), *og = old_gain(k);
        bool ch = false;
        if (lane < K) {
            ch = ci[lane] != oi[lane];
            const unsigned gc = cg ? cg[lane] : kOne, go = og ? og[lane] : kOne;
            ch = ch || gc != go;
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
    for (int t = t_first; t < b1; ++t) {
        const bool dry = t < b0;
        float2 w[16];
        bool old_half = chg != 0ull;    // the passes through the old directions come first
        int p = first_pair(chg);
        bool first = true;
        for (;;) {
            const bool fading = ((chg >> (2 * p)) & 3ull) != 0ull;
            const unsigned *ri = old_half ? old_idx(lay_k) : cur_idx(lay_k), *rg = old_half ? old_gain(lay_k) : cur_gain(lay_k);
            const bool partner = 2 * p + 1 < K;
            const unsigned da = uniform_entry(ri + 2 * p);
            const unsigned db = partner ? uniform_entry(ri + 2 * p + 1) : L.zero_dir;
            const float ga = __uint_as_float(rg ? uniform_entry(rg + 2 * p) : kOne);
            const float gb = __uint_as_float(rg && partner ? uniform_entry(rg + 2 * p + 1) : kOne);
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
            const float2 *ap = L.ahalf + (size_t)da * kFft + u, *bp = L.ahalf + (size_t)db * kFft + u;
            if (first) p1_spectral_product_objects<false>(v, w, ap, bp, lane);
            else p1_spectral_product_objects<true>(v, w, ap, bp, lane);
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

// the direction table of k_conv_p1_objects: dst[dir][i] = 0.5 (Hl + j Hr)[src], src = paired_to_natural(i & 63, i >> 6) -- the half of
// k_build_cd's sum that belongs to one channel, in k_irs_tables' permutation, without the 1/N (launch_conv_p1_objects applies it)
__global__ void k_object_tables(const float2 *__restrict__ H, int n_dirs, float2 *__restrict__ dst)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, dir = blockIdx.y;
    if (i >= kFft || dir >= n_dirs) return;
    const float2 *hl = H + (size_t)dir * 2 * kFft, *hr = hl + kFft;
    const int src = paired_to_natural(i & 63, i >> 6);
    dst[(size_t)dir * kFft + i] = make_float2(0.5f * (hl[src].x - hr[src].y), 0.5f * (hl[src].y + hr[src].x));
}
hipError_t launch_object_tables(const float2 *H, int n_dirs, float2 *dst, hipStream_t st)
{
    if (n_dirs <= 0 || n_dirs > 65535) return hipErrorInvalidValue;     // (grid.y; the host builds in slices)
    hipLaunchKernelGGL(k_object_tables, dim3(kFft / 256, (unsigned)n_dirs), dim3(256), 0, st, H, n_dirs, dst);
    return hipGetLastError();
}

// the objects kernel: launch_conv_p1_layout's checks and shape, plus the rows
hipError_t launch_conv_p1_objects(const ConvP1Args &args, const ConvObjectsArgs &l, hipStream_t st)
{
    ConvP1Args a = args;
    a.gain = args.gain * (1.0f / kLayoutTableScale);        // the inverse transform's 1/N: the direction table comes without it
    if (a.n_blocks <= 0 || a.n_streams <= 0 || a.chunks > a.n_blocks) return hipErrorInvalidValue;
    if (!(a.chunks == 1 || a.chunks == 2 || a.chunks == 4 || a.chunks == 8 || a.chunks == 16)) return hipErrorInvalidValue;
    if (a.xcd_n < 1 || a.xcd_n > 8 || a.xcd_lo < 0 || a.xcd_lo + a.xcd_n > 8) return hipErrorInvalidValue;
    if (!a.in || !a.out || !a.merged_in || !a.merged_out || a.merged_in == a.merged_out || !a.tw) return hipErrorInvalidValue;
    if (!l.ahalf || l.n_objects < 1 || l.n_objects > 64 || l.n_pairs != (l.n_objects + 1) / 2) return hipErrorInvalidValue;
    if (!l.idx || l.seg < 1 || l.stream < 0 || l.prev_stream < 0) return hipErrorInvalidValue;
    const size_t shmem = (kTabComplex + kLayoutWaves * kWaveLdsComplex) * sizeof(float2);
    static std::atomic<unsigned long long> lds_ok{0};
    hipError_t e = obj_allow_large_lds(reinterpret_cast<const void *>(k_conv_p1_objects), shmem, lds_ok);
    if (e != hipSuccess) return e;
    const long long waves = (long long)a.n_streams * a.chunks;
    const dim3 grid(xcd_grid((unsigned)((waves + kLayoutWaves - 1) / kLayoutWaves), a.xcd_n));
    hipLaunchKernelGGL(k_conv_p1_objects, grid, dim3(64 * kLayoutWaves), shmem, st, a, l);
    return hipGetLastError();
}

}  // namespace ohs
