// conv_objects_kernels.hip -- k_conv_p1_objects: K independently moving sources per stream -> two ears in one kernel, one direction
// per object (ohs_scene_process, include/ohs_scene.h; kernels.h: ConvObjectsArgs), and the direction table all three object kernels read.
//
// A sibling of k_conv_p1_layout_irs (conv_kernels.hip) in a translation unit of its own: with this kernel inside conv_kernels.hip
// hipcc allocated six of that file's other kernels differently (k_conv_p1 107 instead of 108 VGPRs, k_conv_p1_edges 103 instead of
// 115, ...), and the kernels every earlier measurement was taken on are to stay the code they were.  The helpers, the
// two-row pass and the launch are conv_objects_body.hpp's; the block loop below is this kernel's own.  What the build gives (hipcc, gfx950; libohs_hip.resources.json,
// DESIGN.md section 4.5h): 165 VGPRs of the 168 that three waves per SIMD leave, 86 SGPRs, no scratch -- with the load group of four
// as it is.
#include "conv_objects_body.hpp"

namespace ohs {

static_assert(kObjLdsPlanFits, "k_conv_p1_objects: LDS plan");

// The block loop of k_conv_p1_objects is its own, with the header's helpers, two-row pass and launch: out of the shared loop the
// kernel had the same register figures and all but 6 of its 3 146 opcodes, yet missed the speed rule in two benchmark sessions by
// 2 - 4 % at 16 to 48 objects; as it stands it is the instruction stream it was.  `old` is
// the previous segment's entry, the caller's prev_* in front of the call's first block, the block's own where there is none; an object
// changes when its index or its gain's bits differ from old.  Pass order, ramps, prefetch, tail and store: objects_block_loop's.
__global__ __launch_bounds__(64 * kObjWaves, kObjWavesPerSimd) void k_conv_p1_objects(const ConvP1Args A, const ConvObjectsArgs L)
{
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
            if (first) objects_pass_rows2<false>(v, w, ap, bp, lane);
            else objects_pass_rows2<true>(v, w, ap, bp, lane);
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

hipError_t launch_conv_p1_objects(const ConvP1Args &args, const ConvObjectsArgs &l, hipStream_t st)
{
    return launch_objects_kernel(k_conv_p1_objects, args, l, st);
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

}  // namespace ohs
