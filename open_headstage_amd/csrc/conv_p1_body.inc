// conv_p1_body.inc -- the body of k_conv_p1 (conv_kernels.hip), included once per kernel that shares it:
//   k_conv_p1        OHS_P1_GAIN = A.gain, OHS_P1_BLOCK_GAIN(t) empty: the kernel as it has always been
//   k_conv_p1_gains  a gain per segment (ohs_batch_process_scheduled): OHS_P1_BLOCK_GAIN(t) reads the gain of block t's segment
//                    from A.gain_tab -- wave-uniform, one scalar load per block -- into the variable OHS_P1_GAIN names
//   k_conv_p1_irs    a set of impulse responses per segment and stream (ohs_batch_process_ir_scheduled): no (C, D) table in LDS;
//                    OHS_P1_BLOCK_BEGIN(t) reads the set index of block t's segment -- wave-uniform, one scalar load per block --,
//                    zeroes the incoming overlap at a run's first block in the CUT mode, and OHS_P1_PRODUCT takes (C, D) of that
//                    set from the device table I.cd
//   k_conv_p1_irs_xf the same with a crossfade (ohs_batch_process_ir_crossfaded): in the first block of a segment whose set differs
//                    from the one in front of it, OHS_P1_PRE_PRODUCT runs x * (512 - n) / 512 through the OLD set as a block of
//                    its own (head into tail[], tail kept for OHS_P1_BLOCK_END) and leaves x * n / 512 in v for the block
//                    that follows.  Every other block is k_conv_p1_irs's
// The hooks the includer defines: OHS_P1_TABLE(cd) fills the LDS table, OHS_P1_LOOP_INIT runs once in front of the block loop,
// OHS_P1_BLOCK_BEGIN(t) / OHS_P1_BLOCK_END at the loop's top and bottom, OHS_P1_PRE_PRODUCT(v, w) sits between the block's input
// (v filled, xl / xr still alive) and its forward transform, OHS_P1_PRODUCT(v, w) is the spectral product.
// Textual inclusion, so that the plain kernel's code does not depend on the other one's existence.
{
    const long long wg = p1_xcd_block(A);
    if (wg < 0) return;
    ohs_set_fp_mode(A.fp_mode);
    OHS_P1_STAMP_ENTRY();
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    float2 *tab = smem;
    float2 *cd = smem + kTabComplex;                    // [2][16][64]
    fill_twiddle_tables(tab, A.tw, threadIdx.x, 64 * kP1Waves);
    OHS_P1_TABLE(cd)
    __syncthreads();
    // wave-uniform quantities are forced into SGPRs: stream, chunk, block range and the four audio base
    // pointers then cost no VGPRs and the address arithmetic runs on the scalar unit
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    float2 *lds = smem + kTabComplex + 2 * kFft + wave * kWaveLdsComplex;
    const long long gw = wg * kP1Waves + wave;
    long long s64;
    int ck;
    p1_wave_job(gw, A.chunks, s64, ck);
    // A.own_tails: the wave computes the overlap entering its chunk itself -- one dry block in front of its range (b0 - 1,
    // nothing stored) instead of a boundary tail from the pre-pass.  In place that block's input is the LAST thing the
    // wave of chunk ck - 1 overwrites, so every wave of the workgroup (all chunks of a stream live in one workgroup in
    // these launches: launch_conv_p1) reads its first inputs in front of a barrier and stores behind it; waves without
    // work take part in the barrier too.
    bool active = s64 < (long long)A.n_streams;
    const int s = active ? (int)s64 : 0;
    const int n_main = A.n_blocks;        // every block's output is this kernel's
    const int b0 = __builtin_amdgcn_readfirstlane(p1_chunk_begin(s, ck, n_main, A.chunks, A.weights));
    const int b1 = __builtin_amdgcn_readfirstlane(p1_chunk_begin(s, ck + 1, n_main, A.chunks, A.weights));
    active = active && b0 < b1;
    if (!active) {
        if (A.own_tails) __syncthreads();
        return;
    }
    const bool own_tail = A.own_tails && ck > 0;
    const int t_first = own_tail ? b0 - 1 : b0;
    OHS_P1_STAMP_START();

    const float *in_l = A.in + (size_t)s * A.in_stream_stride;
    const float *in_r = in_l + A.in_ch_stride;
    float *out_l = A.out + (size_t)s * A.out_stream_stride;
    float *out_r = out_l + A.out_ch_stride;

    float2 tail[8];
    if (ck == 0 && A.merged_in) {
        const float2 *mt = A.merged_in + (size_t)s * (8 * 64);
#pragma unroll
        for (int a = 0; a < 8; ++a) tail[a] = mt[a * 64 + lane];
    } else if (ck == 0) {
        const float2 *tails = A.tails + (size_t)s * (2 * 8 * 64);
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const float2 t1 = tails[a * 64 + lane], t2 = tails[(8 + a) * 64 + lane];
            tail[a] = make_float2(t1.x + t2.x, t1.y + t2.y);
        }
    } else if (own_tail) {
#pragma unroll
        for (int a = 0; a < 8; ++a) tail[a] = make_float2(0.0f, 0.0f);
    } else {
        const float2 *ct = A.chunk_tails + ((size_t)s * A.chunks + ck) * (size_t)(8 * 64);
#pragma unroll
        for (int a = 0; a < 8; ++a) tail[a] = ct[a * 64 + lane];
    }
    // All waves of a workgroup leave the table barrier together and run the same program, so their LDS
    // bursts and their arithmetic phases coincide; a start offset per wave spreads them over the block time.
    for (int i = 0; i < wave * A.stagger; ++i) __builtin_amdgcn_s_sleep(1);
    // The next block's 16 input dwords are requested BEFORE this block's 16 stores are issued: vector-memory
    // operations retire in order, so loads issued after the stores (at the top of the next iteration) could not be
    // consumed before every one of those stores had been acknowledged.  (Requesting them a whole inverse
    // transform earlier would hide the HBM latency entirely, but needs 16 more VGPRs at the kernel's register
    // peak: hipcc spilled 80 VGPRs at 4 waves per SIMD and still 24 at 3.)
    float xl[8], xr[8];
    // one address per channel and direction, advanced by a block per iteration; every access is base + immediate
    const float *pl = in_l + (size_t)t_first * kBlock + lane, *pr = in_r + (size_t)t_first * kBlock + lane;
    float *ql = out_l + (size_t)t_first * kBlock + lane, *qr = out_r + (size_t)t_first * kBlock + lane;
#pragma unroll
    for (int a = 0; a < 8; ++a) { xl[a] = OHS_P1_LD(&pl[64 * a]); xr[a] = OHS_P1_LD(&pr[64 * a]); }
    if (A.own_tails) __syncthreads();       // (waits for the loads above: no wave has stored anything yet)
    // Issue arbitration between the four waves of a SIMD is "priority, then age": left alone, the oldest wave of
    // every SIMD runs almost unimpeded and the youngest gets the leftover slots -- waves 0..3 of a workgroup finished
    // their ranges after 156 us, waves 12..15 after 268 us (tools/p1_stamps.py), and a CU's slots stood empty for a
    // quarter of the launch, because the workgroup holds all of the CU's LDS until its last wave is done.  So the
    // priority rotates: in block k the wave of age rank g (wave >> 2) runs at priority (g + k) & 3, every wave gets
    // every level a quarter of the time and all sixteen finish together.
    const int age_rank = wave >> 2;
    int prio_phase = age_rank;
    const PairedPlan plan = paired_plan(lane);
    OHS_P1_LOOP_INIT
    for (int t = t_first; t < b1; ++t) {
        const bool dry = t < b0;            // the block in front of the range: its overlap is all that is wanted
        OHS_P1_BLOCK_BEGIN(t)
        if (A.prio_mode == 1) {
            switch (prio_phase & 3) {       // (s_setprio takes an immediate)
            case 0: __builtin_amdgcn_s_setprio(0); break;
            case 1: __builtin_amdgcn_s_setprio(1); break;
            case 2: __builtin_amdgcn_s_setprio(2); break;
            default: __builtin_amdgcn_s_setprio(3); break;
            }
            ++prio_phase;
        }
        if (A.last_in && t == A.n_blocks - 1) {     // lazy state: the launch's last block keeps a copy of its input
            float *li = A.last_in + (size_t)s * (2 * kBlock) + lane;
#pragma unroll
            for (int a = 0; a < 8; ++a) { li[64 * a] = xl[a]; li[kBlock + 64 * a] = xr[a]; }
        }
        float2 v[16];
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            v[a] = make_float2(xl[a], xr[a]);
            v[a + 8] = make_float2(0.0f, 0.0f);
        }
        float2 w[16];
        OHS_P1_PRE_PRODUCT(v, w)
        wave_fft_fwd_paired(v, lds, tab, lane, plan);
        OHS_P1_PRODUCT(v, w)
        // the prefetch of block t + 1 needs no guard except behind the launch's last block, where it re-reads that
        // block (its own frames: in bounds; the values are never used)
        const int adv = (t + 1 < A.n_blocks) ? kBlock : 0;
        pl += adv; pr += adv;
        wave_fft_inv_paired(w, lds, tab, lane, plan);
#pragma unroll
        for (int a = 0; a < 8; ++a) { xl[a] = OHS_P1_LD(&pl[64 * a]); xr[a] = OHS_P1_LD(&pr[64 * a]); }
        if (!dry) {
            OHS_P1_BLOCK_GAIN(t)
#pragma unroll
            for (int a = 0; a < 8; ++a) {
                OHS_P1_ST(&ql[64 * a], (w[a].x + tail[a].x) * OHS_P1_GAIN);         // (1/N is in C and D)
                OHS_P1_ST(&qr[64 * a], (w[a].y + tail[a].y) * OHS_P1_GAIN);
            }
        }
#pragma unroll
        for (int a = 0; a < 8; ++a) tail[a] = w[a + 8];
        ql += kBlock; qr += kBlock;
        OHS_P1_BLOCK_END
    }
    if (A.merged_out && b1 == A.n_blocks) {         // lazy state: the merged overlap the launch leaves behind
        float2 *mo = A.merged_out + (size_t)s * (8 * 64);
#pragma unroll
        for (int a = 0; a < 8; ++a) mo[a * 64 + lane] = tail[a];
    }
    OHS_P1_STAMP_END(gw, lane);
}
