// eq_quad_ring_body.hpp -- the wave ring (one chain per wave, <= 12 bands) with ONE BAND PER QUAD of lanes: four VOP2+DPP
// instructions per sample instead of the six of eq_ring64_body.hpp.  Device code of k_eq_ring's third form (eq_kernels.hip),
// shared table only.
// Every file that includes this header MUST be built with -ffp-contract=off (parametric_eq.rs:116-122: every product and
// sum of the recurrence rounds by itself).
//
// tools/model_eq_quad_ring.py is the lane-level model and the specification (bit-exact against the oracle:
// tests/test_cpu_eq_quad_ring.py); its header comment has the step, the timeline and the port.  In short: band k owns lanes
// 4k .. 4k+3 = (a, b, c, d) with C1 = (1, 1, a2, a1), C2 = (b2, b1, b0, 1); every other quad passes samples on with
// C1 = (1, 1, 0, 0), C2 = (0, 0, 1, 1); quads 12 .. 15 are the conveyor the port serves.  A step, Zc = Z[step & 1]:
//     alpha  Zc = Zp(wave_ror:1) + G            delta  Zp = Zo(quad_perm 0,0,0,3) * C2       <one free issue slot>
//     beta   P  = Zc(quad_perm 0,0,3,3) * C1    gamma  G  = Zc(quad_perm 0,0,1,2) - P
// s1 lives in G of lane d, s2 in G of lane c.  A lane that has nothing to compute in an instruction is an exact identity by
// its constant (1.0 v, v + 0, v - 1.0 v = 0).  Sample i is in lane a of quad q at step i + 1 + 4q, in its lane d at step
// i + 3 + 4q; the ring is 64 steps round and outputs leave 64 samples behind the inputs that replace them.
//
// The free slot: gfx9 / CDNA need two wait states between a VALU write of a VGPR and a DPP read of it, and beta reads what
// alpha wrote.  The slot carries the port (a group = 16 steps: two stores, two injects, one load, one wait), so the steady
// state is 81 issue slots per 16 samples -- 5.06 per sample against 6.02 + 4.75 / 48.  The loop is generated from the model's
// own instruction list (tools/gen_eq_quad_ring_asm.py -> eq_quad_ring_asm.inc), which also checks every DPP read's distance.
// Where the port's memory instructions issue is what the loop's time above 4 ticks per slot is made of: each of the three,
// alone between VALU instructions, costs the wave about 8 ticks beyond its slot, one directly behind another about none
// (without them the loop runs at 20.41 ticks per sample, with them at 21.91).  Round 15's loop
// (eq_quad_ring_cl_asm.inc, the model's port variant C2; kQuadLoopCluster, experiments build, Tuning::eq_quad_cluster_port)
// parks step 8's value in a holding register (v20, a plain v_mov in that step's slot) and issues store, store, load back
// to back in step 15's slot: 83 slots per 16 samples at 21.44 ticks per sample.  The loop the kernel runs
// (eq_quad_ring_mg_asm.inc, the model's variant D1W; round 17) pays per memory instruction, not per byte, so it stores once
// per group: step 10's slot moves the parked value's lanes a, d to lanes b, c (v_mov_b32_dpp quad_perm:[0,0,3,3] on v20),
// step 15's merges Zc's lanes a, d in (v_cndmask_b32_e64 under a constant SGPR-pair mask: a plain read of Zc, VCC stays
// the injects'), and ONE store carries the group's 16 outputs -- lanes b, c with the offsets of lanes a, d seven samples
// earlier.  Store and load issue in the next group's step-1 slot behind the group's wait (s_waitcnt, s_nop: step 14's
// slot holds a v_nop instead), in an iteration's last group in its own step 16 behind inject A: no holding register is
// live across the end of an iteration.  21.01 ticks per sample.  Same ring, same lanes, same addresses, same bits; stores
// and the load only issue later than they did, so in place a store still never passes the load of its sample.
// kQuadLoopLone (experiments build, Tuning::eq_quad_lone_port) is the loop of round 12 with the three alone in the slots
// of steps 8, 10 and 15.
// A slot with nothing to carry holds a v_nop.  kQuadLoopFill (experiments build, Tuning::eq_quad_fill) is round 12's loop with a fill
// instruction there, v_and_b32_dpp on v19 (a register nothing else touches), which keeps the vector unit for the four
// cycles a step instruction takes instead of leaving them to a convolution wave of the same SIMD: a tie -- the loop runs at
// the lone prototype's 21.9 ticks per sample with or without the convolution underneath.
//
// A launch: groups -1 .. 4 at least in the C++ form of the same step (the ring starts at zero one group early; band k's
// state goes into G of its lanes c, d behind step 4k + 2), then whole iterations of K groups in asm while every step
// filters existing samples, then the C++ form again (band k's state leaves behind step n + 4k + 2, the ring runs on zeros
// until the last output is stored).  The C++ form checks every load and store against n; the asm goes through buffer
// resources over the chain's n samples (eq_ring64_body.hpp: out-of-range lanes neither store nor load).  A launch has 11 to
// 18 groups in the C++ form and a batch step six launches, so that form is written to compile to the loop's own four
// VOP2+DPP instructions per step (quad_dpp, group_cpp below).
#pragma once
#include "kernels.h"
#include "eq_ring64_body.hpp"   // kWaveRor1, ring64_rsrc, ring2_ld / ring2_st, dpp_mov
#include "eq_quad_ring_asm.inc"
#include "eq_quad_ring_cl_asm.inc"
#include "eq_quad_ring_mg_asm.inc"
#include <type_traits>

namespace ohs {

constexpr int kQuadGroup = 16;          // steps = samples per group
constexpr int kQuadK = EQ_QUAD_RING_K;  // groups per asm iteration = input registers in rotation
constexpr int kQp0003 = 0xC0, kQp0033 = 0xF0, kQp0012 = 0x90, kQp0101 = 0x44;

struct QuadRegs { float Z0, Z1, Zp, G, P; };
// the asm run's loop: one merged store and one load per group (the product's), or -- experiments build -- round 15's with
// store, store, load in one cluster per group, or round 12's with each of them alone in its slot, without or with the fill
// instruction in the slots that carry nothing
enum { kQuadLoopMerged, kQuadLoopCluster, kQuadLoopLone, kQuadLoopFill };

// A DPP read for the C++ form of the step.  Every control of the step (wave_ror:1, the quad_perms) gives every lane a source
// lane, so bound_ctrl changes no value; with it the compiler folds the move into the VOP2 instruction that consumes it --
// v_add_f32_dpp and so on, the loop's own four instructions -- where dpp_mov (eq_ring_body.hpp) leaves a v_mov_b32_dpp in
// front of each.
template <int CTRL>
__device__ __forceinline__ float quad_dpp(float src)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(src), CTRL, 0xf, 0xf, true));
}

template <int LOOP = kQuadLoopMerged>
__device__ __forceinline__ void eq_quad_ring_wave(const float *in, float *out, long long stream_stride, long long ch_stride,
                                                  long long n, int n_chains, int nb, const EqPassTable &tab,
                                                  float *__restrict__ state, long long chain)
{
    constexpr int G = kQuadGroup, K = kQuadK;
    static_assert(K == 8, "the operand list below names x0 .. x7");
    static_assert(EQ_QUAD_RING_CL_HOLD == 1 && EQ_QUAD_RING_MG_HOLD == 1, "the clobber lists below name one holding register, v20");
    static_assert(EQ_QUAD_RING_MG_PAIRS == 0, "the operand list below is that of one load and one store per group");
    if (chain >= n_chains) return;
    const int lane = threadIdx.x & 63, q = lane >> 2, role = lane & 3;
    const int n32 = (int)n;
    const bool band = q < nb, conv = q >= 12;
    const int j = band ? q : 0;
    const float C1 = role < 2 ? 1.0f : !band ? 0.0f : role == 2 ? tab.a2[j] : tab.a1[j];
    const float C2 = !band ? (role < 2 ? 0.0f : 1.0f) : role == 0 ? tab.b2[j] : role == 1 ? tab.b1[j] : role == 2 ? tab.b0[j] : 1.0f;
    const long long base = (chain >> 1) * stream_stride + (chain & 1) * ch_stride;
    const float *src0 = in + base;
    float *dst0 = out + base;
    float *state0 = state + chain * (kEqStateSlots * 2);
    // lane d holds s1, lane c holds s2
    const bool st_band = band && role >= 2;
    const unsigned state_off = (unsigned)(tab.slot[j] * 2 + (role == 2 ? 1 : 0)) * 4u;
    const float s_init = st_band ? ring2_ld(state0, state_off) : 0.0f;
    float s_save = s_init;
    const int t_in = 4 * q + 2;                 // behind this step the band's state goes in; behind n + t_in it comes out
    // the x register of group g holds, in conveyor quad q, (a, b, c, d) = samples 16 g + (71, 69, 62, 60) - 4 q;
    // a store at step m finds sample m - 1 - 4 q in lane a and m - 3 - 4 q in lane d of Zc
    const int xs = (role == 0 ? 71 : role == 1 ? 69 : role == 2 ? 62 : 60) - 4 * q;
    const int ss = (role == 0 ? -1 : -3) - 4 * q;
    const bool st_lane = conv && (role == 0 || role == 3), inj_lane = conv && role >= 2;
    auto load_x = [&](int g) -> float {         // zeros where the sample does not exist
        const int i = g * G + xs;
        return (conv && (unsigned)i < (unsigned)n32) ? ring2_ld(src0, (unsigned)i * 4u) : 0.0f;
    };
    QuadRegs r = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float xcur = load_x(-1), xnext = load_x(0);

    // the asm run: groups g0 .. g1 - 1, whole iterations, g0 >= 5 (every store offset of the run is >= 0), the last step
    // 16 g1 <= n + 1 (the first state leaves behind step n + 2)
    const int g_hi = (n32 + 1) / G;
    const int iters = g_hi - 5 >= K ? (g_hi - 5) / K : 0;
    const int g1 = iters ? g_hi : -1, g0 = iters ? g_hi - iters * K : -1;
    // the inputs of groups g0 + 2 .. g0 + 7, requested here: they are long there when the head has run (g0, g0 + 1: the head's)
    float x2 = 0.0f, x3 = 0.0f, x4 = 0.0f, x5 = 0.0f, x6 = 0.0f, x7 = 0.0f;
    if (iters) {
        x2 = load_x(g0 + 2); x3 = load_x(g0 + 3); x4 = load_x(g0 + 4);
        x5 = load_x(g0 + 5); x6 = load_x(g0 + 6); x7 = load_x(g0 + 7);
    }

    // one group in the C++ form; (xcur, xnext) = the inputs of groups (g, g + 1) on entry, of (g + 1, g + 2) on exit: a
    // request has a whole group's steps to arrive
    // The port's steps are known when the code is written (8 and 15 store, 9 and 16 inject), so the step takes its kind as a
    // constant and a group is written out around them: the plain steps in between carry no test of s and no branch, and a
    // group that no band's state enters or leaves (STATE false) no test of the step number either.  (With s tested at run
    // time in every step a group cost ~4 300 ticks against the loop's 350: 11 to 18 such groups per launch were ~27 us of
    // each of a step's six launches -- DESIGN.md 4.5, round 12.)
    enum { kPlain, kStore, kInjectB, kInjectA };
    auto group_cpp = [&](int g, auto with_state) {
        constexpr bool STATE = decltype(with_state)::value;
        const float xnext2 = load_x(g + 2);
        auto step = [&](auto kind, float &zc, const float zo, int s) {
            const int stp = g * G + s;
            zc = quad_dpp<kWaveRor1>(r.Zp) + r.G;                               // alpha
            r.Zp = quad_dpp<kQp0003>(zo) * C2;                                  // delta
            if constexpr (kind() == kStore) {                                   // the slot: the port
                const int yi = stp + ss;
                if (st_lane && (unsigned)yi < (unsigned)n32) ring2_st(dst0, (unsigned)yi * 4u, zc);
            } else if constexpr (kind() == kInjectB) {
                const float xb = quad_dpp<kQp0101>(xcur);
                r.Zp = inj_lane ? xb : r.Zp;
            } else if constexpr (kind() == kInjectA) {
                r.Zp = inj_lane ? xnext : r.Zp;
            }
            r.P = quad_dpp<kQp0033>(zc) * C1;                                   // beta
            r.G = quad_dpp<kQp0012>(zc) - r.P;                                  // gamma
            if constexpr (STATE) {
                r.G = (st_band && stp == t_in) ? s_init : r.G;
                s_save = (st_band && stp == n32 + t_in) ? r.G : s_save;
            }
        };
        using Plain = std::integral_constant<int, kPlain>;
        auto plain_pairs = [&](int s0, int s1) {       // steps s0 .. s1, s0 odd, s1 even
#pragma unroll 1
            for (int s = s0; s < s1; s += 2) {
                step(Plain{}, r.Z1, r.Z0, s);
                step(Plain{}, r.Z0, r.Z1, s + 1);
            }
        };
        plain_pairs(1, 6);
        step(Plain{}, r.Z1, r.Z0, 7);
        step(std::integral_constant<int, kStore>{}, r.Z0, r.Z1, 8);
        step(std::integral_constant<int, kInjectB>{}, r.Z1, r.Z0, 9);
        step(Plain{}, r.Z0, r.Z1, 10);
        plain_pairs(11, 14);
        step(std::integral_constant<int, kStore>{}, r.Z1, r.Z0, 15);
        step(std::integral_constant<int, kInjectA>{}, r.Z0, r.Z1, 16);
        xcur = xnext;
        xnext = xnext2;
    };

    const int g_total = (n32 + 62 + G - 1) / G;         // groups -1 .. g_total - 1 (the model's n_groups)
    int g = -1;
    const int head_end = iters ? g0 : g_total;
    // a band's state goes in behind step 4k + 2 <= 46 (groups 0 .. 2) and comes out behind step n + 4k + 2, which lies behind
    // the asm run where there is one (16 g1 <= n + 1): with a run, the head's groups 3 .. g0 - 1 touch no state
#pragma unroll 1
    for (; g < head_end && (g < 3 || !iters); ++g) group_cpp(g, std::true_type{});
#pragma unroll 1
    for (; g < head_end; ++g) group_cpp(g, std::false_type{});
    if (iters) {
        const unsigned bytes = (unsigned)n32 * 4u;
        const ring64_rsrc_t rin = ring64_rsrc(src0, bytes), rout = ring64_rsrc(dst0, bytes);
        // v0: the store of step 16 (g0 - 1) + 8; v1: group g0's inputs
        // (the merged loop: v0 holds an offset in all 16 lanes of the conveyor -- every store carries the offset of its
        // group's step 15, 28 bytes on; lanes b, c store what lanes a, d held at step 8: samples -8 - 4q and -10 - 4q from there)
        constexpr bool kMerged = LOOP == kQuadLoopMerged;
        const int ms = (role == 0 ? -1 : role == 1 ? -8 : role == 2 ? -10 : -3) - 4 * q;
        unsigned voff_st = kMerged ? (conv ? (unsigned)(G * (g0 - 1) + 15 + ms) * 4u - 28u : 0xFFFFF000u)
                                   : (st_lane ? (unsigned)(G * (g0 - 1) + 8 + ss) * 4u : 0xFFFFF000u);
        unsigned voff_ld = conv ? (unsigned)(G * g0 + xs) * 4u : 0xFFFFF000u;
        const unsigned inc_ld = conv ? 4u * G * K : 0u, inc_st = (kMerged ? conv : st_lane) ? 4u * G * K : 0u;
        unsigned cnt = 0u - (unsigned)__builtin_amdgcn_readfirstlane(iters);
#ifdef OHS_EXPERIMENTS
        if constexpr (LOOP == kQuadLoopFill) {
            unsigned fill = 0u;     // the fill's own register: F & F, whatever it holds
            asm volatile(
                "s_nop 4\n"
                EQ_QUAD_RING_LOOP_FILL
                : [Z0] "+{v2}"(r.Z0), [Z1] "+{v3}"(r.Z1), [Zp] "+{v4}"(r.Zp), [Gr] "+{v5}"(r.G), [P] "+{v6}"(r.P),
                  [vs] "+{v0}"(voff_st), [vl] "+{v1}"(voff_ld), [x0] "+{v11}"(xcur), [x1] "+{v12}"(xnext), [x2] "+{v13}"(x2),
                  [x3] "+{v14}"(x3), [x4] "+{v15}"(x4), [x5] "+{v16}"(x5), [x6] "+{v17}"(x6), [x7] "+{v18}"(x7),
                  [F] "+{v19}"(fill), [cnt] "+s"(cnt)
                : [C1] "{v7}"(C1), [C2] "{v8}"(C2), [incl] "{v9}"(inc_ld), [incs] "{v10}"(inc_st), [rin] "s"(rin), [rout] "s"(rout)
                : "memory", "scc", "vcc");
        } else if constexpr (LOOP == kQuadLoopLone) {
            asm volatile(
                "s_nop 4\n"
                EQ_QUAD_RING_LOOP
                : [Z0] "+{v2}"(r.Z0), [Z1] "+{v3}"(r.Z1), [Zp] "+{v4}"(r.Zp), [Gr] "+{v5}"(r.G), [P] "+{v6}"(r.P),
                  [vs] "+{v0}"(voff_st), [vl] "+{v1}"(voff_ld), [x0] "+{v11}"(xcur), [x1] "+{v12}"(xnext), [x2] "+{v13}"(x2),
                  [x3] "+{v14}"(x3), [x4] "+{v15}"(x4), [x5] "+{v16}"(x5), [x6] "+{v17}"(x6), [x7] "+{v18}"(x7), [cnt] "+s"(cnt)
                : [C1] "{v7}"(C1), [C2] "{v8}"(C2), [incl] "{v9}"(inc_ld), [incs] "{v10}"(inc_st), [rin] "s"(rin), [rout] "s"(rout)
                : "memory", "scc", "vcc");
        } else if constexpr (LOOP == kQuadLoopCluster) {
            asm volatile(
                "s_nop 4\n"
                EQ_QUAD_RING_CL_LOOP
                : [Z0] "+{v2}"(r.Z0), [Z1] "+{v3}"(r.Z1), [Zp] "+{v4}"(r.Zp), [Gr] "+{v5}"(r.G), [P] "+{v6}"(r.P),
                  [vs] "+{v0}"(voff_st), [vl] "+{v1}"(voff_ld), [x0] "+{v11}"(xcur), [x1] "+{v12}"(xnext), [x2] "+{v13}"(x2),
                  [x3] "+{v14}"(x3), [x4] "+{v15}"(x4), [x5] "+{v16}"(x5), [x6] "+{v17}"(x6), [x7] "+{v18}"(x7), [cnt] "+s"(cnt)
                : [C1] "{v7}"(C1), [C2] "{v8}"(C2), [incl] "{v9}"(inc_ld), [incs] "{v10}"(inc_st), [rin] "s"(rin), [rout] "s"(rout)
                : "memory", "scc", "vcc", "v20");
        } else
#endif
        {
            static_assert(LOOP == kQuadLoopMerged, "the product library has the merged loop only");
            // (v20: the holding register, written and read inside the loop only -- v19 is left to the fill; mk: lanes a, d of
            // every quad, where the merge takes Zc)
            const unsigned long long mk = 0x9999999999999999ull;
            asm volatile(
                "s_nop 4\n"
                EQ_QUAD_RING_MG_LOOP
                : [Z0] "+{v2}"(r.Z0), [Z1] "+{v3}"(r.Z1), [Zp] "+{v4}"(r.Zp), [Gr] "+{v5}"(r.G), [P] "+{v6}"(r.P),
                  [vs] "+{v0}"(voff_st), [vl] "+{v1}"(voff_ld), [x0] "+{v11}"(xcur), [x1] "+{v12}"(xnext), [x2] "+{v13}"(x2),
                  [x3] "+{v14}"(x3), [x4] "+{v15}"(x4), [x5] "+{v16}"(x5), [x6] "+{v17}"(x6), [x7] "+{v18}"(x7), [cnt] "+s"(cnt)
                : [C1] "{v7}"(C1), [C2] "{v8}"(C2), [incl] "{v9}"(inc_ld), [incs] "{v10}"(inc_st), [rin] "s"(rin), [rout] "s"(rout),
                  [mk] "s"(mk)
                : "memory", "scc", "vcc", "v20");
        }
        // (x0, x1 now hold the inputs of groups g1, g1 + 1: the run's last inject A took x0, group g1's inject B is next)
        g = g1;
#pragma unroll 1
        for (; g < g_total; ++g) group_cpp(g, std::true_type{});
    }
    if (st_band) ring2_st(state0, state_off, s_save);
}

}  // namespace ohs
