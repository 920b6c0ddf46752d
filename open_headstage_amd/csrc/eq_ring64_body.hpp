// eq_ring64_body.hpp -- the ring-form DF2T cascade (<= 12 bands) with the ring closed over ALL 64 lanes of a wave: ONE
// chain per wave.  Device code of k_eq_ring's second form (eq_kernels.hip), chosen where the chip has a SIMD to spare
// for every chain (BASELINE configs[2]: 512 chains, 1 024 SIMDs).
// Every file that includes this header MUST be built with -ffp-contract=off (parametric_eq.rs:116-122: every product and
// sum of the recurrence rounds by itself).
//
// Why.  The ring form's time is its VALU instruction count: a lone wave issues one instruction per ~4.1 cycles whatever
// its lanes do.  In a 16-lane DPP row (eq_ring2_body.hpp) a chain has 10 bands + 6 pass-on lanes, and the
// I/O port -- capture 4 outputs, inject 4 inputs -- runs every 4 steps: 6 + 2 / 4 = 6.5 instructions per sample.  gfx950
// still executes gfx9's wave-wide DPP controls at the row controls' cost (wave_ror:1; tools/ubench_wave_dpp.hip,
// profiles/r05_ubench_wave_dpp.txt).  With the ring closed over the wave, lanes 13 .. 63 pass samples on, rows 1 .. 3
// are a conveyor of 48 samples, and the port -- one store, one inject move, one load (eq_ring64_groups) -- runs every 48 steps:
// 6 + 1 / 48 = 6.02 VALU instructions per sample (prototype: tools/proto_eq_wave_ring.py, 11.02 against 11.49 ns with the
// round-5 port of two moves).
//
// Lane roles and arithmetic are eq_ring2_body.hpp's (band L: pre lane L, post lane L + 1; O T A P N M per step), with
// wave_ror:1 where that form has row_ror:1.  What differs is how a launch starts and ends.  The same six instructions
// run on every lane from the first step to the last -- no step is gated.  Instead
//   head   the ring starts empty (X = 0, state = 0: a band that sees zeros in a zero state stays at zero), and band L's
//          state from the previous launch is put into its post lane behind step L + 1, the step in front of the one in
//          which its first sample arrives;
//   tail   band L's state is taken out of its post lane behind step n + L + 1, the step in which it filters sample
//          n - 1; the ring then runs on zeros until the last outputs have travelled into the conveyor and been stored.
// Timeline (steps count from 1; lane 63 - i of rows 1 .. 3 holds sample 48 g + i when group g is injected, behind step 48 g):
//   sample i is in lane 0 at step i + 1, filtered by band L (post lane L + 1) at step i + L + 2, whatever the number of
//   bands it reaches lane 16 + m at step i + 17 + m; the port behind step 48 (g + 1) finds sample 48 g + 47 - l in lane
//   l >= 16: outputs leave 16 samples behind the inputs that replace them.
//
// Coefficient boundaries inside a launch (the SCHED form: k_eq_ring_sched, ohs_batch_process_scheduled).  Sample B is the first
// one of a new table: every band takes five new constants and keeps s1, s2 (update_coefficients, parametric_eq.rs:85-114).
// The ring is systolic, so the boundary reaches the lanes one after the other.  Band L filters sample B in step B + L + 2 on
// its post lane L + 1 (O T A N); the P that feeds that step ran in step B + L + 1 on its pre lane L, the M in step B + L + 1 on
// lane L + 1.  Per lane l:
//   a1, a2    new from the A of step B + l + 1
//   pb0, pb1  new from the P of step B + l + 1
//   b2        new from the M of step B + l
// i.e. in step t lane t - B - 1 takes its new (pb0, pb1, a1, a2) in front of A, and lane t - B its new b2 in front of M.  Lane 0
// has no b2, so all of it happens in steps B + 1 .. B + 13, and with B a multiple of 512 (B mod 48 = 0, 16 or 32) these lie in
// ONE group, group B / 48, which runs in the C++ form; the groups around it run through eq_ring64_groups unchanged (its
// constants are asm inputs).  tools/model_eq_wave_ring.py is the lane-level CPU model that confirms the rule bit for bit
// against the oracle refreshed per segment (tests/test_cpu_schedule.py).  Segments are >= 512 samples: at most one boundary
// is in the ring at a time.  The next table's constants are requested in front of the asm run that leads up to the boundary.
#pragma once
#include "kernels.h"
#include "eq_ring2_body.hpp"    // v2f, dpp helpers, RingLane, ring2_ld / ring2_st

namespace ohs {

constexpr int kWaveRor1 = 0x13C;        // DPP_WF_RR1: lane l <- lane l - 1, lane 0 <- lane 63
constexpr int kR64Group = 48;           // samples per group = lanes of the conveyor

struct Ring64Regs {
    float X, st;        // v2, st: the C++ form's outgoing samples (the asm stores from X)
    v2f u;              // v[4:5]   (b0, b1) * X of the pre lane
    float b2x;          // v7       b2 * X(wave_ror:1) of the post lane
    v2f s;              // v[10:11] (s1, s2)
};

// rows 1 .. 3 of `src` into `old` (row 0 keeps `old`)
__device__ __forceinline__ float ring64_rows123(float old, float src)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), kQuadIdentity, 0xe, 0xf, false));
}

// P and M: what a step leaves behind for the next one
__device__ __forceinline__ void ring64_pm(Ring64Regs &r, const RingLane &c)
{
    r.u = (v2f){c.pb0 * r.X, c.pb1 * r.X};
    r.b2x = c.b2 * dpp_mov<kWaveRor1>(r.X, r.X);
}

// A raw buffer resource (V#) over `bytes` bytes from `base`: stride 0, no swizzle, DATA_FORMAT 32 (a gfx9 buffer with format 0
// is invalid).  Wave-uniform: it lives in four scalar registers.
typedef unsigned ring64_rsrc_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ ring64_rsrc_t ring64_rsrc(const void *base, unsigned bytes)
{
    const unsigned long long a = (unsigned long long)base;
    ring64_rsrc_t v;
    v.x = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)a);
    v.y = (unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned)(a >> 32) & 0xFFFFu));
    v.z = (unsigned)__builtin_amdgcn_readfirstlane((int)bytes);
    v.w = 0x00020000u;
    return v;
}

#define R64_FULL "row_mask:0xf bank_mask:0xf\n"
#define R64_O "v_add_f32_dpp v2, v4, v10 wave_ror:1 " R64_FULL
#define R64_T "v_add_f32_dpp v6, v5, v11 wave_ror:1 " R64_FULL
#define R64_A "v_pk_mul_f32 v[8:9], v[14:15], v[2:3] op_sel_hi:[1,0]\n"
#define R64_P "v_pk_mul_f32 v[4:5], v[12:13], v[2:3] op_sel_hi:[1,0]\n"
#define R64_N "v_pk_add_f32 v[10:11], v[6:7], v[8:9] neg_lo:[0,1] neg_hi:[0,1]\n"
#define R64_M "v_mul_f32_dpp v7, v2, v1 wave_ror:1 " R64_FULL
#define R64_STEP R64_O R64_T R64_A R64_P R64_N R64_M
#define R64_X2(B) B B
#define R64_X4(B) R64_X2(B) R64_X2(B)
#define R64_X8(B) R64_X4(B) R64_X4(B)
#define R64_X16(B) R64_X8(B) R64_X8(B)
#define R64_X32(B) R64_X16(B) R64_X16(B)
#define R64_STEPS47 R64_X32(R64_STEP) R64_X8(R64_STEP) R64_X4(R64_STEP) R64_X2(R64_STEP) R64_STEP

// The port of one group: 4 issue slots.  The 48 outputs in rows 1 .. 3 of X leave straight from X (buffer_store_dword: a
// store of 32 data bits needs no wait state before a VALU overwrites its data register -- only stores wider than 64 bits do,
// and the s_waitcnt is between them anyway), then v_cndmask (VCC = rows 1 .. 3) injects the input register REG into rows
// 1 .. 3, and REG is refilled three groups ahead.  Row 0 is kept out of the I/O by its offset, not by EXEC: v0 is
// 0xFFFFF000 there, beyond any launch's num_records, so its store is dropped and its load returns 0 (never injected: VCC).
// SOFF / LOFF: the group's store / load byte offsets from v0, which is this lane's store slot of the block's first group.
#define R64_PORT(REG, SOFF, LOFF) \
        "buffer_store_dword v2, v0, %[rout], 0 offen offset:" SOFF "\n" \
        "s_waitcnt vmcnt(3)\n" \
        "v_cndmask_b32_e32 v2, v2, " REG ", vcc\n" \
        "buffer_load_dword " REG ", v0, %[rin], 0 offen offset:" LOFF "\n"
// One interior group as asm text: 47 plain steps, the port step.  Group k (0 .. 3) of a block stores at 192 k and loads
// group k + 3 at 192 k + 640 (the store slot of lane l >= 16 is sample 48 g + 47 - l, its input slot 48 g + 63 - l).
#define R64_GROUP(REG, SOFF, LOFF) \
        R64_STEPS47 \
        R64_O R64_T R64_A \
        R64_PORT(REG, SOFF, LOFF) \
        R64_P R64_N R64_M
#define R64_GROUP0 R64_GROUP("v16", "0", "640")
#define R64_GROUP1 R64_GROUP("v17", "192", "832")
#define R64_GROUP2 R64_GROUP("v16", "384", "1024")
#define R64_GROUP3 R64_GROUP("v17", "576", "1216")

// `groups` >= 1 interior groups (1, 2, ...) in ONE statement: every sample they filter and store exists, no band starts or
// ends inside them.  The input register is double-buffered (v16: odd groups, v17: even ones): the port of group g injects
// group g + 1, requested at port g - 2, and requests group g + 3 into the register it has just emptied -- 96 steps =
// ~1.06 us between a load and its use (with one register and 48 steps the wave waited for memory at every port: the
// prototype, alone on the chip, 11.05 -> 10.88 ns per sample; profiles/r05_proto_eq_wave_ring_ahead.txt).  Behind a port's
// store the store and the load of each of the two previous ports may still be in flight: vmcnt(3) (they retire in issue
// order).
// The I/O goes through buffer resources over the launch's n samples of the chain (`rin` / `rout`, num_records = 4 n).  Raw
// buffer (stride 0) range check, gfx9 / CDNA MUBUF rule: an access is out of range when its offset -- VGPR offset plus the
// instruction's offset field; the scalar soffset is NOT part of the check, so it is 0 here -- is >= num_records; an
// out-of-range load returns 0, an out-of-range store is dropped.  So loads beyond the launch's last sample return 0, as in
// the C++ form, and row 0 (v0 = 0xFFFFF000 >= 4 n: eq_ring2_addressable keeps 4 n + 4096 below 2^32, and row 0's v0 never
// moves: `inc` is 0 there) neither stores nor loads anything.
// Loop: four groups per iteration, immediate offsets inside it, one v0 advance (v_add of `inc` = 768 bytes in rows 1 .. 3)
// and one counter step + branch; then a tail of groups % 4 groups (0 .. 3) that leaves where they end.  Issue slots per
// group beyond the 288 step instructions: (4 x 4 + 3) / 4 = 4.75 (before: 6.04 ... 11.5 per group: DESIGN 4.5).
// On entry: the first step's P and M have run (by the C++ form), v16 / v17 = the inputs of the two groups BEHIND the first
// one here, v0 = this lane's store slot of the first group; on exit `xnext` = the inputs of the group behind the next one.
// Every 8-byte encoding is 8-byte aligned (a lone wave pays for one that straddles a fetch line): the 4-byte instructions
// come in pairs (s_waitcnt + v_cndmask, s_add + s_cbranch, s_cmp + s_cbranch; v_add_u32 in its 8-byte VOP3 form).
__device__ __forceinline__ void eq_ring64_groups(const RingLane &c, Ring64Regs &r, float &xnext, float xnext2, unsigned lane_off,
                                                 unsigned inc, ring64_rsrc_t rin, ring64_rsrc_t rout, int groups)
{
    const v2f pb01 = {c.pb0, c.pb1}, a12 = {c.a1, c.a2};
    const unsigned ng = (unsigned)__builtin_amdgcn_readfirstlane(groups);
    unsigned cnt = 0u - (ng >> 2);                      // counts up to 0: s_add_u32's carry ends the loop
    const unsigned tail = ng & 3u;
    asm volatile(
        "s_mov_b32 vcc_lo, 0xffff0000\n"                // VCC = rows 1 .. 3 (the C++ form's last P and M are 2+ wait states
        "s_mov_b32 vcc_hi, -1\n"                        // behind by the first DPP read of v4)
        "s_cmp_eq_u32 %[cnt], 0\n"
        "s_cbranch_scc1 2f\n"
        ".p2align 5\n"
        "1:\n"
        R64_GROUP0 R64_GROUP1 R64_GROUP2 R64_GROUP3
        "v_add_u32_e64 v0, v0, v3\n"
        "s_add_u32 %[cnt], %[cnt], 1\n"
        "s_cbranch_scc0 1b\n"
        "2:\n"
        "s_cmp_eq_u32 %[tail], 0\n"
        "s_cbranch_scc1 3f\n"
        R64_GROUP0
        "s_cmp_eq_u32 %[tail], 1\n"
        "s_cbranch_scc1 3f\n"
        R64_GROUP1
        "s_cmp_eq_u32 %[tail], 2\n"
        "s_cbranch_scc1 3f\n"
        R64_GROUP2
        "3:\n"
        "s_waitcnt vmcnt(0)\n"
        "s_nop 1\n"
        : [X] "+{v2}"(r.X), [u] "+{v[4:5]}"(r.u), [b2x] "+{v7}"(r.b2x), [s] "+{v[10:11]}"(r.s),
          [voff] "+{v0}"(lane_off), [xa] "+{v16}"(xnext), [xb] "+{v17}"(xnext2), [cnt] "+s"(cnt)
        : [b2] "{v1}"(c.b2), [inc] "{v3}"(inc), [pb01] "{v[12:13]}"(pb01), [a12] "{v[14:15]}"(a12), [rin] "s"(rin),
          [rout] "s"(rout), [tail] "s"(tail)
        : "v6", "v8", "v9", "vcc", "memory", "scc");
    if (ng & 1u) xnext = xnext2;                        // (an odd number of groups ends on v16's turn: v17 holds the next)
}

// PER_STREAM: the chain's stream owns its bands (parametric_eq.rs:125-129) -- constants, state slots and the NUMBER of enabled
// bands come from stabs[chain / 2] (kernels.h: EqStreamTable) instead of the launch's one table.
// SCHED: the launch's table changes at segment boundaries (kernels.h: EqRingSched; the rule in the header comment).
// Both (k_eq_ring_sched_streams, ohs_batch_process_scheduled_streams): the chain's stream follows its OWN row of segment indices,
// sch->seg_tab + (chain >> 1) * idx_stride, and stabs holds one EqStreamTable per SCHEDULE TABLE: lane roles, band count and
// state slots are those of the table the row names for the launch's first sample (all tables the stream meets inside the launch
// have that table's enabled flags).  One chain per wave, so the row walk stays wave-uniform and every wave pays for its own
// boundaries only.
template <bool PER_STREAM, bool SCHED = false>
__device__ __forceinline__ void eq_ring64_wave_t(const float *in, float *out, long long stream_stride, long long ch_stride,
                                                 long long n, int n_chains, int nb_shared, const EqPassTable &tab,
                                                 const EqStreamTable *__restrict__ stabs, float *__restrict__ state, long long chain,
                                                 const EqRingSched *sch = nullptr, long long idx_stride = 0)
{
    constexpr int G = kR64Group;
    if (chain >= n_chains) return;
    const int lane = threadIdx.x & 63;
    const int n32 = (int)n;
    int nb = nb_shared;
    [[maybe_unused]] const unsigned *seg_row = nullptr;     // SCHED: the row of segment indices this wave follows
    if constexpr (SCHED) seg_row = sch->seg_tab;
    [[maybe_unused]] long long stab_i = chain >> 1;         // PER_STREAM: the stream's table, or (SCHED) its first schedule table
    if constexpr (PER_STREAM && SCHED) {
        seg_row += (chain >> 1) * idx_stride;
        stab_i = (unsigned)__builtin_amdgcn_readfirstlane((int)seg_row[sch->seg0]);
    }
    if constexpr (PER_STREAM) nb = stabs[stab_i].nb;
    const bool pre = lane < nb, band = lane >= 1 && lane <= nb;
    const int jb = band ? lane - 1 : 0, jp = pre ? lane : 0;
    RingLane c;
    int slot;
    if constexpr (PER_STREAM) {
        const EqStreamTable *T = stabs + stab_i;
        c.pb0 = pre ? T->b0[jp] : 1.0f;
        c.pb1 = pre ? T->b1[jp] : 0.0f;
        c.b2 = band ? T->b2[jb] : 0.0f;
        c.a1 = band ? T->a1[jb] : 0.0f;
        c.a2 = band ? T->a2[jb] : 0.0f;
        slot = T->slot[jb];
    } else {
        c.pb0 = pre ? tab.b0[jp] : 1.0f;
        c.pb1 = pre ? tab.b1[jp] : 0.0f;
        c.b2 = band ? tab.b2[jb] : 0.0f;
        c.a1 = band ? tab.a1[jb] : 0.0f;
        c.a2 = band ? tab.a2[jb] : 0.0f;
        slot = tab.slot[jb];
    }
    // wave-uniform bases + per-lane 32-bit byte offsets (rows 1 .. 3: lane 63 - i <-> sample i of a group)
    const long long base = (chain >> 1) * stream_stride + (chain & 1) * ch_stride;
    const float *src0 = in + base;
    float *dst0 = out + base;
    float *state0 = state + chain * (kEqStateSlots * 2);
    const unsigned state_off = (unsigned)(slot * 2) * 4u;
    const bool conv = lane >= 16;
    v2f s_init = {0.0f, 0.0f};
    if (band) { s_init.x = ring2_ld(state0, state_off); s_init.y = ring2_ld(state0, state_off + 4u); }
    v2f s_save = s_init;
    auto load_group = [&](int g) -> float {         // group g's inputs, zeros beyond n
        const int i = g * G + 63 - lane;
        return (conv && i < n32) ? ring2_ld(src0, (unsigned)i * 4u) : 0.0f;
    };
    Ring64Regs r;
    r.st = 0.0f; r.b2x = 0.0f; r.u = (v2f){0.0f, 0.0f}; r.s = (v2f){0.0f, 0.0f};
    const float x0 = load_group(0);
    float xnext = load_group(1);
    r.X = conv ? x0 : 0.0f;
    ring64_pm(r, c);
    // one group in the C++ form: the launch's first group (the bands' states arrive), its last ones (they leave; loads
    // and stores are checked against n)
    constexpr int kNoBoundary = 0x3fffffff;
    [[maybe_unused]] int bnd = kNoBoundary;         // SCHED: the boundary the group meets (its sample index), c_new its constants
    [[maybe_unused]] RingLane c_new = c;
    auto group_cpp = [&](int g) {
        auto step = [&](int k, bool port) {
            const int stp = g * G + k + 1;
            if constexpr (SCHED) {
                if (lane == stp - bnd - 1) { c.pb0 = c_new.pb0; c.pb1 = c_new.pb1; c.a1 = c_new.a1; c.a2 = c_new.a2; }
            }
            const float o = dpp_mov<kWaveRor1>(r.u.x, r.u.x) + r.s.x;           // O
            const float t2 = dpp_mov<kWaveRor1>(r.u.y, r.u.y) + r.s.y;          // T
            r.X = o;
            const v2f ao = {c.a1 * o, c.a2 * o};                                // A
            if (port) {
                r.st = ring64_rows123(r.st, r.X);
                r.X = ring64_rows123(r.X, xnext);
                const int yi = g * G + 47 - lane;
                if (conv && (unsigned)yi < (unsigned)n32) ring2_st(dst0, (unsigned)yi * 4u, r.st);
                xnext = load_group(g + 2);
            }
            const v2f sn = {t2 - ao.x, r.b2x - ao.y};                           // N (with the previous step's M)
            if constexpr (SCHED) {
                if (lane == stp - bnd) c.b2 = c_new.b2;
            }
            ring64_pm(r, c);                                                    // P, M
            r.s = sn;
            if (band && lane == stp) r.s = s_init;          // behind step L + 1: band L's first sample is next
            if (band && lane == stp - n32) s_save = r.s;    // behind step n + L + 1: band L has filtered sample n - 1
        };
#pragma unroll 1
        for (int k = 0; k < G - 1; ++k) step(k, false);
        step(G - 1, true);
    };
    const int g_total = (n32 + 16 + G - 1) / G;
    group_cpp(0);
    int g = 1;
    // groups 1 .. n / 48 - 1 in asm: every step filters existing samples (the last of them ends at step 48 (n / 48) <= n: the
    // first state leaves behind step n + 1), every store lands below n; the one or two groups behind them run in the C++ form
    const int n_full = n32 / G;
    if constexpr (SCHED) {
        // groups g .. g_end - 1 (1 <= g, g_end <= n_full) in asm; xnext holds group g + 1's inputs on entry and g_end + 1's on exit
        auto run_asm = [&](int g_end) {
            if (g_end <= g) return;
            const float xnext2 = load_group(g + 2);
            const unsigned bytes = (unsigned)n32 * 4u;
            eq_ring64_groups(c, r, xnext, xnext2, conv ? (unsigned)(g * G + 47 - lane) * 4u : 0xFFFFF000u, conv ? 4u * G * 4u : 0u,
                             ring64_rsrc(src0, bytes), ring64_rsrc(dst0, bytes), g_end - g);
            g = g_end;
        };
        // the launch starts off0 samples into segment seg0; segment seg0 + j starts at sample j * seg_len - off0
        const int n_segs = sch->n_segs, seg_len = sch->seg_len;
        unsigned cur = (unsigned)__builtin_amdgcn_readfirstlane((int)seg_row[sch->seg0]);
        int B = seg_len - sch->off0;
#pragma unroll 1
        for (int seg = sch->seg0 + 1; seg < n_segs && B < n32; ++seg, B += seg_len) {
            const unsigned t = (unsigned)__builtin_amdgcn_readfirstlane((int)seg_row[seg]);
            if (t == cur) continue;             // (consecutive segments with one table are one run)
            cur = t;
            const int gb = B / G;               // the group of steps B + 1 .. B + 13
            if (gb < g || gb + 1 > n_full) continue;    // (never: boundaries are multiples of 512 in [512, n - 512])
            if (lane < 16) {                    // requested here, needed behind the asm run
                const float *lt = sch->lane_tabs + (size_t)t * (5 * 16) + lane;
                c_new.pb0 = lt[0]; c_new.pb1 = lt[16]; c_new.b2 = lt[32]; c_new.a1 = lt[48]; c_new.a2 = lt[64];
            }
            run_asm(gb);
            bnd = B;
            group_cpp(gb);
            bnd = kNoBoundary;
            c = c_new;
            g = gb + 1;
        }
        run_asm(n_full);
    } else if (n_full >= 2) {
        const float xnext2 = load_group(3);         // (zeros beyond n)
        const unsigned bytes = (unsigned)n32 * 4u;
        eq_ring64_groups(c, r, xnext, xnext2, conv ? (unsigned)(G + 47 - lane) * 4u : 0xFFFFF000u, conv ? 4u * G * 4u : 0u,
                         ring64_rsrc(src0, bytes), ring64_rsrc(dst0, bytes), n_full - 1);
        g = n_full;
    }
    for (; g < g_total; ++g) group_cpp(g);
    if (band) {
        ring2_st(state0, state_off, s_save.x);
        ring2_st(state0, state_off + 4u, s_save.y);
    }
}

// the shared-table form
__device__ __forceinline__ void eq_ring64_wave(const float *in, float *out, long long stream_stride, long long ch_stride,
                                               long long n, int n_chains, int nb, const EqPassTable &tab,
                                               float *__restrict__ state, long long chain)
{
    eq_ring64_wave_t<false>(in, out, stream_stride, ch_stride, n, n_chains, nb, tab, nullptr, state, chain);
}

}  // namespace ohs
