// eq_plan.h -- the ONE rule of the EQ launch layer: which form serves a launch, with which wave body, in workgroups of how many
// waves, on a grid of what size.  Every launcher of eq_kernels.hip and eq_pass_takes_wave_ring ask eq_plan(); nothing else
// decides.  Host code only, no HIP: tools/check_eq_plan.cpp builds it alone (tests/test_cpu_eq_plan.py).
#pragma once

#include "../../include/ohs_hip.h"      // OHS_EQ_FORM_*
#include "tuning.h"

namespace ohs {

// XCD partition of a launch.  The dispatcher hands workgroup b of a grid to XCD b % 8 (MI355X: 8 XCDs of 32 CUs, each
// with its own L2); a kernel confined to the XCDs [lo, lo + n) is launched with xcd_grid(workgroups, n) workgroups, those
// on other XCDs return at once and the rest renumber themselves ((b >> 3) * n + (b & 7) - lo).  ohs_batch_process gives
// the EQ and the overlapped convolution disjoint XCD sets: an EQ wave saturates the vector unit of its SIMD, and a
// convolution workgroup that shares a CU with one waits for its starved waves (LABNOTES.md, "What sharing a CU is worth").
inline unsigned xcd_grid(unsigned workgroups, int xcd_n)
{
    return xcd_n == 8 ? workgroups : ((workgroups + (unsigned)xcd_n - 1) / (unsigned)xcd_n) * 8u;
}

struct EqPlan {
    bool valid = false;             // false: the launcher returns hipErrorInvalidValue (form stays NONE)
    int form = OHS_EQ_FORM_NONE;    // NONE with valid: nothing to launch, the events still mark this point of the stream
    int body = 0;                   // the ring kernels' `wave_ring` argument: 0 = four chains per wave in 16-lane rows; one chain
                                    // per wave: 1 = a band per pair of lanes, 2 = per quad (the experiments build: 3 = the quad
                                    // body's fill loop, 4 = its lone-port loop, 5 = its cluster-port loop)
    bool ring_v1 = false;           // the experiments build's k_eq_ring_v1: no XCD partition, events around the launch
    int wg_waves = 1;               // waves per workgroup
    unsigned grid = 0;              // workgroups
    int prio = 0;                   // the ring kernels raise their waves' priority
    int lds = 0;                    // LDS reserved per workgroup of a ring kernel, bytes
};

// one_table: launch_eq_pass and the scheduled launchers (one EqPassTable of n_bands bands for all chains); else
// launch_eq_ring_streams (a table per stream in device memory: ring forms only, no band count, chains in pairs -- n_bands and
// exact_specials are not looked at, and neither are eq_conveyor and eq_ring_v1).
// addressable: eq_ring_addressable() of the launch's strides and n.  cus: the device's compute units.
//
// The conveyor form (k_eq_pass, one wave of four chains per workgroup) serves what the ring forms cannot: more than 12 bands,
// the exact-specials mode, strides beyond 32-bit offsets.  Of the ring forms the wave-wide one (one chain per wave: 5.06
// instead of 6.5 issue slots per sample) is taken where it pays: every chain needs a SIMD of its own, and the convolution
// that runs underneath needs issue slots too -- up to TWO chains per CU (BASELINE configs[2]: 512 chains on 256 CUs) the
// batch step is 2.8 - 3.4 % shorter, at 2.5 per CU it is a tie, at 3 per CU 1.2 % longer, and at 4 per CU (every SIMD taken)
// the convolution starves: 13.4 against 5.6 ms (profiles/r05_ab_eq_form.jsonl).  Calls under 8192 samples, too short for
// their first and last groups (which run in the C++ form) not to matter, keep four chains per wave.  Its body is one band
// per quad of lanes; the experiments build's eq_form = 3 forces that, eq_form = 2 the body with one band per pair of lanes
// (with per-stream tables the wave ring has the pair body only), eq_form = 1 the rows.
// Workgroups: the wave ring one wave each.  The rows, few chains (headline: 128 waves): one wave per workgroup, i.e. per CU
// -- alone on its CU a wave runs 2-3 % faster than next to three others.  From one wave per CU upwards: four per workgroup,
// so that the EQ fills whole CUs and leaves the others entirely to the overlapped convolution, whose 14-wave workgroups
// otherwise wait for their slowest wave on every CU (512 streams: 7.28 -> 6.38 ms per step, 1024 streams: 8.62 -> 7.62 ms).
inline EqPlan eq_plan(bool one_table, bool addressable, long long n, int n_chains, int n_bands, bool exact_specials, int xcd_lo,
                      int xcd_n, int cus, const Tuning &tn)
{
    EqPlan p;
    if (n <= 0 || n_chains <= 0) { p.valid = true; return p; }
    if (one_table ? (n_bands < 1 || n_bands > 16) : ((n_chains & 1) || !addressable)) return p;
    bool ring_v1 = false;
#ifdef OHS_EXPERIMENTS
    ring_v1 = one_table && tn.eq_ring_v1 != 0;
#endif
    const int blocks = (n_chains + 3) / 4;          // waves of four chains
    if (one_table && (n_bands > 12 || tn.eq_conveyor || exact_specials || !(ring_v1 || addressable))) {
        p.valid = true;
        p.form = OHS_EQ_FORM_CONVEYOR;
        p.grid = (unsigned)blocks;
        return p;
    }
    const bool wave_ring = !ring_v1 && (tn.eq_form == 2 || tn.eq_form == 3 || (tn.eq_form == 0 && n_chains <= 2 * cus && n >= 8192));
    const int waves = wave_ring ? n_chains : blocks;
    const int wg_override = (ring_v1 && tn.eq_wg_waves > 4) ? 0 : tn.eq_wg_waves;
    p.wg_waves = wg_override ? wg_override : (wave_ring ? 1 : (blocks >= cus ? 4 : 1));
    const unsigned workgroups = (unsigned)((waves + p.wg_waves - 1) / p.wg_waves);
    p.ring_v1 = ring_v1;
    if (ring_v1) {
        p.grid = workgroups;
    } else {
        if (xcd_n < 1 || xcd_n > 8 || xcd_lo < 0 || xcd_lo + xcd_n > 8) return EqPlan();
        p.grid = xcd_grid(workgroups, xcd_n);
        p.prio = tn.eq_no_prio ? 0 : 1;
        p.lds = tn.eq_lds;
#ifdef OHS_EXPERIMENTS
        p.body = !wave_ring ? 0 : (!one_table || tn.eq_form == 2) ? 1 : tn.eq_quad_fill ? 3 : tn.eq_quad_lone_port ? 4 :
                 tn.eq_quad_cluster_port ? 5 : 2;
#else
        p.body = !wave_ring ? 0 : (!one_table || tn.eq_form == 2) ? 1 : 2;
#endif
    }
    p.valid = true;
    p.form = wave_ring ? OHS_EQ_FORM_WAVE_RING : OHS_EQ_FORM_ROW_RING;
    return p;
}

}  // namespace ohs
