// check_eq_plan.cpp -- csrc/eq_plan.h alone (with tuning.h, whose Tuning it reads), for tests/test_cpu_eq_plan.py (built with
// -fsanitize=address,undefined; with and without -DOHS_EXPERIMENTS).
// stdin: native 32-bit integers, 17 per case:
//   one_table addressable n n_chains n_bands exact_specials xcd_lo xcd_n cus
//   eq_form eq_conveyor eq_wg_waves eq_ring_v1 eq_quad_fill eq_quad_lone_port eq_no_prio eq_lds
// stdout, one line per case: valid form body ring_v1 wg_waves grid prio lds
#include <cstdio>

#include "eq_plan.h"
#include "tuning.h"

int main()
{
    int w[17];
    while (std::fread(w, sizeof(int), 17, stdin) == 17) {
        ohs::Tuning tn;
        tn.eq_form = w[9]; tn.eq_conveyor = w[10]; tn.eq_wg_waves = w[11]; tn.eq_ring_v1 = w[12];
        tn.eq_quad_fill = w[13]; tn.eq_quad_lone_port = w[14]; tn.eq_no_prio = w[15]; tn.eq_lds = w[16];
        const ohs::EqPlan p = ohs::eq_plan(w[0] != 0, w[1] != 0, w[2], w[3], w[4], w[5] != 0, w[6], w[7], w[8], tn);
        std::printf("%d %d %d %d %d %u %d %d\n", p.valid, p.form, p.body, p.ring_v1, p.wg_waves, p.grid, p.prio, p.lds);
    }
    return std::ferror(stdin) || !std::feof(stdin) ? 2 : 0;
}
