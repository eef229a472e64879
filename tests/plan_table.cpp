// plan_table.cpp -- prints the projector's split plan (csrc/vp_plan.h) for the calls listed on standard input; built and run by
// tests/test_plan_cpu.py with the host compiler, once plain and once with -fsanitize=address,undefined.
// Input, one call per line:   B V H W C serial_sums opt_heavy_t opt_part_px opt_one_view opt_one_view_split
// Output, one line per call:  slot_cap host_heavy_t  heavy_t part_t part_px count_heavy dyn_px_min dyn_t_ratio dyn_t_floor cell_in_item
//                             one_view one_split plans_parts
#include <cstdio>

#include "vp_plan.h"

int main()
{
    PlanIn in;
    int serial = 0;
    while (std::scanf("%d %d %d %d %d %d %lld %lld %lld %lld", &in.B, &in.V, &in.H, &in.W, &in.C, &serial, &in.opt_heavy_t,
                      &in.opt_part_px, &in.opt_one_view, &in.opt_one_view_split) == 10) {
        in.serial_sums = serial != 0;
        const SplitPlan sp = plan_split(in);
        const PlanArgs &p = sp.plan;
        std::printf("%lld %d  %d %d %d %d %d %d %d %d  %d %d %d\n", part_slot_cap(in.B, in.V, in.H, in.W, in.C), sp.heavy_t, p.heavy_t,
                    p.part_t, p.part_px, p.count_heavy, p.dyn_px_min, p.dyn_t_ratio, p.dyn_t_floor, p.cell_in_item, (int)sp.one_view,
                    (int)sp.one_split, (int)sp.plans_parts);
    }
    return 0;
}
