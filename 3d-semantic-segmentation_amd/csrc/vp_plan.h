// vp_plan.h -- the split plan of a projector call: which voxels are cut into parts, how large the parts are, and how many part
// slots a buffer set has.  Pure host arithmetic over <algorithm> and <cstdint>: no HIP types, compiles with a plain C++17
// compiler (tests/plan_table.cpp prints it, tests/test_plan_cpu.py checks the table).  Included by voxproj.hip in front of
// vp_common.h, whose workspace record keeps the PlanArgs of the last call.
#pragma once

#include <algorithm>
#include <cstdint>

namespace {

// One-view calls size their parts on the device, from the number of pixels the view's rays hit (k_worklist): the smallest part,
// and how many parts' worth of pixels a voxel must exceed to be cut (VP_OPT_PART_PIXELS / VP_OPT_ONE_VIEW_SPLIT fix them)
#ifndef VP_ONE_VIEW_PART_MIN
#define VP_ONE_VIEW_PART_MIN 32
#endif
#ifndef VP_ONE_VIEW_T_RATIO
#define VP_ONE_VIEW_T_RATIO 2
#endif
#ifndef VP_ONE_VIEW_T_FLOOR_SMALL
#define VP_ONE_VIEW_T_FLOOR_SMALL 256
#endif
constexpr int ONE_VIEW_PART_MIN = VP_ONE_VIEW_PART_MIN, ONE_VIEW_T_RATIO = VP_ONE_VIEW_T_RATIO, ONE_VIEW_T_FLOOR_SMALL = VP_ONE_VIEW_T_FLOOR_SMALL;

// What k_worklist plans with.  Calls of more than one view: heavy_t == part_t and part_px are the host's (plan_split).
// One-view calls that split (round 6): no voxel is shared by a workgroup any more, heavy_t == part_t again, and both numbers may
// be left to the device: dyn_px_min > 0 -> part_px = max(dyn_px_min, 2 * hits / slots), with `hits` the pixels of the view whose
// ray hit a voxel (counted by the march, ST_NHIT) -- about one part per wavefront the machine holds on a frame that is all large
// voxels, parts of 32 pixels on a frame that is mostly misses, where the longest single item IS the launch (a wavefront alone
// pulls ~5 GB/s: 320 rows of 2 KiB last 128 us); dyn_t_ratio > 0 -> part_t = heavy_t = max(dyn_t_ratio * part_px, dyn_t_floor): a
// voxel is worth cutting only when one wavefront would need a good part of the launch's duration for it -- ~26 us are 64 pixels
// with 4 rows in flight per wavefront, and views of up to 262144 pixels (8 rows in flight; a quarter-resolution frame is ten
// thousand voxels of a dozen pixels, bounded by round trips per voxel, not by its longest voxel) gain nothing below 256.
struct PlanArgs {
    int heavy_t, part_t, part_px;
    int count_heavy;      // add the split voxels to ST_NHEAVY (0: the march counts the voxels above heavy_t, one-view calls without parts)
    int dyn_px_min, dyn_t_ratio, dyn_t_floor;
    int cell_in_item;     // parts[].w = the voxel's cell in batch 0 instead of its first slot (one-view calls: B == 1)
};

// Views whose first ID tile is fetched together by the one-wavefront gather (template argument G of k_gather; 1 = one view
// at a time).  fp16 rows: 4 (-1 % pipelined, round 2).  fp32 rows: 4 for small images (a voxel of R1's 484x274 views gathers
// half the rows per view an R2 voxel does, so the dependent tile fetch in front of them weighs twice as much: -1.4 % per
// pipelined R1 call), 1 otherwise (968x548: equal alone, +0.3 % pipelined) -- profiles/r03_ab_id_tile_grouping_fp32.log.
// The same size separates the one-view views that keep 8 rows in flight per wavefront, and whose parts have a floor (above).
constexpr long long GATHER_G32_SMALL_IMAGE = 262144;     // pixels per view up to which fp32 calls use G = 4

// Part slots of one buffer set (split voxels, vp_gather.h): a voxel above the heavy threshold is summed as P parts, each
// part's C-wide partial row in a slot.  The number of slots bounds how finely a call can be cut: with part_px >= 2*B*V*H*W /
// slots and heavy_t >= part_px the parts of a call can never outnumber the slots (plan_split raises both to that bound).
// 65536 slots -- parts of 2048 pixels for calls of up to 67 M pixels (126 views of 968x548: the 100-108 views a call of fp16 maps
// holds; round 5's 32768 slots forced parts of 3238-3373 pixels on those calls: R2T fp16 25.3 -> 24.9 ms, A1 fp16 14.9 -> 13.9 ms
// per pass, profiles/r06_f16_part_slots.log) --, fewer when the rows are wide (128 MiB of partial rows per set at most) or the
// call is small.
#ifndef VP_MAX_SLOTS
#define VP_MAX_SLOTS 65536
#endif
#ifndef VP_ONE_VIEW_SLOTS
#define VP_ONE_VIEW_SLOTS 8192
#endif
inline long long part_slot_cap(int B, int V, int H, int W, int C)
{
    const long long px2 = 2ll * B * V * (long long)H * W;
    const long long by_bytes = std::max<long long>(1024, ((long long)VP_MAX_SLOTS * 2048) / (std::max(C, 1) * 4ll));
    long long cap = std::max<long long>(64, std::min<long long>(VP_MAX_SLOTS, std::min(px2, by_bytes)));
    // a call of ONE view cuts voxels into parts of 256 pixels by default (128 at the least for a view of 524 k pixels): 8192 slots
    // (16 MiB at C = 512) -- the drop-in module's scratch buffer should not carry 2 x 128 MiB it never touches
    if ((long long)B * V == 1) cap = std::min<long long>(cap, VP_ONE_VIEW_SLOTS);
    return cap;
}

struct PlanIn {
    int B, V, H, W, C;
    bool serial_sums;                  // VP_FLAG_SERIAL_SUMS
    // options of the workspace (vp_workspace_set_option); -1 = the library's default
    long long opt_heavy_t, opt_part_px, opt_one_view, opt_one_view_split;
};

struct SplitPlan {
    PlanArgs plan;                     // what k_worklist is told
    int heavy_t;                       // the host's copy of the heavy threshold (after the part-slot bound)
    bool one_view;                     // the call takes the one-view gather (k_gather_one)
    bool one_split;                    // ... and cuts its large voxels into parts
    bool plans_parts;                  // the work list may hold part items: k_combine_parts follows the gather
};

inline bool plan_has_parts(const PlanArgs &plan) { return plan.part_px > 0 || plan.dyn_px_min > 0; }

inline SplitPlan plan_split(const PlanIn &in)
{
    const int B = in.B, V = in.V, H = in.H, W = in.W;
    const long long slot_cap = part_slot_cap(B, V, H, W, in.C);
    // More pixels than heavy_t in one call -> the voxel is not one wavefront's job: it is cut into parts of part_px pixels
    // (vp_gather.h, "Split voxels").  Calls of more than one view: both numbers default to min(256 + 64*B*V, 2048) -- the longest
    // item a wavefront can be handed bounds the tail of the launch; the last items run on an emptying machine at ~4 GB/s per
    // wavefront, 2048 rows of 2 KiB in a millisecond (sweep of 512 ... 4096: profiles/r05_ab_split_voxels.log, fp16 calls:
    // r06_f16_part_slots.log).  One-view calls: the device sizes both from the view's hit total (PlanArgs); 256 + 64 is the
    // threshold of round 5's workgroup role, kept as the A/B arm (VP_OPT_ONE_VIEW_SPLIT = 0).
    int heavy_t = (int)std::min<long long>(256 + 64ll * B * V, 2048);
    if ((long long)B * V == 1) heavy_t = 256 + 64;
    if (in.opt_heavy_t > 0) heavy_t = (int)std::min<long long>(in.opt_heavy_t, 2147483647ll);   // VP_OPT_HEAVY_THRESHOLD
    if (in.serial_sums) heavy_t = 2147483647;
    // One-view calls (the drop-in module's, the parity aggregator's) take the one-view gather: a fixed grid of wavefronts
    // dealt the size-ordered list, a wavefront's boxes computed one voxel per lane, the next voxel's tile and row fetched
    // under the current voxel's rows (vp_gather.h, k_gather_one).  VP_OPT_ONE_VIEW_GATHER = 0 keeps k_gather as the A/B arm.
    const bool one_view = (long long)B * V == 1 && in.opt_one_view != 0;
    // The parts' partial rows live in the buffer set's part slots, and a call's parts must never outnumber them: a split voxel
    // has c > heavy_t >= part_px pixels and P = ceil(c / part_px) <= 2c / part_px parts, the c of a call add up to at most
    // B*V*H*W, so part_px >= 2*B*V*H*W / slots is enough -- both values are raised to that bound (only calls larger than the
    // bench's are: 65536 slots allow parts of 2048 pixels up to 67 M pixels per call).
    PlanArgs plan;
    plan.heavy_t = heavy_t; plan.part_t = 2147483647; plan.part_px = 0; plan.count_heavy = 1; plan.dyn_px_min = 0; plan.dyn_t_ratio = 0;
    plan.dyn_t_floor = 0; plan.cell_in_item = 0;
    const long long px2 = 2ll * B * V * (long long)H * W;
    // One-view calls (round 6) cut their large voxels into parts too -- one wavefront of k_gather_one per part, k_combine_parts
    // behind it -- and size the parts on the device from the view's hit total (PlanArgs).  VP_OPT_ONE_VIEW_SPLIT = 0
    // keeps round 5's path (a workgroup per voxel above 320 pixels) as the A/B arm.
    const bool one_split = one_view && heavy_t != 2147483647 && in.opt_one_view_split != 0;
    if (!one_view && heavy_t != 2147483647) {
        long long ppx = in.opt_part_px > 0 ? in.opt_part_px : std::max<long long>(1, heavy_t);     // VP_OPT_PART_PIXELS
        ppx = std::max(ppx, (px2 + slot_cap - 1) / slot_cap);
        plan.part_px = (int)std::min<long long>(ppx, 2147483647ll);
        heavy_t = std::max(heavy_t, plan.part_px);
        plan.heavy_t = plan.part_t = heavy_t;
    } else if (one_split) {
        // fixed numbers where the options give them (VP_OPT_ONE_VIEW_SPLIT, else VP_OPT_HEAVY_THRESHOLD; VP_OPT_PART_PIXELS), raised
        // to the slot bound like those of multi-view calls; otherwise the device's
        const long long T = in.opt_one_view_split > 0 ? in.opt_one_view_split : in.opt_heavy_t > 0 ? in.opt_heavy_t : 0;
        long long ppx = in.opt_part_px > 0 ? std::max(in.opt_part_px, (px2 + slot_cap - 1) / slot_cap) : 0;
        if (ppx == 0 && T > 0) ppx = std::max<long long>((T + ONE_VIEW_T_RATIO - 1) / ONE_VIEW_T_RATIO, (px2 + slot_cap - 1) / slot_cap);
        plan.part_px = (int)std::min<long long>(ppx, 2147483646ll);
        plan.dyn_px_min = ppx > 0 ? 0 : ONE_VIEW_PART_MIN;
        plan.heavy_t = plan.part_t = T > 0 ? (int)std::min<long long>(std::max(T, ppx), 2147483646ll) : 0;
        plan.dyn_t_ratio = T > 0 ? 0 : ONE_VIEW_T_RATIO;
        plan.dyn_t_floor = (long long)H * W <= GATHER_G32_SMALL_IMAGE ? ONE_VIEW_T_FLOOR_SMALL : 0;
        plan.cell_in_item = 1;
        heavy_t = plan.heavy_t;
    } else if (one_view) {
        plan.count_heavy = 0;      // the march enlists and counts the voxels above heavy_t
    }
    return SplitPlan{plan, heavy_t, one_view, one_split, plan_has_parts(plan)};
}

}  // namespace
