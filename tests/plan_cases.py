"""The split plan of a projector call (csrc/vp_plan.h, plan_split) for a list of calls, derived BY HAND from the rules -- not
printed by the code.  tests/test_plan_cpu.py checks the function against it on the host, tests/test_gpu_plan_counters.py checks
that the device was told the same numbers.

A case: (B, V, H, W, C), serial_sums, options, slot_cap, plan; options are -1 (the library's default) unless named; plan =
(heavy_t, part_t, part_px, count_heavy, dyn_px_min, dyn_t_ratio, dyn_t_floor, cell_in_item).

The rules.  slot_cap = max(64, min(65536, 2*B*V*H*W, max(1024, 65536 * 2048 / (4 * C)))), one-view calls (B*V == 1): 8192 at most.
bound = ceil(2*B*V*H*W / slot_cap).  heavy_t = min(256 + 64*B*V, 2048), one-view calls 320, VP_OPT_HEAVY_THRESHOLD replaces it,
VP_FLAG_SERIAL_SUMS makes it 2^31 - 1 (nothing is split).  Calls that are not one-view calls (more views, or
VP_OPT_ONE_VIEW_GATHER = 0): part_px = max(VP_OPT_PART_PIXELS or heavy_t, bound), heavy_t = part_t = max(heavy_t, part_px).
One-view calls: VP_OPT_ONE_VIEW_SPLIT = 0: the march counts the voxels above heavy_t (count_heavy = 0), no parts.  Otherwise
T = VP_OPT_ONE_VIEW_SPLIT, else VP_OPT_HEAVY_THRESHOLD, else 0; part_px = max(VP_OPT_PART_PIXELS, bound) if that option is set,
else max(ceil(T / 2), bound) if T > 0, else 0 with dyn_px_min = 32 (the device sizes the parts); heavy_t = part_t = max(T, part_px) if
T > 0, else 0 with dyn_t_ratio = 2 (the device's); dyn_t_floor = 256 for views of up to 262144 pixels; cell_in_item = 1."""
INT_MAX = 2147483647
HEAVY, PART, ONE_VIEW, ONE_SPLIT = "opt_heavy_t", "opt_part_px", "opt_one_view", "opt_one_view_split"

CASES = [
    ((1, 4, 32, 48, 8), False, {}, 12288, (512, 512, 512, 1, 0, 0, 0, 0)),
    ((1, 126, 548, 968, 512), False, {}, 65536, (2048, 2048, 2048, 1, 0, 0, 0, 0)),
    ((1, 300, 548, 968, 512), False, {}, 65536, (4857, 4857, 4857, 1, 0, 0, 0, 0)),
    ((1, 4, 32, 48, 8), True, {}, 12288, (INT_MAX, INT_MAX, 0, 1, 0, 0, 0, 0)),
    ((1, 1, 548, 968, 512), False, {}, 8192, (0, 0, 0, 1, 32, 2, 0, 1)),
    ((1, 1, 274, 484, 512), False, {}, 8192, (0, 0, 0, 1, 32, 2, 256, 1)),
    ((1, 1, 548, 968, 512), False, {ONE_SPLIT: 0}, 8192, (320, INT_MAX, 0, 0, 0, 0, 0, 0)),
    ((1, 1, 548, 968, 512), False, {ONE_VIEW: 0}, 8192, (320, 320, 320, 1, 0, 0, 0, 0)),
    ((1, 1, 548, 968, 512), False, {ONE_SPLIT: 600}, 8192, (600, 600, 300, 1, 0, 0, 0, 1)),
    ((1, 1, 32, 48, 8), False, {ONE_SPLIT: 600}, 3072, (600, 600, 300, 1, 0, 0, 256, 1)),
    # VP_OPT_HEAVY_THRESHOLD alone: 2*B*V*H*W = 12288 = slot_cap, bound 1; part_px = heavy_t = 100
    ((1, 4, 32, 48, 8), False, {HEAVY: 100}, 12288, (100, 100, 100, 1, 0, 0, 0, 0)),
    # VP_OPT_PART_PIXELS alone: part_px = max(64, 1), heavy_t = max(512, 64)
    ((1, 4, 32, 48, 8), False, {PART: 64}, 12288, (512, 512, 64, 1, 0, 0, 0, 0)),
    # ... on a one-view call: the parts are fixed (max(16, 1)), the threshold stays the device's (2 * part_px, 256 at the least)
    ((1, 1, 32, 48, 8), False, {PART: 16}, 3072, (0, 0, 16, 1, 0, 2, 256, 1)),
    # a one-view call with both options where the slot bound wins: 2*H*W = 1060928, bound = ceil(1060928 / 8192) = 130 > 50;
    # heavy_t = max(100, 130); 530464 pixels > 262144: no floor
    ((1, 1, 548, 968, 512), False, {ONE_SPLIT: 100, PART: 50}, 8192, (130, 130, 130, 1, 0, 0, 0, 1)),
    # the A/B arm on the small view (tests/test_gpu_plan_counters.py)
    ((1, 1, 32, 48, 8), False, {ONE_SPLIT: 0}, 3072, (320, INT_MAX, 0, 0, 0, 0, 0, 0)),
]


def options(case):
    """The four options of a case, in plan_table.cpp's order."""
    return [case[2].get(k, -1) for k in (HEAVY, PART, ONE_VIEW, ONE_SPLIT)]
