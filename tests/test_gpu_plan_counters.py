"""The split plan the host computes (csrc/vp_plan.h) is the plan the device was told: for the small calls of the hand-derived
table (tests/plan_cases.py) whose numbers are fixed on the host, one tiny blocking call, and the heavy threshold, the split
threshold and the pixels per part that k_worklist left in the call's status words are the table's."""
import numpy as np
import pytest
import torch

from plan_cases import CASES, HEAVY, ONE_SPLIT, ONE_VIEW, PART
from synthetic_scene import make_features_np, make_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# 32 x 48 images, and neither number left to the device (dyn_px_min, dyn_t_ratio)
SMALL = [c for c in CASES if c[0][2:4] == (32, 48) and c[4][4] == 0 and c[4][5] == 0]


@pytest.fixture(scope="module")
def scene():
    s = make_scene(2000, 4, 48, 32, seed=911, room=(5.0, 4.0, 2.4))
    return s, make_features_np(4, 32, 48, 8, seed=911)[None]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: f"V{c[0][1]}{'-serial' if c[1] else ''}" + "".join(f"-{k[4:]}={v}" for k, v in c[2].items()))
def test_counters_hold_the_planned_numbers(scene, case):
    import voxproj_host
    (B, V, H, W, C), serial, opts, _, plan = case
    s, feats = scene
    assert (B, H, W, C) == (1, s.height, s.width, feats.shape[-1]) and V <= s.n_views
    dev = torch.device(DEV)
    n_rows = s.n_vox + 1
    ws = voxproj_host.Workspace()
    for key, opt in ((HEAVY, voxproj_host.VP_OPT_HEAVY_THRESHOLD), (PART, voxproj_host.VP_OPT_PART_PIXELS),
                     (ONE_VIEW, voxproj_host.VP_OPT_ONE_VIEW_GATHER), (ONE_SPLIT, voxproj_host.VP_OPT_ONE_VIEW_SPLIT)):
        if key in opts:
            ws.set_option(opt, opts[key])
    count, out = torch.zeros(n_rows, dtype=torch.int32, device=dev), torch.zeros(n_rows, C, device=dev)
    voxproj_host.project_features_raw(torch.from_numpy(np.ascontiguousarray(feats[:, :V])).to(dev),
                                      torch.from_numpy(s.occ[None].astype(np.int64)).to(dev),
                                      torch.from_numpy(s.c2w[:V]).reshape(-1).contiguous().to(dev), torch.from_numpy(s.intr[None]).to(dev),
                                      [float(x) for x in s.opts()], count, out, [float(x) for x in s.grid_origin], s.voxel_size,
                                      workspace=ws, sync=True, serial_sums=serial)
    ctr = voxproj_host.counters(ws, dev)
    ws.release()
    assert int(count.sum()) > 0, "the scene has no voxel in view"
    assert (ctr["heavy_t"], ctr["part_t"], ctr["part_px"]) == plan[:3]
