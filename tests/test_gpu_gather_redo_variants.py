"""The whole-image redo in every row variant and every role.  The suite's other redo tests run at C = 8 or 12 in fp32 only:
<1,4,.> with a single channel pass.  Here the several-cells-per-ID scene of
test_split_voxels_whose_boxes_miss_pixels_are_redone_over_whole_images (IDs = occ % 5 + 1: the search box is built around ONE
cell of an ID and misses the others' pixels) runs with rows of
    fp32 C = 12   <1,4,.>  one ragged pass        fp32 C = 259  <4,1,.>  two passes
    fp32 C = 520  <2,4,.>  two, the second ragged  fp16 C = 520  <1,8,.>  two passes
in the five roles a voxel can have: a multi-view call that splits nothing (gather_voxel_wave) or splits above 64 pixels into parts
of 32 (gather_part_wave, k_combine_parts and its workgroup redo), and one-view calls view by view: serial (k_gather_one's deal),
parts (VP_OPT_ONE_VIEW_SPLIT = 12, VP_OPT_PART_PIXELS = 5) and the workgroup arm (VP_OPT_ONE_VIEW_SPLIT = 0, threshold 6).
Counts and view counts exact, rows one wavefront summed the oracle's bytes, split rows by tests/sum_criteria.py; the fp16 runs
moreover leave the bytes of the same role's fp32 run on the widened values.

The feature maps carry a mean of half their element's standard deviation (unit vectors + 0.5 / sqrt(C), as the single-voxel test of
test_gpu_trajectory.py does), so that the element-wise clause (E) of sum_criteria has something to bite on: with zero-mean maps a
row of n ~ 2000 pixels is a cancellation residue (|sum| / sum|addend| ~ 1 / sqrt(n) = 0.02) and (E) promises nothing on it.  With
the mean, |sum| / sum|addend| ~ 0.5 / 0.9 = 0.55 +- 0.02 for every element, while (E) promises an element from
4 sqrt(n) 2^-24 / 1e-4 = 0.11 (n = 2149, the longest row) on, and every element is within a few per cent of its row's largest: ALL
C elements of the five touched rows are promised.  That count is asserted (_min_promised), from the oracle's data alone."""
import numpy as np
import pytest
import torch

from sum_criteria import assert_sums_vs_oracle
from synthetic_scene import make_features_np, make_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V, W, H, N_ROWS = 6, 48, 32, 7
SERIAL = 10 ** 8                  # a heavy threshold no voxel reaches
ROWS = [("f32", 12), ("f32", 520), ("f32", 259), ("f16", 520)]
ROLES = ["wave", "parts", "one_serial", "one_parts", "one_workgroup"]
_refs = {}


def _min_promised(C):
    return 5 * C                  # every element of the rows of IDs 1 .. 5 (see the module's docstring)


def _options(vh, role):
    return {"wave": {vh.VP_OPT_HEAVY_THRESHOLD: SERIAL},
            "parts": {vh.VP_OPT_HEAVY_THRESHOLD: 64, vh.VP_OPT_PART_PIXELS: 32},
            "one_serial": {vh.VP_OPT_HEAVY_THRESHOLD: SERIAL},
            "one_parts": {vh.VP_OPT_ONE_VIEW_SPLIT: 12, vh.VP_OPT_PART_PIXELS: 5},
            "one_workgroup": {vh.VP_OPT_HEAVY_THRESHOLD: 6, vh.VP_OPT_ONE_VIEW_SPLIT: 0}}[role]


def _reference(oracle_mod, kind, C):
    """Scene, the feature maps as the GPU reads them and widened to fp32, and the oracle's call on the widened values (computed once)."""
    if (kind, C) not in _refs:
        s = make_scene(2000, V, W, H, seed=71, room=(5.0, 4.0, 2.4))
        occ = np.where(s.occ > 0, (s.occ % 5) + 1, 0).astype(np.int64)[None]
        feats = make_features_np(V, H, W, C, seed=72)[None] + np.float32(0.5 / np.sqrt(C))
        if kind == "f16":
            feats = feats.astype(np.float16)
        f32 = feats.astype(np.float32)
        count, out = np.zeros(N_ROWS, np.int32), np.zeros((N_ROWS, C), np.float32)
        r = oracle_mod.project_features(f32, occ, s.c2w.reshape(-1), s.intr[None], s.opts(), s.grid_origin, s.voxel_size, count, out,
                                        want_f64=True)
        assert r["rc"] == 0
        per_view = np.stack([np.bincount(r["hits"][0, v].reshape(-1), minlength=N_ROWS) for v in range(V)])
        views = (per_view[:, 1:] > 0).sum(axis=0)
        _refs[(kind, C)] = (s, occ, feats, f32, r, count, out, per_view, views)
    return _refs[(kind, C)]


def _run(role, s, occ, feats):
    """The role's call(s) into fresh outputs: (count, out, views_hit, box misses, rows some call split)."""
    import voxproj_host as vh
    dev = torch.device(DEV)
    C = feats.shape[-1]
    ws = vh.Workspace()
    for opt, val in _options(vh, role).items():
        ws.set_option(opt, val)
    count_t = torch.zeros(N_ROWS, dtype=torch.int32, device=dev)
    out_t = torch.zeros(N_ROWS, C, device=dev)
    views_t = torch.zeros(N_ROWS, dtype=torch.int32, device=dev)
    occ_t, intr_t = torch.from_numpy(occ).to(dev), torch.from_numpy(s.intr[None]).to(dev)
    box_miss, thresholds = 0, []
    for views in ([list(range(V))] if role in ("wave", "parts") else [[v] for v in range(V)]):
        vh.project_features_raw(torch.from_numpy(np.ascontiguousarray(feats[:, views])).to(dev), occ_t,
                                torch.from_numpy(np.ascontiguousarray(s.c2w[views])).reshape(-1).to(dev), intr_t,
                                [float(x) for x in s.opts()], count_t, out_t, [float(x) for x in s.grid_origin], s.voxel_size,
                                workspace=ws, sync=True, views_hit=views_t)
        ctr = vh.counters(ws, dev)
        assert ctr["bad_id"] == 0, ctr
        box_miss += ctr["box_miss"]
        thresholds.append(ctr["part_t"] if role == "one_parts" else ctr["heavy_t"])
    res = count_t.cpu().numpy(), out_t.cpu().numpy(), views_t.cpu().numpy(), box_miss, thresholds
    ws.release()
    return res


@pytest.mark.parametrize("role", ROLES)
@pytest.mark.parametrize("kind,C", ROWS)
def test_boxes_that_miss_pixels_are_redone_in_every_row_variant_and_role(oracle_mod, kind, C, role):
    s, occ, feats, f32, r, count, out, per_view, views = _reference(oracle_mod, kind, C)
    got_c, got_o, got_v, box_miss, thresholds = _run(role, s, occ, feats)
    print(f"{kind} C={C} {role}: box_miss {box_miss}, thresholds {thresholds}, pixels per row {count.tolist()}")
    assert box_miss > 0
    assert np.array_equal(got_c, count)
    assert np.array_equal(got_v[1:], views) and got_v[0] == 0
    if role in ("wave", "parts"):
        split = count > thresholds[0]
    else:
        split = (per_view > np.asarray(thresholds)[:, None]).any(axis=0)
    assert split.any() == (role not in ("wave", "one_serial")), (role, thresholds)
    assert got_o[~split].tobytes() == out[~split].tobytes(), "rows summed by one wavefront must be the oracle's bytes"
    if split.any():
        res = assert_sums_vs_oracle(got_o, r, f32, count, split=split, oracle32=out, dev=DEV)
        print(f"  sum criterion {res}")
        assert res["promised"] >= _min_promised(C), res
        assert "split_vs_serial" in res, res
    if kind == "f16":
        wide_c, wide_o, wide_v, _, _ = _run(role, s, occ, f32)
        assert np.array_equal(got_c, wide_c) and np.array_equal(got_v, wide_v)
        assert got_o.tobytes() == wide_o.tobytes(), "fp16 maps must leave the bits of the fp32 call on the widened values"
