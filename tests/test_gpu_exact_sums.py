"""Every role of the gather (csrc/vp_gather.h: k_gather, k_gather_one, k_combine_parts) on feature maps whose sums are exact in
every order (tests/exact_maps.py): small integers, count * max|value| < 2^24 per row.  The serial wavefront, parts added in slot
order, the LDS meet of the workgroup arm, the whole-image redo behind a part, fp16 maps widened on load and accumulation across
calls must then all leave the bytes of the int64 scatter-add over the oracle's hit image -- no tolerance anywhere in this file,
every comparison of ``out`` is tobytes() equality through assert_exact, whose message names the row and, for a lost or doubled
pixel, (v, y, x).

Every case asserts, in this order: the hit image is the oracle's; ``count`` is the reference's; ``views_hit`` is exact; the
counters say the path the case claims really ran; the headroom holds (from the oracle's counts); all rows are exact; and for fp16
maps the bytes are also those of the same role's run on the widened fp32 maps.

  a  multi-view calls with parts of 32 pixels above 64 (k_combine_parts), one case per row variant, at V = 9 (G = 4) and V = 3
     (G = 1); the same rows with the library's default thresholds, where nothing splits
  b  B = 2: two grids in one call
  c  boxes that miss pixels: the whole-image redo in five roles and four row variants; the same with voxels whose parts are
     added in the same launch
  d  three one-view calls into one ``out``: serial, fixed parts, the workgroup arm
  e  one-view calls with device-sized parts (no option set), with and without the 256-pixel floor
  f  the part-slot bound raising the part size (rows of 32 KiB)
  g  one fixed call sequence on one workspace: ranged pipelined pair, whole pipelined call, one-view call, smaller call
  h  more than 512 split voxels in one call: k_combine_parts' workgroups take a second lap (tests/README_laps.md), adding parts
     and redoing voxels over whole images there; k_worklist hands out split entries from two workgroups; job mode
  i  two one-view calls on one workspace whose hit counters k_zero_call clears in two laps"""
import numpy as np
import pytest
import torch

from exact_maps import assert_exact, assert_headroom, exact_maps, int_reference
from synthetic_scene import make_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOM = (5.0, 4.0, 2.4)
SERIAL = 10 ** 8                  # a heavy threshold no voxel reaches
_scenes, _refs = {}, {}


class _Scene:
    """A scene as one call sees it: occ int64 [B, Z, Y, X], c2w [B * V, 4, 4], intr [B, 4], and the oracle's hit image [B, V, H, W]."""

    def __init__(self, oracle_mod, key, s, occ, c2w, intr, B, n_rows):
        self.key, self.s, self.occ, self.c2w, self.intr, self.B, self.n_rows = key, s, occ, np.ascontiguousarray(c2w), intr, B, n_rows
        self.V, self.H, self.W = len(c2w) // B, s.height, s.width
        self.hits = oracle_mod.first_hit(occ, self.c2w.reshape(-1), intr, s.opts(), s.grid_origin, s.voxel_size, B, self.V)
        assert self.hits.shape == (B, self.V, self.H, self.W) and 0 <= self.hits.min() and self.hits.max() < n_rows

    def counts(self, views=None):
        """Pixels per row of a call of ``views`` (all by default), from the oracle's hit image; row 0 (no hit) zeroed."""
        h = self.hits if views is None else self.hits[:, views]
        c = np.bincount(h.reshape(-1), minlength=self.n_rows).astype(np.int64)
        c[0] = 0
        return c

    def views_hit(self, views=None):
        n = np.zeros(self.n_rows, np.int64)
        for b in range(self.B):
            for v in (range(self.V) if views is None else views):
                ids = np.unique(self.hits[b, v])
                n[ids[ids > 0]] += 1
        return n


def _room(oracle_mod, V, seed, W=48, H=32):
    key = ("room", V, seed, W, H)
    if key not in _scenes:
        s = make_scene(2000, V, W, H, seed=seed, room=ROOM)
        _scenes[key] = _Scene(oracle_mod, key, s, s.occ[None].astype(np.int64), s.c2w, s.intr[None], 1, s.n_vox + 1)
    return _scenes[key]


def _redo_scene(oracle_mod):
    """Several cells per ID (occ % 5 + 1, 7 rows, V = 6): the search box is built around ONE cell of an ID and misses the others'
    pixels (test_gpu_gather_redo_variants.py)."""
    if "redo" not in _scenes:
        s = make_scene(2000, 6, 48, 32, seed=71, room=ROOM)
        occ = np.where(s.occ > 0, (s.occ % 5) + 1, 0).astype(np.int64)[None]
        _scenes["redo"] = _Scene(oracle_mod, "redo", s, occ, s.c2w, s.intr[None], 1, 7)
    return _scenes["redo"]


def _mixed_scene(oracle_mod):
    """The redo scene, except that the nine voxels of more than 64 pixels keep a row of their own (rows 6 .. 14; 16 rows): their
    boxes hold every pixel.  A call that splits then has voxels whose parts k_combine_parts adds next to voxels it redoes over whole
    images -- in the redo scene alone EVERY split voxel is redone (box_miss == n_split) and the adding arm never runs."""
    if "mixed" not in _scenes:
        base = _room(oracle_mod, 6, 71)
        big = np.nonzero(base.counts() > 64)[0]
        assert len(big) == 9
        own = np.zeros(base.n_rows, np.int64)
        own[big] = 6 + np.arange(len(big))
        occ = np.where(base.s.occ > 0, np.where(own[base.s.occ] > 0, own[base.s.occ], (base.s.occ % 5) + 1), 0).astype(np.int64)[None]
        _scenes["mixed"] = _Scene(oracle_mod, "mixed", base.s, occ, base.s.c2w, base.s.intr[None], 1, 16)
        assert (_scenes["mixed"].counts()[6:15] == base.counts()[big]).all()
    return _scenes["mixed"]


def _two_grids(oracle_mod):
    """Two different grids with other intrinsics in one call, three views each (test_batch_of_two_grids)."""
    if "two" not in _scenes:
        s = make_scene(2000, 6, 48, 32, seed=16, room=ROOM)
        s2 = make_scene(2000, 6, 48, 32, seed=17, room=ROOM)
        assert s.occ.shape == s2.occ.shape
        occ = np.stack([s.occ, s2.occ]).astype(np.int64)
        intr = np.stack([s.intr, s.intr * np.float32(1.1)])
        _scenes["two"] = _Scene(oracle_mod, "two", s, occ, s.c2w, intr, 2, s.n_vox + 1)
    return _scenes["two"]


def _maps(sc, C, kind, seed=72):
    """[B, V, H, W, C] exact maps, fp32 or fp16 (the same numbers), and the int64 reference of the whole scene; computed once.
    In channel 3 the view of batch b is b * V + v."""
    if (sc.key, C) not in _refs:
        m = exact_maps(sc.B * sc.V, sc.H, sc.W, C, seed=seed).reshape(sc.B, sc.V, sc.H, sc.W, C)
        ref, count = int_reference(sc.hits, m, sc.n_rows)
        assert np.array_equal(count, sc.counts())
        for a in (ref, count):
            a.setflags(write=False)
        _refs[(sc.key, C)] = (m, ref, count)
    m, ref, count = _refs[(sc.key, C)]
    return (m.astype(np.float16) if kind == "f16" else m), ref, count


def _blocking_calls(sc, maps, options, view_sets):
    """One blocking call per entry of ``view_sets`` (a list of views; None = the whole scene) on a fresh workspace with
    ``options``, all adding into one count / out / views_hit.  After every call the hit image is compared with the oracle's.
    Returns count, out, views_hit and every call's counters."""
    import voxproj_host as vh
    dev = torch.device(DEV)
    C = maps.shape[-1]
    ws = vh.Workspace()
    for opt, val in options.items():
        ws.set_option(opt, val)
    count_t = torch.zeros(sc.n_rows, dtype=torch.int32, device=dev)
    out_t = torch.zeros(sc.n_rows, C, device=dev)
    views_t = torch.zeros(sc.n_rows, dtype=torch.int32, device=dev)
    occ_t, intr_t = torch.from_numpy(sc.occ).to(dev), torch.from_numpy(sc.intr).to(dev)
    ctrs = []
    for views in view_sets:
        assert views is None or sc.B == 1
        feats = maps if views is None else np.ascontiguousarray(maps[:, views])
        c2w = sc.c2w if views is None else np.ascontiguousarray(sc.c2w[views])
        vh.project_features_raw(torch.from_numpy(feats).to(dev), occ_t, torch.from_numpy(c2w).reshape(-1).to(dev), intr_t,
                                [float(x) for x in sc.s.opts()], count_t, out_t, [float(x) for x in sc.s.grid_origin], sc.s.voxel_size,
                                workspace=ws, sync=True, views_hit=views_t)
        want = sc.hits if views is None else sc.hits[:, views]
        assert np.array_equal(vh.hit_image(ws, dev).cpu().numpy(), want), f"hit image of the call of views {views}"
        ctrs.append(vh.counters(ws, dev))
    res = count_t.cpu().numpy(), out_t.cpu().numpy(), views_t.cpu().numpy(), ctrs
    ws.release()
    return res


# What the counters of one call must say for the role it claims; each returns the rows the call summed other than by one wavefront
def _ran_serial(ctr, c):
    assert ctr["n_split"] == 0 and ctr["n_parts"] == 0 and ctr["n_heavy"] == 0, ctr
    return np.zeros(len(c), bool)


def _ran_parts(ctr, c, part_t, part_px):
    assert (ctr["part_t"], ctr["part_px"], ctr["heavy_t"]) == (part_t, part_px, part_t), ctr
    big = c[c > part_t]
    assert ctr["n_split"] == len(big) and ctr["n_heavy"] == len(big), (ctr, len(big))
    assert ctr["n_parts"] == int(np.sum((big + part_px - 1) // part_px)), ctr
    return c > part_t


def _ran_workgroup(ctr, c, heavy_t):
    assert ctr["heavy_t"] == heavy_t and ctr["n_split"] == 0 and ctr["n_parts"] == 0, ctr
    assert ctr["n_heavy"] == int((c > heavy_t).sum()), ctr
    return c > heavy_t


def _role(vh, role):
    """options, one-view calls?, the counters' check"""
    return {
        "wave": ({vh.VP_OPT_HEAVY_THRESHOLD: SERIAL}, False, _ran_serial),
        "parts": ({vh.VP_OPT_HEAVY_THRESHOLD: 64, vh.VP_OPT_PART_PIXELS: 32}, False, lambda ctr, c: _ran_parts(ctr, c, 64, 32)),
        "one_serial": ({vh.VP_OPT_HEAVY_THRESHOLD: SERIAL}, True, _ran_serial),
        "one_parts": ({vh.VP_OPT_ONE_VIEW_SPLIT: 12, vh.VP_OPT_PART_PIXELS: 5}, True, lambda ctr, c: _ran_parts(ctr, c, 12, 5)),
        "one_workgroup": ({vh.VP_OPT_HEAVY_THRESHOLD: 6, vh.VP_OPT_ONE_VIEW_SPLIT: 0}, True, lambda ctr, c: _ran_workgroup(ctr, c, 6)),
    }[role]


def _check_role(label, sc, C, kind, role, box_miss=False, options=None, ran=None):
    """The seven assertions for one role on one scene and row variant.  Returns (rows some call split, the calls' counters)."""
    import voxproj_host as vh
    role_options, one_view, role_ran = _role(vh, role)
    options = role_options if options is None else options
    ran = role_ran if ran is None else ran
    maps, ref, count = _maps(sc, C, kind)
    view_sets = [[v] for v in range(sc.V)] if one_view else [None]
    got_c, got_o, got_v, ctrs = _blocking_calls(sc, maps, options, view_sets)           # 1. hit images, inside
    assert np.array_equal(got_c, count), label                                            # 2.
    assert np.array_equal(got_v, sc.views_hit()), label                                   # 3.
    split = np.zeros(sc.n_rows, bool)
    for views, ctr in zip(view_sets, ctrs):                                               # 4.
        assert ctr["bad_id"] == 0, ctr
        split |= ran(ctr, sc.counts(views))
    misses = sum(ctr["box_miss"] for ctr in ctrs)
    assert (misses > 0) == box_miss, (label, [ctr["box_miss"] for ctr in ctrs])
    print(f"{label}: {int(split.sum())} rows split, box misses {misses}, largest row {int(count.max())} pixels, counters {ctrs[0]}")
    assert_headroom(count, maps)                                                          # 5.
    assert_exact(got_o, ref, count, label, split=split)                                   # 6.
    if kind == "f16":                                                                     # 7.
        wide = _blocking_calls(sc, maps.astype(np.float32), options, view_sets)
        assert np.array_equal(wide[0], got_c) and np.array_equal(wide[2], got_v), label
        assert got_o.tobytes() == wide[1].tobytes(), f"{label}: fp16 maps must leave the bytes of the fp32 call on the widened values"
    return split, ctrs


# ------------------------------------------------------------------------------------------------------------------------------
# a. Multi-view calls: parts and k_combine_parts in every row variant
# ------------------------------------------------------------------------------------------------------------------------------
# k_gather / k_combine_parts <K, VEC, U>: fp32 C = 12 <1,4,4>; C = 520 <2,4,4>, the second pass ragged; C = 259 <4,1,4> scalar,
# two passes; C = 3 <4,1,4> below one pass and without the pixel code (C < 4); fp16 C = 520 and C = 8 <1,8,U>
ROWS = [("f32", 12), ("f32", 520), ("f32", 259), ("f32", 3), ("f16", 520), ("f16", 8)]
# V = 9: B * V >= 8 on a small image, views walked in groups of G = 4; largest voxel 479 pixels, 13 voxels above 64.
# V = 3: G = 1; largest voxel 927 pixels, 5 voxels above 64.
VIEWS = [(9, 71), (3, 78)]


@pytest.mark.parametrize("V,seed", VIEWS)
@pytest.mark.parametrize("kind,C", ROWS)
def test_multi_view_parts_leave_the_integer_sums(oracle_mod, kind, C, V, seed):
    sc = _room(oracle_mod, V, seed)
    split, _ = _check_role(f"a {kind} C={C} V={V} parts of 32 above 64", sc, C, kind, "parts")
    assert split.sum() >= 5 and sc.counts().max() >= 479


@pytest.mark.parametrize("kind,C", ROWS)
def test_multi_view_default_thresholds_split_nothing_here(oracle_mod, kind, C):
    """No option set: the threshold of a nine-view call is min(256 + 64 * 9, 2048) = 832 pixels, above this scene's largest voxel
    (479): one wavefront per voxel, the oracle's order and (tests/test_exact_maps_cpu.py) the oracle's bytes."""
    sc = _room(oracle_mod, 9, 71)
    assert sc.counts().max() < 832
    split, ctrs = _check_role(f"a {kind} C={C} V=9 default thresholds", sc, C, kind, "parts", options={},
                              ran=lambda ctr, c: _ran_parts(ctr, c, 832, 832))
    assert not split.any() and ctrs[0]["n_split"] == 0


# ------------------------------------------------------------------------------------------------------------------------------
# b. B = 2
# ------------------------------------------------------------------------------------------------------------------------------
def test_two_grids_in_one_call(oracle_mod):
    sc = _two_grids(oracle_mod)
    assert (sc.hits[0] > 0).any() and (sc.hits[1] > 0).any() and not np.array_equal(sc.hits[0], sc.hits[1])
    split, _ = _check_role("b two grids f32 C=12 parts of 32 above 64", sc, 12, "f32", "parts")
    assert split.sum() >= 5


# ------------------------------------------------------------------------------------------------------------------------------
# c. Boxes that miss pixels: the whole-image redo in every role and row variant
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["wave", "parts", "one_serial", "one_parts", "one_workgroup"])
@pytest.mark.parametrize("kind,C", [("f32", 12), ("f32", 520), ("f32", 259), ("f16", 520)])
def test_boxes_that_miss_pixels_are_redone_to_the_integer_sums(oracle_mod, kind, C, role):
    """Five rows of 1700 .. 2150 pixels whose boxes miss most of them: gather_voxel_wave's redo, the parts' shortfall and
    k_combine_parts' workgroup redo, k_gather_one's serial, part and workgroup redo."""
    sc = _redo_scene(oracle_mod)
    split, _ = _check_role(f"c {kind} C={C} {role}", sc, C, kind, role, box_miss=True)
    assert split.any() == (role not in ("wave", "one_serial")), role
    assert sc.counts().max() > 2000


@pytest.mark.parametrize("role", ["wave", "parts", "one_serial", "one_parts", "one_workgroup"])
@pytest.mark.parametrize("kind,C", [("f32", 12), ("f32", 520), ("f32", 259), ("f16", 520)])
def test_redone_and_added_voxels_side_by_side(oracle_mod, kind, C, role):
    """_mixed_scene: in the roles that split, the workgroups of k_combine_parts redo five voxels over whole images and add the
    parts of the others, one after the other through the same LDS rows; the counters must show both (fewer box misses than split
    voxels in the multi-view call)."""
    sc = _mixed_scene(oracle_mod)
    split, ctrs = _check_role(f"c mixed {kind} C={C} {role}", sc, C, kind, role, box_miss=True)
    assert split.any() == (role not in ("wave", "one_serial")), role
    if role == "parts":
        assert ctrs[0]["box_miss"] == 5 and ctrs[0]["n_split"] == 14, ctrs
    if role == "one_parts":
        assert any(0 < ctr["box_miss"] < ctr["n_split"] for ctr in ctrs), ctrs


# ------------------------------------------------------------------------------------------------------------------------------
# d. One-view calls, three per case, accumulating into one out
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["one_serial", "one_parts", "one_workgroup"])
@pytest.mark.parametrize("kind,C", [("f32", 12), ("f32", 259), ("f16", 520)])
def test_one_view_calls_accumulate_the_integer_sums(oracle_mod, kind, C, role):
    sc = _room(oracle_mod, 3, 78)
    split, ctrs = _check_role(f"d {kind} C={C} {role}", sc, C, kind, role)
    if role == "one_serial":
        assert not split.any()
    else:
        assert all(ctr["n_heavy"] > 5 for ctr in ctrs), ctrs             # every view moves voxels out of the one-wavefront deal


# ------------------------------------------------------------------------------------------------------------------------------
# e. One-view calls with device-sized parts
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "f16"])
@pytest.mark.parametrize("W,H", [(640, 416), (512, 384)])
def test_one_view_device_sized_parts(oracle_mod, W, H, kind):
    """No option set: k_worklist sizes the parts from the view's hit total, part_px = max(32, ceil(2 * n_hit / 8192)), and cuts
    above twice that -- but not below 256 pixels on a view of at most 262144 pixels (512 x 384; 640 x 416 has no floor: 266203
    hits, parts of 65 pixels above 130, the largest voxel 10108 pixels)."""
    sc = _room(oracle_mod, 1, 71, W, H)
    n_hit = int(sc.counts().sum())
    px = max(32, -(-2 * n_hit // 8192))
    T = 2 * px if W * H > 262144 else max(2 * px, 256)
    if (W, H) == (640, 416):
        assert (n_hit, px, T, int(sc.counts().max())) == (266203, 65, 130, 10108)

    def ran(ctr, c):
        assert ctr["n_hit"] == n_hit, ctr
        mask = _ran_parts(ctr, c, T, px)
        assert ctr["n_split"] > 20 and ctr["n_parts"] <= 8192, ctr
        return mask

    _check_role(f"e {kind} C=8 {W}x{H} device-sized parts", sc, 8, kind, "one_parts", options={}, ran=ran)


# ------------------------------------------------------------------------------------------------------------------------------
# f. The part-slot bound
# ------------------------------------------------------------------------------------------------------------------------------
def test_part_slot_bound_raises_the_part_size(oracle_mod):
    """Rows of 32 KiB (C = 8192): 128 MiB of partial rows are 4096 slots, and the 49152 pixel-halves of this call (V = 8, 64 x 48)
    asked for parts of 6 pixels are raised to ceil(2 * 24576 / 4096) = 12 (test_gpu_trajectory.py).  fp32 maps: numpy converts and
    compares binary16 in software, so on the host the fp16 form of this case is the slower one, about twice."""
    import voxproj_host as vh
    sc = _room(oracle_mod, 8, 91, 64, 48)
    C = 8192
    maps = exact_maps(sc.V, sc.H, sc.W, C, seed=92)[None]
    ref, count = int_reference(sc.hits, maps, sc.n_rows)
    got_c, got_o, got_v, ctrs = _blocking_calls(sc, maps, {vh.VP_OPT_HEAVY_THRESHOLD: 6, vh.VP_OPT_PART_PIXELS: 6}, [None])
    assert np.array_equal(got_c, count)
    assert np.array_equal(got_v, sc.views_hit())
    bound = -(-2 * sc.V * sc.H * sc.W // 4096)
    assert bound == 12 and ctrs[0]["part_px"] == bound > 6
    split = _ran_parts(ctrs[0], count, bound, bound)
    assert ctrs[0]["bad_id"] == 0 and ctrs[0]["box_miss"] == 0 and 50 < ctrs[0]["n_split"] and ctrs[0]["n_parts"] <= 4096, ctrs
    assert_headroom(count, maps)
    assert_exact(got_o, ref, count, "f f32 C=8192 slot bound", split=split)


# ------------------------------------------------------------------------------------------------------------------------------
# g. A call sequence on one workspace
# ------------------------------------------------------------------------------------------------------------------------------
def test_a_call_sequence_on_one_workspace_adds_up_exactly(oracle_mod):
    """Heavy threshold 6 (most voxels are cut), one Workspace, one count / out / views_hit:
      1. a pipelined call of views 0..8 on rows [0, h);  2. its gather-only call for [h, n_rows);  3. the whole call again,
      pipelined;  4. workspace_status;  5. a blocking one-view call of view 9;  6. a blocking call of views 9..11, C unchanged.
    The reference is the int64 sum of all of them: a part slot, counter or list left by an earlier call shows as an integer
    difference in a named row."""
    import voxproj_host as vh
    dev = torch.device(DEV)
    C = 12
    sc = _room(oracle_mod, 12, 71)
    maps, _, _ = _maps(sc, C, "f32")
    n_rows = sc.n_rows
    nine, one, three = list(range(9)), [9], [9, 10, 11]
    ref, count, views_ref = np.zeros((n_rows, C), np.int64), np.zeros(n_rows, np.int64), np.zeros(n_rows, np.int64)
    split = np.zeros(n_rows, bool)
    for views, times in ((nine, 2), (one, 1), (three, 1)):
        r, c = int_reference(sc.hits[:, views], maps[:, views], n_rows)
        assert np.array_equal(c, sc.counts(views))
        ref += times * r
        count += times * c
        views_ref += times * sc.views_hit(views)
        split |= c > 6

    def tensors(views):
        return (torch.from_numpy(np.ascontiguousarray(maps[:, views])).to(dev),
                torch.from_numpy(np.ascontiguousarray(sc.c2w[views])).reshape(-1).to(dev))

    occ_t, intr_t = torch.from_numpy(sc.occ).to(dev), torch.from_numpy(sc.intr).to(dev)
    t9, t1, t3 = tensors(nine), tensors(one), tensors(three)
    count_t = torch.zeros(n_rows, dtype=torch.int32, device=dev)
    out_t = torch.zeros(n_rows, C, device=dev)
    views_t = torch.zeros(n_rows, dtype=torch.int32, device=dev)
    ws = vh.Workspace()
    ws.set_option(vh.VP_OPT_HEAVY_THRESHOLD, 6)

    def call(t, **kw):
        vh.project_features_raw(t[0], occ_t, t[1], intr_t, [float(x) for x in sc.s.opts()], count_t, out_t,
                                [float(x) for x in sc.s.grid_origin], sc.s.voxel_size, workspace=ws, views_hit=views_t, **kw)

    def hits_are(views):
        assert np.array_equal(vh.hit_image(ws, dev).cpu().numpy(), sc.hits[:, views]), f"hit image of the call of views {views}"

    torch.cuda.synchronize()
    h = n_rows // 3
    ws.set_row_range(0, h)
    call(t9, sync=False, pipeline=True)                                   # 1.
    ws.set_row_range(h, n_rows)
    call(t9, sync=False, pipeline=True, gather_only=True)                 # 2.
    ws.set_row_range()
    call(t9, sync=False, pipeline=True)                                   # 3.
    vh.workspace_status(ws, dev)                                          # 4.
    hits_are(nine)
    ctrs = [vh.counters(ws, dev)]
    call(t1, sync=True)                                                   # 5.
    hits_are(one)
    ctrs.append(vh.counters(ws, dev))
    call(t3, sync=True)                                                   # 6.
    hits_are(three)
    ctrs.append(vh.counters(ws, dev))
    got_c, got_o, got_v = count_t.cpu().numpy(), out_t.cpu().numpy(), views_t.cpu().numpy()
    ws.release()
    assert np.array_equal(got_c, count)
    assert np.array_equal(got_v, views_ref)
    # multi-view calls: parts of heavy_t = 6 pixels above 6; the one-view call: parts of ceil(6 / 2) = 3 above 6
    for ctr, views, px in zip(ctrs, (nine, one, three), (6, 3, 6)):
        assert ctr["bad_id"] == 0 and ctr["box_miss"] == 0, ctr
        assert _ran_parts(ctr, sc.counts(views), 6, px).sum() > 30
    print(f"g: {int(split.sum())} rows split by some call, largest row {int(count.max())} pixels over the sequence, counters {ctrs}")
    assert_headroom(count, maps)
    assert_exact(got_o, ref, count, "g call sequence f32 C=12", split=split)


# ------------------------------------------------------------------------------------------------------------------------------
# h. More split voxels in one call than k_combine_parts has workgroups
# ------------------------------------------------------------------------------------------------------------------------------
# k_combine_parts runs on min(512, slot_cap / 2) workgroups that take the call's split voxels j, j + 512, ...: voxels 512 and
# later are some workgroup's SECOND lap.  A close-up frame has hundreds of split voxels; the scenes above have a few dozen.  Here
# 8000 voxels are seen at 160 x 120 and cut above 12 pixels into parts of 5: every call below that claims it has more than 512
# split voxels, the 8001 (1501) rows are binned by two (one) workgroups of k_worklist, and the split list is in the order the
# atomics handed its entries out -- which voxels land beyond entry 512 differs from run to run, that some do does not.
LAP = 512                         # COMBINE_BLOCKS (csrc/vp_gather.h); slot_cap / 2 is 4096 or more in every call here
LAP_ROWS = [("f32", 12), ("f32", 259), ("f16", 520)]        # <1,4,4>; scalar, two channel passes; fp16, two channel passes


def _close_up(oracle_mod):
    """8000 voxels with IDs of their own (8001 rows), three views of 160 x 120: 671 / 535 / 318 voxels above 12 pixels in views
    0 / 1 / 2 (3542 / 2795 / 3102 parts of 5), 1524 over the three views together (9439 parts, the largest row 479 pixels)."""
    if "close_up" not in _scenes:
        s = make_scene(8000, 3, 160, 120, seed=71, room=ROOM)
        _scenes["close_up"] = _Scene(oracle_mod, "close_up", s, s.occ[None].astype(np.int64), s.c2w, s.intr[None], 1, s.n_vox + 1)
    return _scenes["close_up"]


def _close_up_redo(oracle_mod):
    """The same cells under 1500 IDs (occ % 1500 + 1, 1501 rows, about five cells per ID as in _redo_scene): the box around one
    cell of an ID misses the others' pixels.  1134 rows above 12 pixels over the three views, 556 / 556 / 340 per view."""
    if "close_up_redo" not in _scenes:
        s = _close_up(oracle_mod).s
        occ = np.where(s.occ > 0, (s.occ % 1500) + 1, 0).astype(np.int64)[None]
        _scenes["close_up_redo"] = _Scene(oracle_mod, "close_up_redo", s, occ, s.c2w, s.intr[None], 1, 1501)
    return _scenes["close_up_redo"]


def _multi_view_parts_of_5(vh):
    return {vh.VP_OPT_HEAVY_THRESHOLD: 12, vh.VP_OPT_PART_PIXELS: 5}, lambda ctr, c: _ran_parts(ctr, c, 12, 5)


def _say(label, ctrs):
    print(f"{label}: " + "; ".join(f"n_split {c['n_split']}, n_parts {c['n_parts']}, box_miss {c['box_miss']}" for c in ctrs))


@pytest.mark.parametrize("kind,C", LAP_ROWS)
def test_one_view_calls_with_more_split_voxels_than_combine_workgroups(oracle_mod, kind, C):
    """The adding arm, one view per call: part_px = 5 survives the slot bound (ceil(2 * 19200 / 8192) = 5), no box misses a
    pixel, and views 0 and 1 each leave more than 512 voxels to add (the oracle counts 671 and 535; _ran_parts holds the
    counters to the oracle's numbers)."""
    sc = _close_up(oracle_mod)
    assert sc.n_rows == 8001 and [int((sc.counts([v]) > 12).sum()) for v in range(3)] == [671, 535, 318]
    split, ctrs = _check_role(f"h {kind} C={C} one view, parts of 5 above 12", sc, C, kind, "one_parts")
    _say(f"h {kind} C={C} one view", ctrs)
    assert ctrs[0]["n_split"] > LAP and ctrs[1]["n_split"] > LAP and all(ctr["box_miss"] == 0 for ctr in ctrs), ctrs
    assert [ctr["n_parts"] for ctr in ctrs] == [3542, 2795, 3102]


@pytest.mark.parametrize("kind,C", LAP_ROWS)
def test_multi_view_call_with_more_split_voxels_than_combine_workgroups(oracle_mod, kind, C):
    """The adding arm, the three views in one call (k_gather's parts): 1524 split voxels, three laps of k_combine_parts."""
    import voxproj_host as vh
    sc = _close_up(oracle_mod)
    options, ran = _multi_view_parts_of_5(vh)
    split, ctrs = _check_role(f"h {kind} C={C} three views, parts of 5 above 12", sc, C, kind, "parts", options=options, ran=ran)
    _say(f"h {kind} C={C} three views", ctrs)
    assert ctrs[0]["n_split"] == 1524 > 2 * LAP and ctrs[0]["n_parts"] == 9439 and ctrs[0]["box_miss"] == 0, ctrs
    assert int(sc.counts().max()) == 479


def test_whole_image_redos_beyond_the_first_lap_of_the_combine(oracle_mod):
    """The redo arm, fp32 C = 12.  Three views in one call: more than 512 of the 1134 split rows have parts that found fewer
    pixels than the march counted, so by pigeonhole a workgroup of k_combine_parts redoes at least one of them over whole
    images in its second or third lap, whatever order the split list came out in.  One view per call: more than 512 split rows
    in views 0 and 1, redone and added rows side by side."""
    import voxproj_host as vh
    sc = _close_up_redo(oracle_mod)
    assert sc.n_rows == 1501 and int((sc.counts() > 12).sum()) == 1134
    assert [int((sc.counts([v]) > 12).sum()) for v in range(3)] == [556, 556, 340]
    options, ran = _multi_view_parts_of_5(vh)
    _, ctrs = _check_role("h redo f32 C=12 three views", sc, 12, "f32", "parts", box_miss=True, options=options, ran=ran)
    _say("h redo f32 C=12 three views", ctrs)
    assert ctrs[0]["n_split"] == 1134 and ctrs[0]["n_parts"] == 11515 and ctrs[0]["box_miss"] > LAP, ctrs
    # box_miss also counts the rows of up to 12 pixels that their one wavefront redoes (k_gather): at most all of them
    light = int(((sc.counts() > 0) & (sc.counts() <= 12)).sum())
    print(f"h redo three views: {light} rows of 1 .. 12 pixels, so at least {ctrs[0]['box_miss'] - light} split rows were redone")
    assert ctrs[0]["box_miss"] - light > LAP, (ctrs, light)
    _, ctrs = _check_role("h redo f32 C=12 one view", sc, 12, "f32", "one_parts", box_miss=True)
    _say("h redo f32 C=12 one view", ctrs)
    assert ctrs[0]["n_split"] > LAP and ctrs[1]["n_split"] > LAP and all(ctr["box_miss"] > 0 for ctr in ctrs), ctrs


def test_job_mode_leaves_the_blocking_calls_bytes_beyond_the_first_lap(oracle_mod):
    """A blocking one-view call launches k_combine_parts only when the gather's first wavefront notes split voxels to the host
    (project_gather_one, csrc/vp_project.h); job mode always launches it.  Both must leave the same bytes: each view of the
    close-up as a job on a workspace of its own, all adding into one out, against the three blocking calls."""
    import voxproj_host as vh
    dev = torch.device(DEV)
    sc = _close_up(oracle_mod)
    options = _role(vh, "one_parts")[0]
    maps, ref, count = _maps(sc, 12, "f32")
    want_c, want_o, want_v, want_ctrs = _blocking_calls(sc, maps, options, [[v] for v in range(sc.V)])
    assert_exact(want_o, ref, count, "h blocking f32 C=12 one view", split=count > 12)
    count_t = torch.zeros(sc.n_rows, dtype=torch.int32, device=dev)
    out_t = torch.zeros(sc.n_rows, 12, device=dev)
    views_t = torch.zeros(sc.n_rows, dtype=torch.int32, device=dev)
    occ_t, intr_t = torch.from_numpy(sc.occ).to(dev), torch.from_numpy(sc.intr).to(dev)
    ctrs = []
    for v in range(sc.V):
        ws = vh.Workspace()
        for opt, val in options.items():
            ws.set_option(opt, val)
        feats, c2w = torch.from_numpy(np.ascontiguousarray(maps[:, [v]])).to(dev), torch.from_numpy(sc.c2w[[v]]).reshape(-1).to(dev)
        vh.project_features_raw(feats, occ_t, c2w, intr_t, [float(x) for x in sc.s.opts()], count_t, out_t,
                                [float(x) for x in sc.s.grid_origin], sc.s.voxel_size, workspace=ws, sync=False, pipeline=True,
                                views_hit=views_t)
        vh.workspace_status(ws, dev)
        assert np.array_equal(vh.hit_image(ws, dev).cpu().numpy(), sc.hits[:, [v]])
        ctrs.append(vh.counters(ws, dev))
        ws.release()
    _say("h job mode f32 C=12 one view", ctrs)
    assert [(c["n_split"], c["n_parts"], c["box_miss"]) for c in ctrs] == [(c["n_split"], c["n_parts"], c["box_miss"]) for c in want_ctrs]
    assert ctrs[0]["n_split"] > LAP and ctrs[1]["n_split"] > LAP
    assert np.array_equal(count_t.cpu().numpy(), want_c) and np.array_equal(views_t.cpu().numpy(), want_v)
    assert out_t.cpu().numpy().tobytes() == want_o.tobytes()


# ------------------------------------------------------------------------------------------------------------------------------
# i. The march's hit counters, cleared beyond the first lap of k_zero_call
# ------------------------------------------------------------------------------------------------------------------------------
def _pulled_back(oracle_mod):
    """The close-up's cells under 1000 IDs (1001 rows: ONE workgroup of k_zero_call, 256 threads) and two views of 160 x 120
    (80 tiles of 16 x 16, 320 hit counters): view 0 of the close-up, inside the room, and a camera 5.5 m in front of the room's
    -x wall, to which the room is some forty pixels in the image centre."""
    if "pulled_back" not in _scenes:
        s = _close_up(oracle_mod).s
        occ = np.where(s.occ > 0, (s.occ % 1000) + 1, 0).astype(np.int64)[None]
        back = np.zeros((4, 4), np.float32)         # looks along +x: x right = -y of the world, y down = -z
        back[:3, 0], back[:3, 1], back[:3, 2], back[:3, 3], back[3, 3] = (0, -1, 0), (0, 0, -1), (1, 0, 0), (-8.0, 0.0, 1.2), 1.0
        _scenes["pulled_back"] = _Scene(oracle_mod, "pulled_back", s, occ, np.stack([s.c2w[0], back]), s.intr[None], 1, 1001)
    return _scenes["pulled_back"]


def test_hit_counters_of_the_previous_call_are_cleared_beyond_the_first_lap(oracle_mod):
    """A one-view call with no part option sizes its parts from the view's hit total, which k_worklist adds up from one counter
    per wavefront of the march (4 per 16 x 16 tile).  A wavefront without a hit never writes its counter, so k_zero_call clears
    them all -- on a grid sized by n_rows: here 256 threads for 320 counters, a second lap for the counters of tiles 64 .. 79.
    View 0 hits in those tiles; the second call, on the SAME workspace, has hits but none in some of them: a counter left from
    the first call would inflate its n_hit.  Both calls: the oracle's hit image and hit total, the device's part size, exact
    rows; the second call equal to itself on a fresh workspace.  (part_t: twice the part size, but not below 256 pixels on a view
    of at most 262144 pixels -- csrc/vp_plan.h, as in section e.)"""
    import voxproj_host as vh
    dev = torch.device(DEV)
    sc = _pulled_back(oracle_mod)
    C, W, H = 12, sc.W, sc.H
    tx, ty = -(-W // 16), -(-H // 16)
    assert sc.n_rows <= 1024 and 4 * tx * ty == 320 > 256 * -(-sc.n_rows // 1024)           # the clearing loop laps
    per_tile = []
    for v in range(2):
        pad = np.zeros((ty * 16, tx * 16), bool)
        pad[:H, :W] = sc.hits[0, v] > 0
        per_tile.append(pad.reshape(ty, 16, tx, 16).sum(axis=(1, 3)).reshape(-1))          # tile index = ty * tiles per line + tx
    stale = np.nonzero((per_tile[0] > 0) & (per_tile[1] == 0))[0]
    n_hits = [int(t.sum()) for t in per_tile]
    print(f"i: hits {n_hits} of {W * H} pixels; tiles the first view hits and the second does not: {stale.tolist()}")
    assert n_hits[0] > 0.95 * W * H and n_hits[1] > 0 and (stale >= 64).any()
    maps, _, _ = _maps(sc, C, "f32")
    occ_t, intr_t = torch.from_numpy(sc.occ).to(dev), torch.from_numpy(sc.intr).to(dev)

    def call(ws, v):
        count_t = torch.zeros(sc.n_rows, dtype=torch.int32, device=dev)
        out_t = torch.zeros(sc.n_rows, C, device=dev)
        views_t = torch.zeros(sc.n_rows, dtype=torch.int32, device=dev)
        vh.project_features_raw(torch.from_numpy(np.ascontiguousarray(maps[:, [v]])).to(dev), occ_t,
                                torch.from_numpy(sc.c2w[[v]]).reshape(-1).to(dev), intr_t, [float(x) for x in sc.s.opts()], count_t, out_t,
                                [float(x) for x in sc.s.grid_origin], sc.s.voxel_size, workspace=ws, sync=True, views_hit=views_t)
        assert np.array_equal(vh.hit_image(ws, dev).cpu().numpy(), sc.hits[:, [v]]), f"hit image of view {v}"
        return count_t.cpu().numpy(), out_t.cpu().numpy(), views_t.cpu().numpy(), vh.counters(ws, dev)

    ws, fresh = vh.Workspace(), vh.Workspace()
    first, second, alone = call(ws, 0), call(ws, 1), call(fresh, 1)
    ws.release()
    fresh.release()
    for v, (got_c, got_o, got_v, ctr) in ((0, first), (1, second), (1, alone)):
        ref, count = int_reference(sc.hits[:, [v]], maps[:, [v]], sc.n_rows)
        print(f"i: view {v}: counters {ctr}")
        assert ctr["n_hit"] == n_hits[v] == int(count.sum()), (ctr, n_hits[v])
        px = max(32, -(-2 * n_hits[v] // 8192))
        split = _ran_parts(ctr, count, max(2 * px, 256), px)
        assert ctr["bad_id"] == 0, ctr
        assert np.array_equal(got_c, count) and np.array_equal(got_v, sc.views_hit([v]))
        assert_headroom(count, maps)
        assert_exact(got_o, ref, count, f"i view {v}", split=split)
    assert second[3] == alone[3], (second[3], alone[3])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(second[:3], alone[:3]))
