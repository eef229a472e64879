"""The mesh rasterizer on the GPU (vp_mesh_project + vp_mesh_rasterize) against its NumPy twin (tests/mesh_reference.py):
face ids, the bits of the depth, labels and drop counters are compared exactly, at the smallest shapes that take every path
(partial tiles, one tile, one pixel, runs longer than one LDS staging, a face in every tile, clipped faces)."""
import ctypes

import numpy as np
import pytest
import torch

import mesh_reference as mr
import mesh_scenes as ms

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_twins = {}


def _scene(name):
    """(verts, faces, labels, viewmat, K, W, H) of a named case; generated once."""
    kind, _, arg = name.partition(":")
    if kind == "room":
        seed, W, H = (int(v) for v in arg.split(","))
        return ms.room(seed) + (ms.room_camera(seed), ms.intrinsics(W, H), W, H)
    if kind == "room_offcentre":                         # fx != fy and a principal point off the centre
        return ms.room(1) + (ms.room_camera(1), ms.intrinsics(70, 45, fx=61.3, fy=48.9, cx=29.25, cy=30.5), 70, 45)
    if kind == "tiny":
        return ms.tiny_faces() + (np.eye(4, dtype=np.float32), ms.intrinsics(64, 48), 64, 48)
    if kind == "whole":
        return ms.whole_image_face() + (np.eye(4, dtype=np.float32), ms.intrinsics(96, 64), 96, 64)
    if kind == "quad":
        return ms.diagonal_quad(swap=arg == "swap") + ms.exact_camera() + (12, 12)
    if kind == "coincident":
        return ms.coincident_faces() + ms.exact_camera() + (24, 24)
    raise KeyError(name)


def _twin(name):
    if name not in _twins:
        s = _scene(name)
        _twins[name] = (s, mr.render(*s))
    return _twins[name]


def _gpu(s, **kw):
    import voxproj_host as vh
    v, f, l, vm, K, W, H = s
    ids, depth, labels, counters = vh.mesh_render(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV),
                                                  torch.from_numpy(l).to(DEV), vm, K, W, H, **kw)
    return dict(face_ids=ids.cpu().numpy(), depth=depth.cpu().numpy(), labels=labels.cpu().numpy(),
                counters=counters.cpu().numpy())


def _same(got, want):
    assert np.array_equal(got["face_ids"], want["face_ids"]), int((got["face_ids"] != want["face_ids"]).sum())
    assert got["depth"].dtype == np.float32 and got["depth"].tobytes() == want["depth"].tobytes()
    assert np.array_equal(got["labels"], want["labels"])
    assert np.array_equal(got["counters"], want["counters"])


@pytest.mark.parametrize("name", ["room:0,96,64", "room:1,96,64", "room:2,96,64", "room:3,96,64", "room:0,70,45", "room:1,16,16",
                                  "room:2,1,1", "room_offcentre", "tiny", "whole", "quad", "quad:swap", "coincident"])
def test_maps_equal_the_twin_bit_for_bit(name):
    s, want = _twin(name)
    got = _gpu(s)
    _same(got, want)
    if name.startswith("room"):
        assert (got["face_ids"] >= 0).all()                  # a closed room leaves no pixel uncovered
    if name == "tiny":                                       # the case does what it is for
        assert (np.bincount(want["face_ids"][want["face_ids"] >= 0], minlength=20000) == 0).sum() > 5000
    if name == "whole":
        assert (got["face_ids"] == 0).all() and (got["labels"] == 9).all()
    if name == "coincident":
        assert set(np.unique(got["face_ids"])) == {-1, 0}


def test_tiny_faces_fill_more_than_one_lds_staging_per_tile():
    import voxproj_host as vh
    v, f, l, vm, K, W, H = _scene("tiny")
    ws = vh.SplatWorkspace()
    n = int(vh.mesh_project(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), vm, K, W, H, workspace=ws).item())
    assert n > 3 * 256 * 12                                  # 12 tiles: runs of several batches of 256 records on average


def test_shared_diagonal_is_owned_by_geometry_not_by_order():
    a, b = _gpu(_scene("quad")), _gpu(_scene("quad:swap"))
    inside = np.zeros((12, 12), bool)
    inside[2:10, 2:10] = True
    assert ((a["face_ids"] >= 0) == inside).all()
    assert np.array_equal(a["face_ids"][inside], 1 - b["face_ids"][inside])      # the same triangle, under its other index
    assert a["depth"].tobytes() == b["depth"].tobytes()


def _bad_mesh():
    """A room with faces that must be dropped, each kind a known number of times, and indices that would read far outside
    the vertices if they were used: (verts, faces, labels, viewmat)."""
    v, f, l = ms.room(0)
    vm = ms.room_camera(0)
    f = f.copy()
    n = len(v)
    f[5] = [0, 1, 2 ** 31 - 1]
    f[6] = [-5, 1, 2]
    f[7] = [n + 5, 3, 4]
    f[100] = [1, -2 ** 31, 7]
    # a face just in front of the near plane whose first vertex projects 10^12 sub-pixel units out, given in camera space
    guard = (np.array([[1e6, 0.5, 0.02], [0.1, 0.1, 0.5], [0.2, 0.1, 0.5]]) - vm[:3, 3].astype(np.float64)) @ vm[:3, :3].astype(np.float64)
    extra = np.concatenate([np.array([[np.nan, 0, 0], [0, np.inf, 1]]), guard]).astype(np.float32)
    more = np.array([[n, 1, 2], [3, n + 1, 4], [n + 2, n + 3, n + 4]], np.int32)        # NaN, inf, guard band
    return np.concatenate([v, extra]), np.concatenate([f, more]), np.concatenate([l, np.array([1, 2, 3, 4, 5], np.uint8)]), vm


def test_every_drop_counter():
    s = _bad_mesh() + (ms.intrinsics(96, 64), 96, 64)
    want = mr.render(*s)
    assert want["counters"].tolist() == [4, 2, 1]
    _same(_gpu(s), want)


def test_counters_accumulate_and_may_be_absent():
    import voxproj_host as vh
    v, f, l, vm = _bad_mesh()
    tv, tf = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    c = torch.tensor([10, 20, 30], dtype=torch.int32, device=DEV)
    ws = vh.SplatWorkspace()
    a = vh.mesh_project(tv, tf, vm, ms.intrinsics(96, 64), 96, 64, workspace=ws, counters=c)
    b = vh.mesh_project(tv, tf, vm, ms.intrinsics(96, 64), 96, 64, workspace=ws)
    assert c.tolist() == [14, 22, 31] and int(a.item()) == int(b.item())


COUNTER_LAP = 256 * 256         # k_mesh_counters: one workgroup, thread t adds the workgroups t, t + 256, ..; 256 faces each


def _padded_room():
    """room(0) with its faces split round 64 522 faces that lie behind the near plane (the twin and mesh_setup leave them
    after the depth test of their vertices), so that the mesh has more than 65 536 faces: k_mesh_project runs more than 256
    workgroups and every thread of k_mesh_counters that serves one of the workgroups 256.. takes a second lap.  Every dropped
    face (5 bad indices, 3 non-finite, 2 guard band) has an index >= 65 536, in the workgroups 256 and 260."""
    v, f, l = ms.room(0)
    vm = ms.room_camera(0)
    n = len(v)
    R, t = vm[:3, :3].astype(np.float64), vm[:3, 3].astype(np.float64)
    world = lambda cam: (np.asarray(cam, np.float64) - t) @ R  # noqa: E731   (camera space -> world)
    behind = world([[0.3, 0.2, -1.0], [-0.4, 0.1, -1.5], [0.1, -0.3, -2.0]])
    guard = world([[1e6, 0.5, 0.02], [0.1, 0.1, 0.5], [0.2, 0.1, 0.5]])       # _bad_mesh's face: 10^12 sub-pixel units out
    verts = np.concatenate([v, behind, [[np.nan, 0, 0], [0, np.inf, 1]], guard]).astype(np.float32)
    nv = len(verts)
    even, odd = f[::2], f[1::2]                              # both halves hold faces of every wall
    half = len(even)
    pad = np.tile(np.array([[n, n + 1, n + 2]], np.int32), (COUNTER_LAP - half, 1))
    drop_a = np.array([[nv, 1, 2], [-5, 1, 2], [n + 3, 1, 2], [n + 5, n + 6, n + 7]], np.int32)
    drop_b = np.array([[1, -2 ** 31, 7], [0, 1, 2 ** 31 - 1], [nv + 9, nv, -1], [3, n + 4, 4], [n + 3, n + 4, 0],
                       [n + 6, n + 7, n + 5]], np.int32)
    faces = np.concatenate([even, pad, drop_a, odd, pad[:7], drop_b])
    assert len(faces) > COUNTER_LAP and half + len(pad) == COUNTER_LAP
    assert (len(faces) + 255) // 256 == 261 and len(faces) % 256 not in (0, 255)
    labels = np.concatenate([l, np.arange(1, nv - n + 1, dtype=np.uint8)])
    return verts, faces, labels, vm


def test_more_than_65536_faces_and_counters_from_the_second_lap():
    s = _padded_room() + (ms.intrinsics(96, 64), 96, 64)
    want = mr.render(*s)
    assert want["counters"].tolist() == [5, 3, 2]
    assert not mr.render(s[0], s[1][:COUNTER_LAP], *s[2:])["counters"].any()          # none of them in the first lap
    seen = np.unique(want["face_ids"])
    assert seen.min() >= 0 and (seen < 1014).sum() > 20 and (seen > COUNTER_LAP).sum() > 20      # drawn faces on both sides
    _same(_gpu(s), want)


def test_padding_beyond_two_strides_of_the_emit_kernel():
    """k_tile_emit pads the slots [total, capacity) with a stride of gridDim * 256 = 256 * ceil(n_faces / 256) slots: 2048 for
    the 2028 faces of a room.  A spare capacity of 2 * 2048 + 500 gives some threads a third lap, on a workspace whose every
    byte is 0xA5: a slot left unpadded holds the key 0xA5A5A5A5, whose low bits sort it among the real ones."""
    import voxproj_host as vh
    s, want = _twin("room:3,96,64")
    W, H = s[5], s[6]
    stride = 256 * ((len(s[1]) + 255) // 256)
    assert stride == 2048
    runs = []
    for spare in (0, 2 * stride + 500):
        ws = vh.SplatWorkspace()
        ws.ensure(64 << 20, DEV)
        ws.buf.fill_(0xA5)
        (tv, tf, tl), n = _project(s, ws)
        ids, depth, labels = vh.mesh_rasterize(tf, tl, W, H, n + spare, ws)
        runs.append(dict(face_ids=ids.cpu().numpy(), depth=depth.cpu().numpy(), labels=labels.cpu().numpy(),
                         counters=want["counters"]))
    for k in ("face_ids", "depth", "labels"):
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k
    _same(runs[1], want)


def test_no_faces_draw_nothing():
    s = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros(0, np.uint8), np.eye(4, dtype=np.float32),
         ms.intrinsics(40, 20), 40, 20)
    got = _gpu(s)
    assert (got["face_ids"] == -1).all() and (got["depth"] == 0).all() and (got["labels"] == 255).all()
    assert not got["counters"].any()


def _project(s, ws):
    import voxproj_host as vh
    v, f, l, vm, K, W, H = s
    t = (torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), torch.from_numpy(l).to(DEV))
    return t, int(vh.mesh_project(t[0], t[1], vm, K, W, H, workspace=ws).item())


def test_capacity_one_short_writes_nothing_and_raises_the_status():
    import voxproj_host as vh
    s, want = _twin("room:0,70,45")
    W, H = s[5], s[6]
    ws = vh.SplatWorkspace()
    (tv, tf, tl), n = _project(s, ws)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = (torch.full((H, W), 77, dtype=torch.int32, device=DEV), torch.full((H, W), 7.5, device=DEV),
           torch.full((H, W), 99, dtype=torch.uint8, device=DEV))
    vh.mesh_rasterize(tf, tl, W, H, n - 1, ws, status=status, out=out)
    assert int(status.item()) == 1
    assert (out[0] == 77).all() and (out[1] == 7.5).all() and (out[2] == 99).all()
    status.zero_()
    ids, depth, labels = vh.mesh_rasterize(tf, tl, W, H, n, ws, status=status, out=out)
    assert int(status.item()) == 0
    _same(dict(face_ids=ids.cpu().numpy(), depth=depth.cpu().numpy(), labels=labels.cpu().numpy(), counters=want["counters"]), want)


def test_spare_capacity_recycled_workspace_and_second_run_give_the_same_bits():
    import voxproj_host as vh
    s, want = _twin("room:3,96,64")
    W, H = s[5], s[6]
    big = vh.SplatWorkspace()
    big.ensure(64 << 20, DEV)
    big.buf.fill_(0xA5)                                      # a recycled, larger buffer full of something else
    runs = []
    for ws, spare in ((vh.SplatWorkspace(), 0), (vh.SplatWorkspace(), 1000), (big, 37), (big, 0)):
        (tv, tf, tl), n = _project(s, ws)
        ids, depth, labels = vh.mesh_rasterize(tf, tl, W, H, n + spare, ws)
        runs.append(dict(face_ids=ids.cpu().numpy(), depth=depth.cpu().numpy(), labels=labels.cpu().numpy(),
                         counters=want["counters"]))
    for r in runs:
        _same(r, want)


@pytest.mark.parametrize("size,n_tiles", [((1, 1), 1), ((16, 16), 1), ((17, 16), 2), ((64, 64), 16), ((128, 32), 16),
                                          ((61, 47), 12), ((256, 256), 256)])
def test_tile_counts_around_the_extra_key_bit(size, n_tiles):
    """The padding key of the sort is n_tiles, which needs a bit that n_tiles - 1 does not need exactly when n_tiles is a
    power of two: an end bit one short would sort the padding of a spare capacity among the keys of tile 0.  Exact capacity,
    then 300 spare slots on a workspace whose every byte is 0xA5; both equal the twin bit for bit."""
    import voxproj_host as vh
    W, H = size
    tx, ty = (W + 15) // 16, (H + 15) // 16
    assert tx * ty == n_tiles
    s, want = _twin(f"room:1,{W},{H}")
    last = want["face_ids"][16 * (ty - 1):, 16 * (tx - 1):]
    assert last.size > 0 and (last >= 0).all(), "the last tile should hold drawn faces"
    dirty = vh.SplatWorkspace()
    dirty.ensure(8 << 20, DEV)
    dirty.buf.fill_(0xA5)
    total = None
    for ws, spare in ((vh.SplatWorkspace(), 0), (dirty, 300)):
        (tv, tf, tl), n = _project(s, ws)
        assert n >= n_tiles and total in (None, n)
        total = n
        ids, depth, labels = vh.mesh_rasterize(tf, tl, W, H, n + spare, ws)
        _same(dict(face_ids=ids.cpu().numpy(), depth=depth.cpu().numpy(), labels=labels.cpu().numpy(),
                   counters=want["counters"]), want)


def test_depth_and_ids_without_labels():
    import voxproj_host as vh
    s, want = _twin("room:1,16,16")
    v, f, l, vm, K, W, H = s
    ids, depth, labels, _ = vh.mesh_render(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), None, vm, K, W, H)
    assert labels is None and np.array_equal(ids.cpu().numpy(), want["face_ids"])
    assert depth.cpu().numpy().tobytes() == want["depth"].tobytes()


def test_a_small_workspace_and_labels_without_vertex_labels_are_refused():
    import voxproj_host as vh
    L = vh.lib()
    s, _ = _twin("room:1,16,16")
    ws = vh.SplatWorkspace()
    (tv, tf, tl), n = _project(s, ws)
    need = int(L.vp_mesh_workspace_bytes(len(s[1]), 16, 16, n))
    assert need > int(L.vp_mesh_workspace_bytes(len(s[1]), 16, 16, 0)) > 0
    ws.ensure(need, DEV)
    ids = torch.empty((16, 16), dtype=torch.int32, device=DEV)
    lab = torch.empty((16, 16), dtype=torch.uint8, device=DEV)
    assert L.vp_mesh_rasterize(tl.data_ptr(), tf.data_ptr(), len(s[1]), 16, 16, n, ids.data_ptr(), None, None, None, ws.ptr(),
                               need - 1, None) == -2
    assert b"workspace has" in L.vp_last_error()
    assert L.vp_mesh_rasterize(None, tf.data_ptr(), len(s[1]), 16, 16, n, ids.data_ptr(), None, lab.data_ptr(), None, ws.ptr(),
                               need, None) == -1
    assert b"labels needs vertex_labels" in L.vp_last_error()
    vm = (ctypes.c_float * 16)(*np.eye(4).reshape(-1))
    assert L.vp_mesh_project(tv.data_ptr(), len(s[0]), tf.data_ptr(), len(s[1]), vm, 10.0, 10.0, 8.0, 8.0, 16, 16, 0.01, 100.0,
                             None, None, ws.ptr(), 255, None) == -2


def test_the_maps_align_with_the_splatter():
    """One small opaque Gaussian at a visible face's centroid: the splatter's alpha peaks on a pixel that the mesh map gives
    to that face (same camera, same pixel centres)."""
    import voxproj_host as vh
    s, want = _twin("room:1,96,64")
    v, f, l, vm, K, W, H = s
    vm64, fx, fy, cx, cy = mr.camera_f32(vm, K)
    cam = mr.camera_space(v, vm64)
    checked = 0
    for face in np.unique(want["face_ids"])[::7]:
        cen_w = v[f[face]].astype(np.float64).mean(axis=0)
        cen = cam[f[face]].mean(axis=0)
        j, i = int(np.floor(fx * cen[0] / cen[2] + cx)), int(np.floor(fy * cen[1] / cen[2] + cy))
        if not (2 <= j < W - 2 and 2 <= i < H - 2) or want["face_ids"][i, j] != face or (want["face_ids"] == face).sum() < 12:
            continue
        sc = float(cen[2] / fx)                              # one pixel
        r = vh.splat_features(torch.tensor(cen_w[None], dtype=torch.float32, device=DEV),
                              torch.tensor([[1.0, 0, 0, 0]], device=DEV), torch.full((1, 3), sc, device=DEV),
                              torch.tensor([0.95], device=DEV), torch.ones(1, 1, device=DEV), vm, K, W, H, want_alpha=True)
        alpha = r.alpha.cpu().numpy()
        pi, pj = np.unravel_index(alpha.argmax(), alpha.shape)
        assert alpha.max() > 0.3 and want["face_ids"][pi, pj] == face, (face, (i, j), (pi, pj))
        checked += 1
        if checked == 4:
            break
    assert checked == 4
