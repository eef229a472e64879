"""CPU-side checks of the mesh rasterizer (include/voxproj_mesh.h): the NumPy twin of tests/mesh_reference.py against a
brute-force float64 ray caster, its edge and clipping rules, the PLY reader, the third signature table against its header,
the entry points' host-side refusals and the CLI's dense mapping.  No device call is made here."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import mesh_reference as mr
import mesh_scenes as ms
from test_abi_cpu import _binding_error          # the comparison of a ctypes binding with a C prototype, written once

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 96, 64


# ---- the contract against the ray caster ----
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_twin_matches_the_ray_caster_on_closed_rooms(seed):
    """2028 faces, the camera 5 cm to 1.5 m from a wall: the wall beside the camera crosses the near plane and is seen at a
    grazing angle.  Watertight (no pixel uncovered); the face differs from the ray caster's only next to an edge, where the
    1/256-pixel snap decides between coplanar neighbours (<= 0.5 % of the pixels); the depth, taken from the unsnapped
    plane, agrees to 1e-6 relative everywhere (fp32 rounding alone is 6e-8)."""
    v, f, l = ms.room(seed)
    vm, K = ms.room_camera(seed), ms.intrinsics(W, H)
    r = mr.render(v, f, l, vm, K, W, H, want_cover=True)
    ids, depth = mr.ray_cast(v, f, vm, K, W, H)
    cam = mr.camera_space(v, mr.camera_f32(vm, K)[0])[f][:, :, 2]
    assert ((cam.min(axis=1) < 0.01) & (cam.max(axis=1) >= 0.01)).sum() > 50         # faces do cross the near plane
    uncovered, differ = int((r["face_ids"] < 0).sum()), int((r["face_ids"] != ids).sum())
    rel = float((np.abs(r["depth"].astype(np.float64) - depth) / depth).max())
    print(f"room {seed}: uncovered {uncovered}, face differs at {differ} of {W * H}, depth within {rel:.2e}")
    assert uncovered == 0 and (ids >= 0).all()
    assert r["cover"].max() == 1 and r["cover"].min() == 1          # every sample taken exactly once: no overlap, no crack
    assert differ <= 0.005 * W * H
    assert rel <= 1e-6
    assert np.array_equal(r["labels"], mr.face_labels(f, l)[r["face_ids"]])


# ---- shared edges and ties ----
def test_a_diagonal_through_sample_points_gives_every_sample_one_owner():
    vm, K = ms.exact_camera()
    a = mr.render(*ms.diagonal_quad(), vm, K, 12, 12, want_cover=True)
    b = mr.render(*ms.diagonal_quad(swap=True), vm, K, 12, 12, want_cover=True)
    inside = np.zeros((12, 12), bool)
    inside[2:10, 2:10] = True
    for r in (a, b):
        assert (r["cover"] == inside).all() and ((r["face_ids"] >= 0) == inside).all()
    # the diagonal's samples (j + 0.5, j + 0.5) lie exactly on the shared edge; one triangle owns them all, whichever index it has
    diag = a["face_ids"][np.arange(2, 10), np.arange(2, 10)]
    assert len(set(diag.tolist())) == 1
    assert np.array_equal(a["face_ids"][inside], 1 - b["face_ids"][inside])
    assert a["depth"].tobytes() == b["depth"].tobytes() and (a["depth"][inside] == 1.0).all()
    assert np.array_equal(a["labels"][inside], np.where(a["face_ids"][inside] == 0, 2, 1))    # (1,2,2) -> 2, (1,2,4) -> 1


def test_coincident_faces_the_lower_index_wins():
    vm, K = ms.exact_camera()
    v, f, l = ms.coincident_faces()
    r = mr.render(v, f, l, vm, K, 24, 24, want_cover=True)
    assert set(np.unique(r["face_ids"])) == {-1, 0} and r["cover"].max() == 2
    back = mr.render(v, f[::-1].copy(), l, vm, K, 24, 24)
    assert np.array_equal(back["face_ids"], r["face_ids"]) and back["depth"].tobytes() == r["depth"].tobytes()


# ---- clipping, culling, drops ----
def _one(verts, W_=16, H_=16, **kw):
    vm, K = np.eye(4, dtype=np.float32), ms.intrinsics(W_, H_, fx=8.0)
    v = np.asarray(verts, np.float32)
    return mr.render(v, np.arange(len(v), dtype=np.int32).reshape(-1, 3), np.arange(len(v)).astype(np.uint8), vm, K, W_, H_,
                     want_cover=True, **kw)


def front_at(z):
    return [[-z, -z, z], [z, -z, z], [0, z, z]]


def test_zero_area_and_back_facing_faces():
    front = [[-1, -1, 2], [1, -1, 2], [0, 1, 2]]
    a, b = _one(front), _one([front[0], front[2], front[1]])
    assert (a["face_ids"] >= 0).sum() > 20 and np.array_equal(a["face_ids"], b["face_ids"])      # both sides are drawn
    assert a["depth"].tobytes() == b["depth"].tobytes()
    line = _one([[-1, -1, 2], [0, 0, 2], [1, 1, 2]])                   # collinear: zero area
    point = _one([[0, 0, 2]] * 3)
    edge_on = _one([[0, -1, 2], [0, 1, 2], [0, 0, 4]])                 # seen edge-on: projects to a line
    for r in (line, point, edge_on):
        assert (r["face_ids"] == -1).all() and not r["counters"].any() and (r["depth"] == 0).all()


def test_faces_behind_and_across_the_near_plane():
    behind = _one([[-1, -1, -2], [1, -1, -2], [0, 1, -0.5]])
    assert (behind["face_ids"] == -1).all() and not behind["counters"].any()
    # a floor under the camera from z = -3 to z = 6: clipped at the near plane, drawn in the image's lower half only
    floor = [[-4, 1, -3], [4, 1, -3], [4, 1, 6], [-4, 1, -3], [4, 1, 6], [-4, 1, 6]]
    r = _one(floor)
    ids, depth = mr.ray_cast(np.asarray(floor, np.float32), np.arange(6).reshape(2, 3), np.eye(4), ms.intrinsics(16, 16, fx=8.0), 16, 16)
    assert ((r["face_ids"] >= 0) == (ids >= 0)).all() and (ids >= 0).sum() > 40 and (r["face_ids"][:8] == -1).all()
    hit = ids >= 0
    assert (np.abs(r["depth"][hit] - depth[hit]) <= 1e-6 * depth[hit]).all() and r["cover"].max() == 1
    # one vertex inside gives a triangle, two give a quad of two sub-triangles: both stay within the unclipped face's plane
    one_in = mr.clip_and_snap([(0.0, 0.0, 1.0), (1.0, 0.0, -1.0), (0.0, 1.0, -1.0)], 0.01, 8.0, 8.0, 8.0, 8.0)
    two_in = mr.clip_and_snap([(0.0, 0.0, 1.0), (1.0, 0.0, 1.0), (0.0, 1.0, -1.0)], 0.01, 8.0, 8.0, 8.0, 8.0)
    assert len(one_in) == 1 and len(two_in) == 2
    # far plane and depth range
    assert (_one(front_at(200.0))["face_ids"] == -1).all() and (_one(front_at(50.0), far=100.0)["face_ids"] >= 0).any()


def test_the_guard_band_drops_the_whole_face_and_counts_it():
    r = _one([[1e6, 0.0, 0.02], [0.0, 0.0, 2.0], [1.0, 1.0, 2.0]] + front_at(3.0))
    assert r["counters"].tolist() == [0, 0, 1] and set(np.unique(r["face_ids"])) <= {-1, 1}
    # 2^29 / 256 pixels is the band: just inside is kept (and clipped to the image), just outside is dropped
    x_edge = (2.0 ** 29 / 256 - 8.0) / 8.0 * 2.0                       # projects to X = 2^29 exactly at z = 2
    assert _one([[x_edge, -1.0, 2.0], [-1.0, -1.0, 2.0], [-1.0, 1.0, 2.0]])["counters"].tolist() == [0, 0, 0]
    assert _one([[x_edge * 1.01, -1.0, 2.0], [-1.0, -1.0, 2.0], [-1.0, 1.0, 2.0]])["counters"].tolist() == [0, 0, 1]
    bad = mr.render(np.array(front_at(3.0) + [[np.nan, 0, 1]], np.float32), np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4], [-1, 1, 2]], np.int32),
                    None, np.eye(4), ms.intrinsics(16, 16, fx=8.0), 16, 16)
    assert bad["counters"].tolist() == [2, 1, 0] and set(np.unique(bad["face_ids"])) == {-1, 0} and bad["labels"] is None


def test_majority_label_with_its_ties():
    faces = np.array([[0, 1, 2], [0, 0, 1], [3, 4, 4], [5, 6, 5], [7, 8, 9], [9, 8, 7]])
    labels = np.array([4, 4, 4, 9, 2, 7, 1, 200, 30, 100], np.uint8)
    got = mr.face_labels(faces, labels)
    want = [np.bincount(labels[t]).argmax() for t in faces]
    assert got.tolist() == want == [4, 4, 2, 7, 30, 30]


# ---- mesh_ply ----
@pytest.mark.parametrize("double", [False, True])
def test_mesh_ply_round_trip(tmp_path, double):
    import mesh_ply
    v, f, l = ms.room(1)
    raw = l.astype(np.int64) - 100
    path = str(tmp_path / "m.ply")
    mesh_ply.write_mesh_ply(path, v.astype(np.float64) if double else v, f, raw, double=double, index_type="uint" if double else "int",
                            vertex_extra=[("red", "uchar", np.arange(len(v)) % 256), ("quality", "double", np.linspace(0, 1, len(v)))],
                            face_extra=[("flags", "int", np.arange(len(f)))])
    m = mesh_ply.read_mesh_ply(path)
    assert m["verts"].dtype == np.float32 and m["verts"].tobytes() == v.tobytes()
    assert m["faces"].dtype == np.int32 and np.array_equal(m["faces"], f) and np.array_equal(m["labels"], raw)
    head = open(path, "rb").read().split(b"end_header\n")[0]
    assert (b"property double x" if double else b"property float x") in head and b"property list uchar" in head


def test_mesh_ply_without_labels_and_its_refusals(tmp_path):
    import mesh_ply
    v, f, _ = ms.whole_image_face()
    path = str(tmp_path / "plain.ply")
    mesh_ply.write_mesh_ply(path, v, f)
    assert mesh_ply.read_mesh_ply(path)["labels"] is None
    quad = str(tmp_path / "quad.ply")
    mesh_ply.write_mesh_ply(quad, np.zeros((4, 3), np.float32), [[0, 1, 2], [0, 2, 3], [1, 2, 3]], face_sizes=[3, 4, 3])
    with pytest.raises(ValueError, match=r"face 1 has 4 vertices"):
        mesh_ply.read_mesh_ply(quad)
    raw = open(path, "rb").read()
    for name, data, msg in (("ascii.ply", raw.replace(b"binary_little_endian", b"ascii"), "format ascii"),
                            ("short.ply", raw[:-5], "of 1 face records"), ("nolist.ply", raw.replace(b"list uchar int", b"list ushort int"), "face list must be"),
                            ("noply.ply", b"plx\n" + raw, "not a PLY file")):
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        with pytest.raises(ValueError, match=msg):
            mesh_ply.read_mesh_ply(p)


# ---- the third signature table against include/voxproj_mesh.h ----
def _mesh_prototypes():
    """{name: (return type, [parameter type, ...])} of every vp_* prototype of include/voxproj_mesh.h, ``const`` and
    parameter names dropped; a pointer type ends in `` *``."""
    txt = open(os.path.join(ROOT, "include", "voxproj_mesh.h")).read()
    txt = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))

    def ctype(decl, named):
        words = [w for w in decl.replace("*", " ").split() if w != "const"]
        return " ".join(words[:-1] if named else words) + (" *" if "*" in decl else "")

    return {name: (ctype(ret, False), [ctype(q, True) for q in params.split(",")])
            for ret, name, params in re.findall(r"([A-Za-z_][\w \t]*?[\s\*]+)(vp_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", txt)}


def test_mesh_header_matches_the_third_signature_table():
    import voxproj_host
    voxproj_host.build()
    protos = _mesh_prototypes()
    assert sorted(protos) == sorted(voxproj_host.EXPORTS_MESH) == ["vp_mesh_project", "vp_mesh_rasterize", "vp_mesh_workspace_bytes"]
    assert len(voxproj_host.EXPORTS) == 64 and len(voxproj_host.EXPORTS_EXT) == 2 and voxproj_host.VP_ABI_VERSION == 4
    assert not set(voxproj_host.EXPORTS_MESH) & (set(voxproj_host.EXPORTS) | set(voxproj_host.EXPORTS_EXT))
    L = voxproj_host.lib()
    for name, proto in protos.items():
        fn = getattr(L, name)
        assert _binding_error(proto, fn.restype, fn.argtypes) is None, (name, _binding_error(proto, fn.restype, fn.argtypes))
    proto, good = protos["vp_mesh_project"], list(L.vp_mesh_project.argtypes)
    assert len(good) == 18 and proto[1][1] == "int64_t" and good[4] is ctypes.POINTER(ctypes.c_float)
    assert "argument 1 is int64_t" in _binding_error(proto, ctypes.c_int, good[:1] + [ctypes.c_int] + good[2:])
    assert "takes 18 arguments, bound with 17" in _binding_error(proto, ctypes.c_int, good[:-1])


def test_entry_points_validate_on_the_host_before_any_launch():
    """Fake device addresses that are never dereferenced: every refusal is host arithmetic."""
    import voxproj_host
    L = voxproj_host.lib()
    P = 0x7000_0000_0000
    eye = (ctypes.c_float * 16)(*np.eye(4).reshape(-1))
    nan = (ctypes.c_float * 16)(*np.eye(4).reshape(-1))
    nan[6] = float("nan")
    base = dict(verts=P, nv=100, faces=P + 4096, nf=50, vm=eye, fx=80.0, fy=80.0, cx=48.0, cy=32.0, W=96, H=64, near=0.01, far=100.0,
                n=P + 8192, c=P + 12288, ws=P + 16384, wb=1 << 30)

    def project(**kw):
        a = dict(base, **kw)
        return L.vp_mesh_project(a["verts"], a["nv"], a["faces"], a["nf"], a["vm"], a["fx"], a["fy"], a["cx"], a["cy"], a["W"], a["H"],
                                 a["near"], a["far"], a["n"], a["c"], a["ws"], a["wb"], None)

    for kw, code, msg in ((dict(nf=-1), -1, b"n_faces = -1 outside [0, 2^31 - 1]"), (dict(nf=1 << 31), -1, b"n_faces"),
                          (dict(nv=-2), -1, b"n_verts"), (dict(W=0), -1, b"image 0 x 64"), (dict(H=32769), -1, b"outside [1, 32768]"),
                          (dict(faces=None), -1, b"null pointer"), (dict(verts=None), -1, b"null pointer"), (dict(vm=None), -1, b"null viewmat"),
                          (dict(vm=nan), -1, b"viewmat[6] is not finite"), (dict(fx=0.0), -1, b"fx, fy must be"), (dict(fy=-3.0), -1, b"fx, fy must be"),
                          (dict(near=0.0), -1, b"0 < near < far"), (dict(far=0.01), -1, b"0 < near < far"), (dict(far=float("inf")), -1, b"near < far"),
                          (dict(ws=None), -2, b"workspace is NULL"), (dict(ws=P + 16400), -2, b"256-byte aligned")):
        assert project(**kw) == code, kw
        assert msg in L.vp_last_error(), (kw, L.vp_last_error())

    rbase = dict(vl=P, faces=P + 4096, nf=50, W=96, H=64, cap=1000, ids=P + 8192, depth=P + 12288, labels=P + 16384, st=P + 20480,
                 ws=P + 24576, wb=1 << 30)

    def rasterize(**kw):
        a = dict(rbase, **kw)
        return L.vp_mesh_rasterize(a["vl"], a["faces"], a["nf"], a["W"], a["H"], a["cap"], a["ids"], a["depth"], a["labels"], a["st"],
                                   a["ws"], a["wb"], None)

    for kw, code, msg in ((dict(nf=-1), -1, b"n_faces"), (dict(cap=-1), -1, b"capacity = -1"), (dict(cap=1 << 31), -1, b"capacity"),
                          (dict(W=40000), -1, b"image 40000 x 64"), (dict(vl=None), -1, b"labels needs vertex_labels"),
                          (dict(faces=None), -1, b"labels needs vertex_labels and faces"), (dict(ws=None), -2, b"workspace is NULL"),
                          (dict(ws=P + 24577), -2, b"256-byte aligned")):
        assert rasterize(**kw) == code, kw
        assert msg in L.vp_last_error(), (kw, L.vp_last_error())
    assert L.vp_mesh_workspace_bytes(-1, 96, 64, 0) == 0 and L.vp_mesh_workspace_bytes(10, 0, 64, 0) == 0
    assert L.vp_mesh_workspace_bytes(10, 96, 64, 1 << 31) == 0


def test_host_wrappers_refuse_cpu_tensors_and_bad_shapes_before_any_device_call(monkeypatch):
    import torch

    import voxproj_host

    def no_call(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(voxproj_host, "_call", no_call)
    v, f, l = torch.zeros(5, 3), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(5, dtype=torch.uint8)
    K = torch.eye(3)
    with pytest.raises(ValueError, match="verts must be a CUDA tensor: there is no CPU path"):
        voxproj_host.mesh_render(v, f, l, torch.eye(4), K, 8, 8)
    with pytest.raises(ValueError, match="faces must be torch.int32"):
        voxproj_host.mesh_render(v, f.long(), l, torch.eye(4), K, 8, 8)
    with pytest.raises(ValueError, match="vertex_labels must be torch.uint8"):
        voxproj_host.mesh_render(v, f, l.int(), torch.eye(4), K, 8, 8)
    monkeypatch.setattr(voxproj_host, "_require_tensors", lambda *specs: None)
    for args, msg in (((torch.zeros(5, 2), f, l), r"verts must be \[V, 3\]"), ((v, torch.zeros(2, 4, dtype=torch.int32), l), r"faces must be \[F, 3\]"),
                      ((v, f, torch.zeros(4, dtype=torch.uint8)), r"vertex_labels must be \[5\]")):
        with pytest.raises(ValueError, match=msg):
            voxproj_host.mesh_render(*args, torch.eye(4), K, 8, 8)
    with pytest.raises(ValueError, match="viewmat must be"):
        voxproj_host.mesh_project(v, f, torch.zeros(3, 4), K, 8, 8)
    with pytest.raises(ValueError, match="need 0 < near < far"):
        voxproj_host.mesh_project(v, f, torch.eye(4), K, 8, 8, near=1.0, far=0.5)


# ---- the CLI ----
def test_cli_dense_mapping_and_options(tmp_path):
    import render_mesh_labels as rml
    raw = np.array([7, -100, 3, 3, 1200, 7, -100])
    m = rml.build_dense_map(raw)
    assert m == {3: 0, 7: 1, 1200: 2, -100: 255}
    dense, unknown = rml.apply_dense_map(raw, m)
    assert dense.dtype == np.uint8 and dense.tolist() == [1, 255, 0, 0, 2, 1, 255] and unknown == 0
    assert rml.build_dense_map(raw, ignore_label=3) == {-100: 0, 7: 1, 1200: 2, 3: 255}
    dense, unknown = rml.apply_dense_map(np.array([3, 8, -5, 5000]), m)          # labels another scene's map does not know
    assert dense.tolist() == [0, 255, 255, 255] and unknown == 3
    assert len(rml.build_dense_map(np.arange(255))) == 256
    with pytest.raises(ValueError, match="256 classes"):
        rml.build_dense_map(np.arange(256))
    path = str(tmp_path / "map.json")
    json.dump({str(k): v for k, v in m.items()}, open(path, "w"))
    assert rml.load_dense_map(path) == m
    json.dump({"1": 300}, open(path, "w"))
    with pytest.raises(ValueError, match="dense labels must lie"):
        rml.load_dense_map(path)
    ap = rml.build_parser()
    a = ap.parse_args(["--mesh_ply", "m", "--cam_params", "c", "--out_dir", "o"])
    assert (a.near, a.far, a.ignore_label, a.principal_point, a.downsample_factor, a.max_images, a.views, a.images_dir) == \
        (0.01, 100.0, -100, "center", None, None, None, "")
    assert not (a.save_depth or a.save_ids or a.index_names) and a.label_mapping == ""
    a = ap.parse_args(["--mesh_ply", "m", "--cam_params", "c", "--out_dir", "o", "--views", "a", "b", "--max_images", "1", "--save_depth",
                       "--save_ids", "--principal_point", "camera", "--downsample_factor", "0.5", "--ignore_label", "0", "--far", "50"])
    assert (a.views, a.max_images, a.save_depth, a.save_ids, a.principal_point, a.downsample_factor, a.ignore_label, a.far) == \
        (["a", "b"], 1, True, True, "camera", 0.5, 0, 50.0)
    for bad in (["--near", "0"], ["--near", "2", "--far", "1"]):
        with pytest.raises(SystemExit):
            rml.main(["--mesh_ply", "m", "--cam_params", "c", "--out_dir", "o"] + bad)
    with pytest.raises(SystemExit):
        ap.parse_args(["--cam_params", "c", "--out_dir", "o"])                  # --mesh_ply is required
