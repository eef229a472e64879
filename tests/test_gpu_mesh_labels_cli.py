"""render_mesh_labels.py end to end on the GPU: a labelled room and three cameras on disk, the CLI's maps against the NumPy
twin through the dense mapping, and evaluate_label_maps.py reading them as ground truth."""
import json
import os

import numpy as np
import pytest

import mesh_reference as mr
import mesh_scenes as ms

pytestmark = pytest.mark.gpu
W, H = 96, 64
WALL = 2                                             # the wall relabelled in the second scene
IGNORE = -100


def _scene():
    """(verts, faces, raw labels int64 with some -100, cameras [(name, viewmat f32)], K)."""
    v, f, l = ms.room(0)
    raw = l.astype(np.int64) * 3 + 5
    raw[np.random.default_rng(3).random(len(raw)) < 0.08] = IGNORE
    cams = [(f"frame_{k:03d}.jpg", ms.room_camera(k)) for k in range(3)]
    return v, f, raw, cams, ms.intrinsics(W, H, fx=77.5, fy=80.25, cx=46.5, cy=33.0)


def _write(tmp, raw):
    import mesh_ply
    v, f, _, cams, K = _scene()
    os.makedirs(tmp, exist_ok=True)
    mesh_ply.write_mesh_ply(os.path.join(tmp, "mesh.ply"), v, f, raw, vertex_extra=[("red", "uchar", np.arange(len(v)) % 251)])
    images = {str(i): dict(name=name, camera_id=1, R=vm[:3, :3].astype(np.float64).tolist(), tvec=vm[:3, 3].astype(np.float64).tolist())
              for i, (name, vm) in enumerate(cams)}
    cameras = {"1": dict(params=[K[0, 0], K[1, 1], K[0, 2], K[1, 2]], width=W, height=H)}
    with open(os.path.join(tmp, "camera_params.json"), "w") as fh:
        json.dump(dict(images=images, cameras=cameras), fh)
    return os.path.join(tmp, "mesh.ply"), os.path.join(tmp, "camera_params.json")


def _run(mesh, cam, out, *more):
    import render_mesh_labels
    render_mesh_labels.main(["--mesh_ply", mesh, "--cam_params", cam, "--out_dir", out, "--downsample_factor", "1.0",
                             "--principal_point", "camera", *more])


def _png(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == "L"
        return np.array(im)


def test_cli_maps_equal_the_twin_and_score_as_ground_truth(tmp_path, capsys):
    import evaluate_label_maps
    import render_mesh_labels
    v, f, raw, cams, K = _scene()
    mesh, cam = _write(str(tmp_path / "a"), raw)
    out = str(tmp_path / "gt")
    _run(mesh, cam, out, "--save_depth", "--save_ids")
    mapping = json.load(open(os.path.join(out, "label_mapping.json")))
    uniq = sorted(set(raw.tolist()) - {IGNORE})
    assert mapping == {**{str(r): i for i, r in enumerate(uniq)}, str(IGNORE): 255}
    dense, unknown = render_mesh_labels.apply_dense_map(raw, {int(k): v for k, v in mapping.items()})
    assert unknown == 0 and (dense[raw == IGNORE] == 255).all() and dense[raw != IGNORE].max() == len(uniq) - 1
    twins = []
    for name, vm in cams:
        want = mr.render(v, f, dense, vm, K, W, H)
        twins.append(want)
        stem = os.path.splitext(name)[0]
        assert np.array_equal(_png(os.path.join(out, stem + ".png")), want["labels"])
        assert np.array_equal(np.load(os.path.join(out, stem + "_face_ids.npy")), want["face_ids"])
        assert np.load(os.path.join(out, stem + "_depth.npy")).tobytes() == want["depth"].tobytes()
    assert capsys.readouterr().out.count("uncovered 0.000 %") == 3
    P = len(uniq)
    rep = evaluate_label_maps.main(["--pred", out, "--gt", out, "--num_classes", str(P), "--out", str(tmp_path / "self.json")])
    assert rep["dataset"]["miou"] == 1.0 and rep["views"] == 3

    # one wall relabelled to a class of its own kind: the confusion moves exactly that wall's pixels
    n = ms.ROOM_GRID ** 2
    raw2 = raw.copy()
    target = uniq[1]
    raw2[WALL * n:(WALL + 1) * n] = target
    mesh2, _ = _write(str(tmp_path / "b"), raw2)
    out2 = str(tmp_path / "relabelled")
    _run(mesh2, cam, out2, "--label_mapping", os.path.join(out, "label_mapping.json"))
    assert json.load(open(os.path.join(out2, "label_mapping.json"))) == mapping
    faces_per_wall = len(f) // 6
    moved = 0
    for k, want in enumerate(twins):
        on_wall = (want["face_ids"] >= WALL * faces_per_wall) & (want["face_ids"] < (WALL + 1) * faces_per_wall)
        moved += int((on_wall & (want["labels"] != 255) & (want["labels"] != 1)).sum())
        assert (want["labels"][~on_wall] == _png(os.path.join(out2, "frame_%03d.png" % k))[~on_wall]).all()
    assert moved > 500
    rep = evaluate_label_maps.main(["--pred", out2, "--gt", out, "--num_classes", str(P), "--out", str(tmp_path / "moved.json")])
    conf = np.array(rep["confusion"])
    off = conf - np.diag(np.diag(conf))
    assert off.sum() == moved and moved in (off[:, 1].sum(), off[1, :].sum())                  # everything moved to class 1
