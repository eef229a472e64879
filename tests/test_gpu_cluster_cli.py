"""cluster_features.py end to end on the GPU, on files written from the planted scene of tests/golden/cluster_golden.npz: both
sub-commands, the .npz schema of query_voxel_features.py, --init, --no_logits, --ply, the partition scikit-learn's KMeans
found on the unit rows (the stored one, up to a renaming of the ids), and render_semantics_logits.py drawing the file."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(HERE, "golden"), ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import label_sums_reference as ref  # noqa: E402
import make_cluster_golden as mk  # noqa: E402  (the scene of the fixture, rebuilt from the seed)
import query_reference as qr  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 64, 48
SCHEMA = {"labels", "logits", "prompts", "colors", "centroids", "counts", "objective", "n_iter"}


def look_at(pos, forward):
    """World-to-camera [4,4] of a camera at ``pos`` looking along ``forward`` (x right, y down, z forward; world z is up)."""
    z = np.asarray(forward, np.float64) / np.linalg.norm(forward)
    x = np.cross(z, (0.0, 0.0, 1.0))
    x /= np.linalg.norm(x)
    c2w = np.eye(4)
    c2w[:3, :3] = np.stack([x, np.cross(z, x), z], axis=1)
    c2w[:3, 3] = pos
    return np.linalg.inv(c2w)


def test_both_sub_commands_the_golden_partition_and_the_renderer(tmp_path, capsys):
    import cluster_features as cf
    import gaussian_ply
    import render_semantics_logits as rsl
    import synthetic_gaussians as sg
    golden = np.load(os.path.join(HERE, "golden", "cluster_golden.npz"))
    rows, truth, _ = mk.scene()
    assert mk.checksum(rows) == str(golden["rows_sha256"]), "the rebuilt scene is not the one the fixture was made from"
    N = len(rows)
    g = sg.make_gaussians(N, seed=7, scale_median=0.08)
    op, ls, q = sg.to_ply_fields(g)
    ply = str(tmp_path / "point_cloud.ply")
    gaussian_ply.write_gaussian_ply(ply, g["means"], op, ls, q)
    xyz = torch.from_numpy(np.asarray(g["means"], np.float32))

    # gaussians: the lifted rows as they are, the defaults (--k 10, --n_init 4, --seed 0)
    lifted = str(tmp_path / "LIFTED.pt")
    torch.save({"xyz": xyz, "avg_feats": torch.from_numpy(rows), "weight": torch.ones(N)}, lifted)
    out = str(tmp_path / "clusters.npz")
    cf.main(["gaussians", "--gauss_feats", lifted, "--out", out, "--ply", str(tmp_path / "clusters.ply")])
    text = capsys.readouterr().out
    d = np.load(out)
    assert set(d.files) == SCHEMA
    assert d["labels"].dtype == np.int16 and d["labels"].shape == (N,) and d["logits"].dtype == np.float32 and d["logits"].shape == (N, 10)
    assert d["prompts"].tolist() == [f"cluster_{k:02d}" for k in range(10)]
    assert d["colors"].dtype == np.uint8 and np.array_equal(d["colors"], qr.palette(10)[d["labels"]])
    assert d["centroids"].dtype == np.float32 and d["centroids"].shape == (10, 32)
    assert np.abs(np.linalg.norm(d["centroids"].astype(np.float64), axis=1) - 1).max() < 1e-6
    assert np.array_equal(d["counts"], np.bincount(d["labels"], minlength=10)) and int(d["n_iter"]) >= 1
    qr.check(rows, d["centroids"], 1.0, d["labels"].astype(np.int32), d["logits"])              # the cosines of one last query
    assert f"[CLUSTER] {N} rows, {N} clustered into K = 10" in text and "cluster_09" in text
    # the partition of the reference's tool on the unit rows, and the planted one
    assert ref.same_partition(d["labels"], golden["labels"]) and ref.adjusted_rand(d["labels"], truth) == 1.0
    head = open(tmp_path / "clusters.ply").read().split("end_header")[0].split("\n")
    assert head[:3] == ["ply", "format ascii 1.0", f"element vertex {N}"]

    # the renderer takes the file as it takes the query tool's
    cam = str(tmp_path / "camera_params.json")
    K0 = np.array([[0.6 * W, 0, W / 2], [0, 0.6 * W, H / 2], [0, 0, 1.0]])
    sg.write_camera_params(cam, [look_at((0.4, 2.2, 1.3), (1.0, 0.1, 0.0))], K0, W, H)
    rsl.main(["--gaussians_ply", ply, "--logit_path", out, "--cam_params", cam, "--out_dir", str(tmp_path / "views"), "--max_images", "1"])
    lab = torch.load(tmp_path / "views" / "labels" / "00000_labels.pt")["label_indices"].numpy()
    assert lab.shape == (H, W) and len(np.unique(lab)) >= 3 and lab.max() < 10
    assert "cluster_0" in capsys.readouterr().out

    # voxels: an aggregation file with two all-zero rows and a NaN row, from the centroids above, without logits
    feats = rows.copy()
    feats[[7, 4000]] = 0
    feats[123, 5] = np.nan
    vox = str(tmp_path / "ALL_nonzero_voxel_features_test.pt")
    torch.save({"xyz": xyz, "avg_feats": torch.from_numpy(feats), "voxel_coords": torch.zeros(N, 3, dtype=torch.int32)}, vox)
    np.save(tmp_path / "centroids.npy", d["centroids"])
    out2 = str(tmp_path / "vox_clusters.npz")
    cf.main(["voxels", "--vox", vox, "--out", out2, "--init", str(tmp_path / "centroids.npy"), "--no_logits"])
    text = capsys.readouterr().out
    e = np.load(out2)
    assert set(e.files) == SCHEMA - {"logits"}
    left = np.zeros(N, bool)
    left[[7, 123, 4000]] = True
    assert (e["labels"][left] == -1).all() and np.array_equal(e["labels"][~left], d["labels"][~left])
    assert not e["colors"][left].any() and int(e["counts"].sum()) == N - 3
    assert "2 all-zero and 1 non-finite row(s) left out" in text and "cluster_09" in text
    with pytest.raises(SystemExit):
        cf.main(["voxels", "--vox", vox, "--out", out2, "--k", "0"])
