"""refine_gaussian_logits.py with the 3D neighbourhood regulariser, on the scene of tests/test_gpu_splat_loss.py's
test_cli_end_to_end (8000 Gaussians, P = 13, four views, 40 steps): with --reg3d_weight 2 the cross-entropy still falls and
the regulariser falls, a second run in a fresh process writes the same bytes, and --reg3d_weight 0 returns no reg3d_* keys.
The share of all 8000 Gaussians whose argmax is the true class is printed with and without the regulariser; it is not
asserted (measured on the MI355X: 0.3336 at the noisy start, 0.3423 after 40 steps without the regulariser, 0.6744 with
--reg3d_weight 2).

Fails without the --reg3d_* flags."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "3d-semantic-segmentation_amd")
for p in (HERE, ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu


def test_cli_with_the_regulariser(tmp_path):
    import refine_gaussian_logits as rgl
    import render_semantics_logits as rsl
    import synthetic_gaussians as sg
    from gaussian_ply import write_gaussian_ply
    P, W, H = 13, 96, 64
    g = sg.make_gaussians(8000, n_classes=P, seed=3, scale_median=0.08)
    true = sg.make_logits(g["classes"], P, seed=3)
    op, ls, q = sg.to_ply_fields(g)
    ply = str(tmp_path / "point_cloud.ply")
    write_gaussian_ply(ply, g["means"], op, ls, q)
    w2c, K0 = sg.make_views(4 * 6, g["room"], W, seed=3)
    w2c = w2c[::6]
    cam = str(tmp_path / "camera_params.json")
    names = sg.write_camera_params(cam, w2c, K0, W, H)
    prompts = np.array([f"c{i}" for i in range(P)])
    np.savez(tmp_path / "true.npz", logits=true, labels=true.argmax(1).astype(np.int16), prompts=prompts)
    rsl.main(["--gaussians_ply", ply, "--logit_path", str(tmp_path / "true.npz"), "--cam_params", cam, "--out_dir",
              str(tmp_path / "true"), "--channels", str(P)])
    tdir = tmp_path / "targets"
    tdir.mkdir()
    for idx, name in enumerate(sorted(names)):
        lab = torch.load(tmp_path / "true" / "labels" / f"{idx:05d}_labels.pt")["label_indices"].numpy().astype(np.int16)
        conf = np.load(tmp_path / "true" / "renders" / f"{idx:05d}_confidence.npy")
        lab[conf < 1e-3] = -1
        np.save(tdir / f"{name}_labels.npy", lab)
        np.save(tdir / f"{name}_confidence.npy", conf)
    noisy = (true + 2.5 * np.random.default_rng(0).normal(size=true.shape)).astype(np.float32)
    np.savez(tmp_path / "start.npz", logits=noisy, labels=noisy.argmax(1).astype(np.int16), prompts=prompts)
    common = ["--gaussians_ply", ply, "--logit_path", str(tmp_path / "start.npz"), "--cam_params", cam, "--targets_dir", str(tdir),
              "--steps", "40", "--views_per_step", "2"]
    reg = ["--reg3d_weight", "2"]
    res = rgl.main(common + reg + ["--out", str(tmp_path / "a.npz")])
    assert res["loss_after"] < res["loss_before"], res                 # the cross-entropy still falls
    assert res["reg3d_after"] < res["reg3d_before"], res
    # a second run in a fresh process, under its own time limit: the same bytes
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    p = subprocess.run([sys.executable, os.path.join(PKG, "refine_gaussian_logits.py")] + common + reg +
                       ["--out", str(tmp_path / "b.npz")], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "reg3d" in p.stdout
    a, b = np.load(tmp_path / "a.npz"), np.load(tmp_path / "b.npz")
    assert a["logits"].tobytes() == b["logits"].tobytes() and a["logits"].shape == (8000, P)
    # without the regulariser: no reg3d_* keys, and another result
    res0 = rgl.main(common + ["--reg3d_weight", "0", "--out", str(tmp_path / "c.npz")])
    assert not [k for k in res0 if k.startswith("reg3d")]
    c = np.load(tmp_path / "c.npz")
    assert c["logits"].tobytes() != a["logits"].tobytes()
    # a drawn sample per application runs too, and is as repeatable within the process
    rgl.main(common + reg + ["--reg3d_sample_size", "1000", "--steps", "4", "--out", str(tmp_path / "d.npz")])
    rgl.main(common + reg + ["--reg3d_sample_size", "1000", "--steps", "4", "--out", str(tmp_path / "e.npz")])
    assert np.load(tmp_path / "d.npz")["logits"].tobytes() == np.load(tmp_path / "e.npz")["logits"].tobytes()
    truth = true.argmax(1)
    share = {name: float((arr.argmax(1) == truth).mean()) for name, arr in (("start", noisy), ("weight 0", c["logits"]),
                                                                            ("weight 2", a["logits"]))}
    print(f"share of all 8000 Gaussians whose argmax is the true class: {share}", flush=True)
