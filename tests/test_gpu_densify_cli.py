"""fit_gaussian_appearance.py with adaptive density control, end to end on the GPU: the scene of
test_gpu_fit_appearance_cli.py thinned to every fourth Gaussian (2000 of 8000, four 96 x 64 views rendered from the full
cloud's true colours), all five parameters trained for 80 steps, a densification every 10 steps and one opacity reset.  The
report's counts add up, the ply has the final count and reads back finite, the loss falls, a second run in a fresh process
writes the same bytes, and --densify_interval 0 is the run without any of the options.  PSNR with and without densification
is printed, not asserted.

Fails without the --densify_* options of fit_gaussian_appearance.py."""
import json
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


def test_cli_with_densification(tmp_path):
    from PIL import Image

    import fit_gaussian_appearance as fga
    import gaussian_ply
    import prepare_tensor_data as ptd
    import render_semantics_logits as rsl
    import synthetic_gaussians as sg
    import voxproj_host
    dev = torch.device("cuda:0")
    N, W, H = 8000, 96, 64
    g = sg.make_gaussians(N, seed=3, scale_median=0.08)
    rng = np.random.default_rng(3)
    true = rng.uniform(0.05, 0.95, (N, 3)).astype(np.float32)
    noisy = np.clip(true + 0.25 * rng.normal(size=true.shape), 0.0, 1.0).astype(np.float32)
    op, ls, q = sg.to_ply_fields(g)
    w2c, K0 = sg.make_views(4 * 6, g["room"], W, seed=3)
    cam = str(tmp_path / "camera_params.json")
    names = sg.write_camera_params(cam, w2c[::6], K0, W, H)
    # the targets: the full cloud with its true colours; the fit starts from every fourth Gaussian with noisy colours
    full = str(tmp_path / "full.ply")
    gaussian_ply.write_gaussian_ply(full, g["means"], op, ls, q, f_dc=fga.dc_from_colors(true))
    back = gaussian_ply.read_gaussian_ply(full)
    t = {k: torch.from_numpy(back[k]).to(dev) for k in ("means", "quats", "scales", "opacities")}
    by_name, cams = ptd.load_camera_params(cam)
    idir = tmp_path / "images"
    idir.mkdir()
    for name in names:
        vm, K = rsl.camera(by_name[name], cams, W, H, W, H)
        r = voxproj_host.splat_features(t["means"], t["quats"], t["scales"], t["opacities"], torch.from_numpy(true).to(dev), vm, K,
                                        W, H, want_logits=True, want_alpha=False, want_confidence=False)
        img = (r.logits.clamp(0, 1) * 255.0 + 0.5).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
        Image.fromarray(np.ascontiguousarray(img)).save(idir / (os.path.splitext(name)[0] + ".png"))
    ply = str(tmp_path / "point_cloud.ply")
    gaussian_ply.write_gaussian_ply(ply, g["means"][::4], op[::4], ls[::4], q[::4], f_dc=fga.dc_from_colors(noisy[::4]))
    n0 = N // 4
    common =["--gaussians_ply", ply, "--cam_params", cam, "--images_dir", str(idir), "--steps", "80", "--views_per_step", "2",
              "--train", "colors,opacities,scales,quats,means"]
    # the trajectory's cameras stand close together (their own extent is 0.06), so the extent given is the room's length
    dens = ["--densify_interval", "10", "--densify_from", "5", "--densify_until", "75", "--opacity_reset_interval", "50",
            "--max_screen_size", "20", "--lr_opacities", "0.2", "--scene_extent", "6.0"]
    res = fga.main(common + dens + ["--out", str(tmp_path / "a.ply"), "--report", str(tmp_path / "a.json")])
    rep = json.load(open(tmp_path / "a.json"))
    # the counts add up
    assert res["n_before"] == n0 and [d["step"] for d in rep["densify"]] == [10, 20, 30, 40, 50, 60, 70]
    n = n0
    for d in rep["densify"]:
        assert d["n_before"] == n and d["n_after"] == d["kept"] + d["clones"] + 2 * d["split"], d
        assert d["pruned"] == d["n_before"] - d["kept"] - d["split"] >= 0, d
        n = d["n_after"]
    assert res["n_after"] == n and n != n0
    assert sum(d["clones"] for d in rep["densify"]) > 0 and sum(d["split"] for d in rep["densify"]) > 0
    a = gaussian_ply.read_gaussian_ply(str(tmp_path / "a.ply"), want_dc=True)
    assert a["means"].shape == (n, 3) and a["f_dc"].shape == (n, 3)
    assert all(np.isfinite(a[k]).all() for k in a)
    print(f"densified: {n0} -> {n} Gaussians, loss {res['loss_before']:.6f} -> {res['loss_after']:.6f}, PSNR "
          f"{res['psnr_before']:.3f} -> {res['psnr_after']:.3f} dB", flush=True)
    assert res["loss_after"] < res["loss_before"], res
    # a second run in a fresh process, under its own time limit: the same bytes
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    p = subprocess.run([sys.executable, os.path.join(PKG, "fit_gaussian_appearance.py")] + common + dens +
                       ["--out", str(tmp_path / "b.ply")], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "[FIT] densify at step 70" in p.stdout and f"{n0} -> {n} Gaussians" in p.stdout
    assert open(tmp_path / "a.ply", "rb").read() == open(tmp_path / "b.ply", "rb").read()
    # --densify_interval 0 is the run without any of the options
    off = fga.main(common + ["--lr_opacities", "0.2", "--densify_interval", "0", "--out", str(tmp_path / "c.ply"),
                             "--report", str(tmp_path / "c.json")])
    fga.main(common + ["--lr_opacities", "0.2", "--out", str(tmp_path / "d.ply")])
    assert open(tmp_path / "c.ply", "rb").read() == open(tmp_path / "d.ply", "rb").read()
    assert off["n_after"] == off["n_before"] == n0 and json.load(open(tmp_path / "c.json"))["densify"] == []
    print(f"PSNR after 80 steps: {off['psnr_after']:.3f} dB without densification ({n0} Gaussians), "
          f"{res['psnr_after']:.3f} dB with ({n} Gaussians)", flush=True)
