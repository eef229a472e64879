"""fit_gaussian_appearance.py end to end on the GPU: 8000 Gaussians with random true colours, four 96 x 64 views whose
targets are rendered by the project's own rasterizer from the true colours and saved as 8-bit PNG; the fit starts from the
colours with noise added and runs 40 steps.  The loss falls, mean PSNR and SSIM rise, the written ply reads back, and a
second run in a fresh process writes the same bytes.  The PSNR values are printed, not asserted.

Fails without fit_gaussian_appearance.py."""
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


def test_cli_end_to_end(tmp_path):
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
    ply = str(tmp_path / "point_cloud.ply")
    gaussian_ply.write_gaussian_ply(ply, g["means"], op, ls, q, f_dc=fga.dc_from_colors(noisy))
    w2c, K0 = sg.make_views(4 * 6, g["room"], W, seed=3)
    cam = str(tmp_path / "camera_params.json")
    names = sg.write_camera_params(cam, w2c[::6], K0, W, H)
    # the targets: the true colours through the project's own rasterizer, with the geometry as the ply stores it
    back = gaussian_ply.read_gaussian_ply(ply, want_dc=True)
    assert set(back) == {"means", "quats", "scales", "opacities", "f_dc"} and back["f_dc"].shape == (N, 3)
    assert set(gaussian_ply.read_gaussian_ply(ply)) == {"means", "quats", "scales", "opacities"}     # the default is unchanged
    assert np.abs(fga.colors_from_dc(back["f_dc"]) - noisy).max() < 1e-6
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
    common = ["--gaussians_ply", ply, "--cam_params", cam, "--images_dir", str(idir), "--steps", "40", "--views_per_step", "2"]
    res = fga.main(common + ["--out", str(tmp_path / "a.ply"), "--report", str(tmp_path / "a.json")])
    print(f"PSNR {res['psnr_before']:.3f} -> {res['psnr_after']:.3f} dB, SSIM {res['ssim_before']:.5f} -> "
          f"{res['ssim_after']:.5f}, loss {res['loss_before']:.6f} -> {res['loss_after']:.6f}", flush=True)
    assert res["loss_after"] < res["loss_before"], res
    assert res["psnr_after"] > res["psnr_before"] and res["ssim_after"] > res["ssim_before"], res
    rep = json.load(open(tmp_path / "a.json"))
    assert len(rep["before"]) == len(rep["after"]) == 4 and rep["train"] == ["colors"]
    assert sorted(r["view"] for r in rep["after"]) == sorted(names)
    # the written ply reads back: new colours, everything else as it was
    a = gaussian_ply.read_gaussian_ply(str(tmp_path / "a.ply"), want_dc=True)
    for k in ("means", "quats", "scales", "opacities"):
        assert a[k].tobytes() == back[k].tobytes(), k
    assert a["f_dc"].shape == (N, 3) and np.isfinite(a["f_dc"]).all() and a["f_dc"].tobytes() != back["f_dc"].tobytes()
    err0 = np.abs(noisy - true).mean()
    seen = np.abs(fga.colors_from_dc(a["f_dc"]) - noisy).max(axis=1) > 1e-4          # the Gaussians some view sees
    err1 = np.abs(fga.colors_from_dc(a["f_dc"]) - true)[seen].mean()
    print(f"{int(seen.sum())} of {N} Gaussians moved; their mean colour error {err1:.4f} (start {err0:.4f})", flush=True)
    # a second run in a fresh process, under its own time limit: the same bytes
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    p = subprocess.run([sys.executable, os.path.join(PKG, "fit_gaussian_appearance.py")] + common + ["--out", str(tmp_path / "b.ply")],
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "[FIT] after 40 step(s)" in p.stdout
    assert open(tmp_path / "a.ply", "rb").read() == open(tmp_path / "b.ply", "rb").read()
    # geometry and opacities train through the same call
    res2 = fga.main(common[:-4] + ["--steps", "5", "--views_per_step", "2", "--train", "colors,opacities,scales,quats,means",
                                   "--out", str(tmp_path / "c.ply")])
    c = gaussian_ply.read_gaussian_ply(str(tmp_path / "c.ply"))
    assert all(np.isfinite(c[k]).all() for k in c) and c["means"].tobytes() != back["means"].tobytes()
    assert np.isfinite(res2["loss_after"])
