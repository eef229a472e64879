"""lift_gaussian_features.py end to end on the GPU: 300 Gaussians of synthetic_gaussians, two 64 x 48 views, 8-channel
maps at half the render size, one of them with a NaN pixel; once with --weights_dir and once without.  What main() saves
(avg_feats, weight, xyz, views) must equal, bit for bit, a voxproj_host.GaussianFeatureLifter driven by hand here over the
same views: the command line adds nothing to the lift but the reading of its inputs."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu
N, C, W, H = 300, 8, 64, 48
NAN_AT = (3, 11, 17)                                       # channel, row, column of the second view's map


def look_at(pos, forward):
    """World-to-camera [4,4] of a camera at ``pos`` looking along ``forward`` (x right, y down, z forward; world z is up)."""
    z = np.asarray(forward, np.float64) / np.linalg.norm(forward)
    x = np.cross(z, (0.0, 0.0, 1.0))
    x /= np.linalg.norm(x)
    c2w = np.eye(4)
    c2w[:3, :3] = np.stack([x, np.cross(z, x), z], axis=1)
    c2w[:3, 3] = pos
    return np.linalg.inv(c2w)


def test_main_saves_what_a_hand_driven_lifter_computes(tmp_path, capsys):
    import gaussian_ply
    import lift_gaussian_features as lgf
    import prepare_tensor_data as ptd
    import render_semantics_logits as rsl
    import synthetic_gaussians as sg
    import voxproj_host
    dev = torch.device("cuda:0")
    g = sg.make_gaussians(N, seed=7, scale_median=0.08)
    op, ls, q = sg.to_ply_fields(g)
    ply = str(tmp_path / "point_cloud.ply")
    gaussian_ply.write_gaussian_ply(ply, g["means"], op, ls, q)
    # two wide cameras (focal 0.6 W) at the ends of the 6 x 5 x 2.8 room, looking along it: the centres of about half the
    # Gaussians fall into each view, more than 100 of them with an opacity above 0.3
    K0 = np.array([[0.6 * W, 0, W / 2], [0, 0.6 * W, H / 2], [0, 0, 1.0]])
    w2c = [look_at((0.4, 2.2, 1.3), (1.0, 0.1, 0.0)), look_at((5.5, 2.8, 1.5), (-1.0, -0.15, -0.05))]
    cam = str(tmp_path / "camera_params.json")
    names = sorted(sg.write_camera_params(cam, w2c, K0, W, H))
    assert len(names) == 2
    fdir, wdir = tmp_path / "features", tmp_path / "weights"
    fdir.mkdir()
    wdir.mkdir()
    rng = np.random.default_rng(7)
    for v, name in enumerate(names):
        fmap = rng.normal(size=(C, H // 2, W // 2)).astype(np.float16)
        if v == 1:
            fmap[NAN_AT] = np.nan
        np.save(fdir / (name + ".npy"), fmap)
        np.save(wdir / (name + "_confidence.npy"), rng.uniform(0.0, 1.0, (H, W)).astype(np.float32))

    back = gaussian_ply.read_gaussian_ply(ply)
    t = {k: torch.from_numpy(back[k]).to(dev) for k in ("means", "quats", "scales", "opacities")}
    by_name, cams = ptd.load_camera_params(cam)

    def by_hand(weights):
        lifter = voxproj_host.GaussianFeatureLifter(N, C, dev)
        masked = []
        for name in names:
            vm, K = rsl.camera(by_name[name], cams, W, H, W, H)                 # 64 wide: the size rule leaves it alone
            src = torch.from_numpy(np.load(fdir / (name + ".npy"))).to(dev)
            feats = voxproj_host.upsample_features(src, H, W, keep_dtype=True)
            m = torch.from_numpy(np.load(wdir / (name + "_confidence.npy"))).to(dev) if weights else None
            bad = ~torch.isfinite(feats).all(dim=2)
            masked.append(int(bad.sum()))
            if masked[-1]:
                m = torch.where(bad, torch.zeros((), device=dev), m if m is not None else torch.ones((H, W), device=dev))
            lifter.add_view(t["means"], t["quats"], t["scales"], t["opacities"], feats, vm, K, W, H, m, check=False)
        return lifter.finish(1e-3) + (masked,)

    saved = {}
    for weights in (True, False):
        out = str(tmp_path / f"lifted_{int(weights)}.pt")
        lgf.main(["--gaussians_ply", ply, "--cam_params", cam, "--features_dir", str(fdir), "--out", out] +
                 (["--weights_dir", str(wdir)] if weights else []))
        text = capsys.readouterr().out
        avg, weight, valid, masked = by_hand(weights)
        assert masked[0] == 0 and masked[1] >= 1                                # the NaN reaches the render size
        assert f"[LIFT] 00000 {names[0]}: {W}x{H}" in text and f"{masked[1]} pixel(s) masked as non-finite" in text
        assert f"[SUMMARY] 2 view(s), {int(valid.sum())} of {N} Gaussians" in text
        d = torch.load(out)
        assert set(d) == {"xyz", "avg_feats", "weight", "views"} and d["views"] == names
        assert d["avg_feats"].dtype == torch.float16 and tuple(d["avg_feats"].shape) == (N, C)
        assert d["avg_feats"].numpy().tobytes() == avg.cpu().numpy().tobytes()
        assert d["weight"].numpy().tobytes() == weight.cpu().numpy().tobytes()
        assert d["xyz"].numpy().tobytes() == back["means"].tobytes()
        seen = int(valid.sum())
        print(f"weights {weights}: {seen} of {N} Gaussians lifted, {masked[1]} masked pixel(s)")
        assert seen >= 30 and bool(torch.isfinite(d["avg_feats"].float()).all()) and bool(d["avg_feats"][valid.cpu()].any())
        saved[weights] = d
    # the weights took part: the two runs are different lifts
    assert saved[True]["weight"].numpy().tobytes() != saved[False]["weight"].numpy().tobytes()
