"""masks -> lift_instance_features.py -> render_gaussian_features.py on a synthetic scene, one JSON line
(metric instance_example_cosine).

  python tools/instance_example.py OUT_DIR [--steps 200] [--lr 0.01] [--dim 16] [--samples 32768 | --all_pixels]

The scene of tools/lift_example.py (8 000 Gaussians of synthetic_gaussians.make_gaussians in 13 classes, eight 192x128
cameras).  The "instance" of a Gaussian is its class; every view's mask is the rendered label image with the ids PERMUTED per
view (seeded), written as an 8-bit .png under OUT_DIR/object_mask -- ids that mean nothing across views, as a per-view
segmenter gives them; unreached pixels get 255.  Then, through the command lines' own main():
  lift_instance_features.py --masks_dir object_mask --out identity.pt        (twice: the tensors are compared)
  render_gaussian_features.py --gauss_feats identity.pt --out_dir identity   (reads the file as any LIFTED.pt)
The line carries the loss before and after, and how well the trained rows separate the instances: over the Gaussians, the
mean cosine between rows of the same class and between rows of different classes (Gaussians no view reaches keep their
start values and are counted with the rest).  Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd"), os.path.join(ROOT, "tools")]
import lift_instance_features as lif  # noqa: E402
import render_gaussian_features as rgf  # noqa: E402
import synthetic_gaussians as sg  # noqa: E402
import voxproj_host  # noqa: E402
from gaussian_ply import write_gaussian_ply  # noqa: E402


def main(argv=None):
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--samples", type=int, default=32768)
    ap.add_argument("--all_pixels", action="store_true")
    args = ap.parse_args(argv)
    out, P, W, H = args.out, 13, 192, 128
    mdir = os.path.join(out, "object_mask")
    os.makedirs(mdir, exist_ok=True)
    g = sg.make_gaussians(8000, n_classes=P, seed=3, scale_median=0.08)
    op, ls, q = sg.to_ply_fields(g)
    ply, cam = os.path.join(out, "point_cloud.ply"), os.path.join(out, "camera_params.json")
    write_gaussian_ply(ply, g["means"], op, ls, q)
    w2c, K0 = sg.make_views(8 * 12, g["room"], W, seed=3)
    w2c = w2c[::12]
    names = sorted(sg.write_camera_params(cam, w2c, K0, W, H))
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(g[k]).to(dev) for k in ("means", "quats", "scales", "opacities")}
    onehot = torch.nn.functional.one_hot(torch.from_numpy(g["classes"].astype(np.int64)), P).float().to(dev)
    rng = np.random.default_rng(0)
    for name, vm in zip(names, w2c):
        r = voxproj_host.splat_features(t["means"], t["quats"], t["scales"], t["opacities"], onehot, vm, K0, W, H, want_alpha=True)
        lab = r.labels.cpu().numpy()
        ids = rng.permutation(P)[np.clip(lab, 0, P - 1)].astype(np.uint8)
        ids[(lab < 0) | (r.alpha.cpu().numpy() < 0.5)] = 255
        Image.fromarray(ids, mode="L").save(os.path.join(mdir, name + ".png"))

    def lift(f):
        return lif.main(["--gaussians_ply", ply, "--cam_params", cam, "--masks_dir", mdir, "--dim", str(args.dim), "--steps",
                         str(args.steps), "--lr", str(args.lr), "--out", os.path.join(out, f)] +
                        (["--all_pixels"] if args.all_pixels else ["--samples", str(args.samples)]))

    res = lift("identity.pt")
    lift("identity_again.pt")
    a, b = torch.load(os.path.join(out, "identity.pt")), torch.load(os.path.join(out, "identity_again.pt"))
    same = all(a[k].numpy().tobytes() == b[k].numpy().tobytes() for k in ("xyz", "avg_feats", "weight"))
    rgf.main(["--gaussians_ply", ply, "--gauss_feats", os.path.join(out, "identity.pt"), "--cam_params", cam, "--out_dir",
              os.path.join(out, "identity")])
    rendered = sorted(f for f in os.listdir(os.path.join(out, "identity")) if f.endswith(".npy"))
    first = np.load(os.path.join(out, "identity", rendered[0]))
    rows = a["avg_feats"].double().numpy()
    rows = rows / np.maximum(np.linalg.norm(rows, axis=1, keepdims=True), 1e-12)
    cos = rows @ rows.T
    eq = g["classes"][:, None] == g["classes"][None, :]
    off = ~np.eye(len(rows), dtype=bool)
    line = dict(metric="instance_example_cosine", ids=P, dim=args.dim, W=W, H=H, views=len(names), gaussians=len(rows),
                steps=args.steps, lr=args.lr, samples=None if args.all_pixels else args.samples,
                loss_before=round(res["loss_before"], 6), loss_after=round(res["loss_after"], 6),
                cosine_same_instance=round(float(cos[eq & off].mean()), 4),
                cosine_other_instance=round(float(cos[~eq].mean()), 4),
                rendered_views=len(rendered), rendered_shape=list(first.shape), identity_files_byte_identical=same)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
