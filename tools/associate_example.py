"""masks -> lift_instance_features.py -> associate_instances.py on the scene of tools/instance_example.py, one JSON line
(metric associate_example).

  python tools/associate_example.py OUT_DIR [--lift_steps 200] [--steps 500] [--lr 5e-3] [--codes 64] [--dim 16]

8 000 Gaussians of synthetic_gaussians.make_gaussians in 13 classes, eight 192x128 cameras; every view's mask is the rendered
class image with the ids permuted per view (seeded), 255 where nothing is reached.  Through the command lines' own main():
  lift_instance_features.py --masks_dir object_mask --out identity.pt
  associate_instances.py --gauss_feats identity.pt --out codebook.pt --labels_dir labels      (twice: the files are compared)
The line carries the loss before and after; the share of mask pixels whose global id (the code written to <name>_labels.png)
belongs to a code that maps to the pixel's true class -- a code's class being the class most of its pixels have over ALL
views, so a code that means different classes in different views loses pixels; the same share for the Gaussians
(gaussian_ids against the Gaussians' classes); and whether the two runs wrote byte-identical files.  Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd"), os.path.join(ROOT, "tools")]
import associate_instances as ai  # noqa: E402
import lift_instance_features as lif  # noqa: E402
import synthetic_gaussians as sg  # noqa: E402
import voxproj_host  # noqa: E402
from gaussian_ply import write_gaussian_ply  # noqa: E402


def majority_share(codes, classes, n_codes, n_classes):
    """The share of samples whose code's majority class (over all samples) is their class."""
    table = np.zeros((n_codes, n_classes), np.int64)
    np.add.at(table, (codes, classes), 1)
    return float(table.max(1).sum()) / max(len(codes), 1)


def main(argv=None):
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lift_steps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--lr", type=float, default=5e-3)
    ap.add_argument("--codes", type=int, default=64)
    ap.add_argument("--dim", type=int, default=16)
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
    truth = {}
    for name, vm in zip(names, w2c):
        r = voxproj_host.splat_features(t["means"], t["quats"], t["scales"], t["opacities"], onehot, vm, K0, W, H, want_alpha=True)
        lab = r.labels.cpu().numpy()
        none = (lab < 0) | (r.alpha.cpu().numpy() < 0.5)
        ids = rng.permutation(P)[np.clip(lab, 0, P - 1)].astype(np.uint8)
        ids[none] = 255
        truth[name] = np.where(none, -1, lab)
        Image.fromarray(ids, mode="L").save(os.path.join(mdir, name + ".png"))
    ident = os.path.join(out, "identity.pt")
    lif.main(["--gaussians_ply", ply, "--cam_params", cam, "--masks_dir", mdir, "--dim", str(args.dim), "--steps",
              str(args.lift_steps), "--out", ident])

    def associate(tag):
        path, ldir = os.path.join(out, f"codebook{tag}.pt"), os.path.join(out, f"labels{tag}")
        res = ai.main(["--gaussians_ply", ply, "--cam_params", cam, "--masks_dir", mdir, "--gauss_feats", ident, "--codes",
                       str(args.codes), "--steps", str(args.steps), "--lr", str(args.lr), "--out", path, "--labels_dir", ldir])
        return res, path, ldir

    res, path, ldir = associate("")
    _, path2, ldir2 = associate("_again")
    same = open(path, "rb").read() == open(path2, "rb").read() and all(
        open(os.path.join(ldir, f), "rb").read() == open(os.path.join(ldir2, f), "rb").read() for f in sorted(os.listdir(ldir)))
    codes, classes = [], []
    for name in names:
        lab = np.array(Image.open(os.path.join(ldir, name + "_labels.png"))).astype(np.int64)
        keep = (truth[name] >= 0) & (lab != 255)
        codes.append(lab[keep])
        classes.append(truth[name][keep])
    d = torch.load(path)
    line = dict(metric="associate_example", classes=P, codes=args.codes, dim=args.dim, W=W, H=H, views=len(names),
                gaussians=int(d["gaussian_ids"].numel()), lift_steps=args.lift_steps, steps=args.steps, lr=args.lr,
                loss_before=round(res["loss_before"], 6), loss_after=round(res["loss_after"], 6),
                pixel_share_consistent=round(majority_share(np.concatenate(codes), np.concatenate(classes), args.codes, P), 4),
                gaussian_share_consistent=round(majority_share(d["gaussian_ids"].numpy().astype(np.int64), g["classes"],
                                                               args.codes, P), 4),
                codes_in_use=int(len(np.unique(np.concatenate(codes)))), files_byte_identical=bool(same))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
