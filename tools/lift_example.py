"""lift -> query -> render -> evaluate on the synthetic scene, one JSON line (metric lift_example_miou).

  python tools/lift_example.py OUT_DIR

Builds, under OUT_DIR: the scene of tools/eval_example.py (8 000 Gaussians of synthetic_gaussians.make_gaussians, 13 classes,
seed 3, eight 192x128 cameras), 13 unit "text embeddings" of 32 channels (text.npy, numpy default_rng(0)) and, as the 2D
feature maps an LSeg run would give, the views rendered from per-Gaussian features = the embedding of the Gaussian's class
(features/<name>.npy, fp16 [32,H,W]).  The ground truth is eval_example.py's: the views rendered from the true logits, pixels
of confidence below 1e-3 set to -1.  Then, through the command lines' own main():
  lift_gaussian_features.py --features_dir features --out lifted.pt          (twice: the two files' tensors are compared)
  query_voxel_features.py gaussians --gauss_feats lifted.pt --text_emb text.npy --logit_scale 10 --out lifted.npz
  render_semantics_logits.py --logit_path lifted.npz -> evaluate_label_maps.py --pred lifted --gt gt  (report_lifted.json)
Needs a GPU."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd")]
import evaluate_label_maps as elm  # noqa: E402
import lift_gaussian_features as lgf  # noqa: E402
import query_voxel_features as qvf  # noqa: E402
import render_semantics_logits as rsl  # noqa: E402
import synthetic_gaussians as sg  # noqa: E402
import voxproj_host  # noqa: E402
from gaussian_ply import write_gaussian_ply  # noqa: E402


def main(out):
    os.makedirs(out, exist_ok=True)
    P, C, W, H = 13, 32, 192, 128
    g = sg.make_gaussians(8000, n_classes=P, seed=3, scale_median=0.08)
    true = sg.make_logits(g["classes"], P, seed=3)
    op, ls, q = sg.to_ply_fields(g)
    ply = os.path.join(out, "point_cloud.ply")
    write_gaussian_ply(ply, g["means"], op, ls, q)
    w2c, K0 = sg.make_views(8 * 12, g["room"], W, seed=3)
    w2c = w2c[::12]
    cam = os.path.join(out, "camera_params.json")
    names = sorted(sg.write_camera_params(cam, w2c, K0, W, H))
    prompts = [f"c{i}" for i in range(P)]
    np.savez(os.path.join(out, "true.npz"), logits=true, labels=true.argmax(1).astype(np.int16), prompts=np.array(prompts))

    def render(npz, d):
        rsl.main(["--gaussians_ply", ply, "--logit_path", os.path.join(out, npz), "--cam_params", cam,
                  "--out_dir", os.path.join(out, d), "--channels", str(P), "--no_logits"])

    def lift(f):
        lgf.main(["--gaussians_ply", ply, "--cam_params", cam, "--features_dir", fdir, "--min_weight", "0.01",
                  "--out", os.path.join(out, f)])

    def evaluate(d, rep):
        return elm.main(["--pred", os.path.join(out, d), "--gt", gdir, "--num_classes", str(P),
                         "--prompts_npz", os.path.join(out, "true.npz"), "--out", os.path.join(out, rep)])

    render("true.npz", "true")
    gdir, fdir = os.path.join(out, "gt"), os.path.join(out, "features")
    os.makedirs(gdir, exist_ok=True)
    os.makedirs(fdir, exist_ok=True)
    for idx in range(len(names)):
        lab = torch.load(os.path.join(out, "true", "labels", f"{idx:05d}_labels.pt"))["label_indices"].numpy().astype(np.int16)
        lab[np.load(os.path.join(out, "true", "renders", f"{idx:05d}_confidence.npy")) < 1e-3] = -1
        np.save(os.path.join(gdir, f"{idx:05d}_labels.npy"), lab)
    # the 2D maps: every Gaussian carries the embedding of its class, rendered per view
    emb = np.random.default_rng(0).normal(size=(P, C))
    emb = (emb / np.linalg.norm(emb, axis=1, keepdims=True)).astype(np.float32)
    np.save(os.path.join(out, "text.npy"), emb)
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(g[k]).to(dev) for k in ("means", "quats", "scales", "opacities")}
    gfeat = torch.from_numpy(emb[g["classes"]]).to(dev)
    for name, vm in zip(names, w2c):
        r = voxproj_host.splat_features(t["means"], t["quats"], t["scales"], t["opacities"], gfeat, vm, K0, W, H,
                                        want_logits=True)
        np.save(os.path.join(fdir, name + ".npy"), r.logits.to(torch.float16).cpu().numpy())
    lift("lifted.pt")
    lift("lifted_again.pt")
    a, b = torch.load(os.path.join(out, "lifted.pt")), torch.load(os.path.join(out, "lifted_again.pt"))
    same = all(a[k].numpy().tobytes() == b[k].numpy().tobytes() for k in ("xyz", "avg_feats", "weight"))
    qvf.main(["gaussians", "--gauss_feats", os.path.join(out, "lifted.pt"), "--text_emb", os.path.join(out, "text.npy"),
              "--prompt", *prompts, "--logit_scale", "10", "--out", os.path.join(out, "lifted.npz")])
    render("lifted.npz", "lifted")
    r1, r2 = evaluate("lifted", "report_lifted.json"), evaluate("true", "report_true.json")
    lab = np.load(os.path.join(out, "lifted.npz"))["labels"]
    valid = lab >= 0
    line = dict(metric="lift_example_miou", P=P, C=C, W=W, H=H, views=len(names), gaussians=8000, min_weight=0.01,
                gaussians_without_feature=int((~valid).sum()),
                gaussian_label_accuracy=round(float((lab[valid] == g["classes"][valid]).mean()), 4),
                lifted=dict(r1["dataset"], lerf_miou=r1["lerf"]["miou"], lerf_mbiou=r1["lerf"]["mbiou"]),
                true=dict(r2["dataset"], lerf_miou=r2["lerf"]["miou"], lerf_mbiou=r2["lerf"]["mbiou"]),
                lifted_files_byte_identical=same)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
