"""render -> evaluate on the synthetic scene, before and after a refinement, one JSON line (metric example_miou).

  python tools/eval_example.py OUT_DIR

Builds, under OUT_DIR: 8 000 Gaussians of synthetic_gaussians.make_gaussians (13 classes, seed 3, scale_median 0.08) as a
.ply, eight 192x128 cameras (every 12th frame of the 96-frame trajectory, seed 3), true.npz (make_logits, seed 3) and
start.npz (the true logits plus N(0, 2.5^2) noise, numpy default_rng(0)).  The ground truth (gt/<idx>_labels.npy, and the same
maps with their confidence as targets/ for the refinement) is render_semantics_logits.py of true.npz with the pixels of
confidence below 1e-3 set to -1.  Then, through the command lines' own main():
  render_semantics_logits.py --logit_path start.npz   -> evaluate_label_maps.py --pred start   --gt gt  (report_start.json)
  refine_gaussian_logits.py --steps 100 --views_per_step 2 --report_miou --logit_path start.npz --out refined.npz
  render_semantics_logits.py --logit_path refined.npz -> evaluate_label_maps.py --pred refined --gt gt  (report_refined.json)
  evaluate_label_maps.py --pred true --gt gt                                                        (report_true.json)
and the refined maps are evaluated a second time to compare the two reports byte for byte.  Needs a GPU."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd")]
import evaluate_label_maps as elm  # noqa: E402
import refine_gaussian_logits as rgl  # noqa: E402
import render_semantics_logits as rsl  # noqa: E402
import synthetic_gaussians as sg  # noqa: E402
from gaussian_ply import write_gaussian_ply  # noqa: E402


def main(out):
    os.makedirs(out, exist_ok=True)
    P, W, H = 13, 192, 128
    g = sg.make_gaussians(8000, n_classes=P, seed=3, scale_median=0.08)
    true = sg.make_logits(g["classes"], P, seed=3)
    op, ls, q = sg.to_ply_fields(g)
    ply = os.path.join(out, "point_cloud.ply")
    write_gaussian_ply(ply, g["means"], op, ls, q)
    w2c, K0 = sg.make_views(8 * 12, g["room"], W, seed=3)
    w2c = w2c[::12]
    cam = os.path.join(out, "camera_params.json")
    names = sg.write_camera_params(cam, w2c, K0, W, H)
    prompts = np.array([f"c{i}" for i in range(P)])
    np.savez(os.path.join(out, "true.npz"), logits=true, labels=true.argmax(1).astype(np.int16), prompts=prompts)
    render = lambda npz, d: rsl.main(["--gaussians_ply", ply, "--logit_path", os.path.join(out, npz), "--cam_params", cam, "--out_dir", os.path.join(out, d), "--channels", str(P), "--no_logits"])
    render("true.npz", "true")
    tdir, gdir = os.path.join(out, "targets"), os.path.join(out, "gt")
    os.makedirs(tdir, exist_ok=True); os.makedirs(gdir, exist_ok=True)
    for idx, name in enumerate(sorted(names)):
        lab = torch.load(os.path.join(out, "true", "labels", f"{idx:05d}_labels.pt"))["label_indices"].numpy().astype(np.int16)
        conf = np.load(os.path.join(out, "true", "renders", f"{idx:05d}_confidence.npy"))
        lab[conf < 1e-3] = -1
        np.save(os.path.join(tdir, f"{name}_labels.npy"), lab); np.save(os.path.join(tdir, f"{name}_confidence.npy"), conf)
        np.save(os.path.join(gdir, f"{idx:05d}_labels.npy"), lab)           # the same maps under the renderer's stems
    noisy = (true + 2.5 * np.random.default_rng(0).normal(size=true.shape)).astype(np.float32)
    np.savez(os.path.join(out, "start.npz"), logits=noisy, labels=noisy.argmax(1).astype(np.int16), prompts=prompts)
    ev = lambda d, rep: elm.main(["--pred", os.path.join(out, d), "--gt", gdir, "--num_classes", str(P), "--prompts_npz", os.path.join(out, "true.npz"), "--out", os.path.join(out, rep)])
    render("start.npz", "start")
    r0 = ev("start", "report_start.json")
    res = rgl.main(["--gaussians_ply", ply, "--logit_path", os.path.join(out, "start.npz"), "--cam_params", cam, "--targets_dir", tdir, "--steps", "100", "--views_per_step", "2", "--report_miou", "--out", os.path.join(out, "refined.npz")])
    render("refined.npz", "refined")
    r1 = ev("refined", "report_refined.json")
    r2 = ev("true", "report_true.json")
    ev("refined", "report_refined_again.json")
    same = open(os.path.join(out, "report_refined.json"), "rb").read() == open(os.path.join(out, "report_refined_again.json"), "rb").read()
    line = dict(metric="example_miou", P=P, W=W, H=H, views=len(names), gaussians=8000, steps=100,
                start=dict(r0["dataset"], lerf_miou=r0["lerf"]["miou"], lerf_mbiou=r0["lerf"]["mbiou"]),
                refined=dict(r1["dataset"], lerf_miou=r1["lerf"]["miou"], lerf_mbiou=r1["lerf"]["mbiou"]),
                true=dict(r2["dataset"], lerf_miou=r2["lerf"]["miou"], lerf_mbiou=r2["lerf"]["mbiou"]),
                refine_cli={k: round(float(v), 6) for k, v in res.items()}, reports_byte_identical=same)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
