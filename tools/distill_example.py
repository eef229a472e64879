"""lift -> distill -> query -> render -> evaluate on the synthetic scene, one JSON line (metric distill_example_miou).

  python tools/distill_example.py OUT_DIR [--steps 200] [--lr 0.01] [--loss cosine|l2] [--min_alpha 0.5]

Continues tools/lift_example.py, whose main() builds the scene under OUT_DIR first (8 000 Gaussians, 13 classes, eight
192x128 cameras, 32-channel maps, the ground truth, lifted.pt and its scores).  Then, through the command lines' own main():
  distill_gaussian_features.py --init lifted.pt --features_dir features --out distilled.pt   (twice: the tensors are compared)
  query_voxel_features.py gaussians --gauss_feats distilled.pt --text_emb text.npy --logit_scale 10 --out distilled.npz
  render_semantics_logits.py --logit_path distilled.npz -> evaluate_label_maps.py --pred distilled --gt gt
The line carries mIoU, fwIoU, accuracy and mBIoU of the distilled rows beside the lifted rows' and the true logits'.
Needs a GPU."""
import argparse
import contextlib
import io
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd"), os.path.join(ROOT, "tools")]
import distill_gaussian_features as dgf  # noqa: E402
import evaluate_label_maps as elm  # noqa: E402
import lift_example  # noqa: E402
import query_voxel_features as qvf  # noqa: E402
import render_semantics_logits as rsl  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--loss", choices=("cosine", "l2"), default="cosine")
    ap.add_argument("--min_alpha", type=float, default=0.5)
    args = ap.parse_args(argv)
    out, P = args.out, 13
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        lift_example.main(out)
    lifted_line = json.loads([ln for ln in buf.getvalue().splitlines() if ln.startswith("{")][-1])
    ply, cam = os.path.join(out, "point_cloud.ply"), os.path.join(out, "camera_params.json")
    prompts = [f"c{i}" for i in range(P)]

    def distill(f):
        return dgf.main(["--gaussians_ply", ply, "--cam_params", cam, "--features_dir", os.path.join(out, "features"),
                         "--init", os.path.join(out, "lifted.pt"), "--loss", args.loss, "--min_alpha", str(args.min_alpha),
                         "--steps", str(args.steps), "--lr", str(args.lr), "--out", os.path.join(out, f)])

    res = distill("distilled.pt")
    distill("distilled_again.pt")
    a, b = torch.load(os.path.join(out, "distilled.pt")), torch.load(os.path.join(out, "distilled_again.pt"))
    same = all(a[k].numpy().tobytes() == b[k].numpy().tobytes() for k in ("xyz", "avg_feats", "weight"))
    qvf.main(["gaussians", "--gauss_feats", os.path.join(out, "distilled.pt"), "--text_emb", os.path.join(out, "text.npy"),
              "--prompt", *prompts, "--logit_scale", "10", "--out", os.path.join(out, "distilled.npz")])
    rsl.main(["--gaussians_ply", ply, "--logit_path", os.path.join(out, "distilled.npz"), "--cam_params", cam,
              "--out_dir", os.path.join(out, "distilled"), "--channels", str(P), "--no_logits"])
    r = elm.main(["--pred", os.path.join(out, "distilled"), "--gt", os.path.join(out, "gt"), "--num_classes", str(P),
                  "--prompts_npz", os.path.join(out, "true.npz"), "--out", os.path.join(out, "report_distilled.json")])
    line = dict(metric="distill_example_miou", P=P, C=32, W=192, H=128, views=8, gaussians=8000, loss=args.loss,
                min_alpha=args.min_alpha, steps=args.steps, lr=args.lr, views_per_step=4,
                loss_before=round(res["loss_before"], 6), loss_after=round(res["loss_after"], 6),
                distilled=dict(r["dataset"], lerf_miou=r["lerf"]["miou"], lerf_mbiou=r["lerf"]["mbiou"]),
                lifted=lifted_line["lifted"], true=lifted_line["true"], distilled_files_byte_identical=same)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
