"""Distil per-view 2D feature maps into per-Gaussian feature rows: optimise the rows so that the RENDERED feature image of
every view matches the view's map.  ``lift_gaussian_features.py`` gives every Gaussian the blend-weighted mean of the pixel
features it touched, which is a weighted average and not a fit; this is the fit, started from that lift.

  distill_gaussian_features.py --gaussians_ply point_cloud.ply --cam_params camera_params.json --features_dir DIR
      [--views NAME ...] [--max_images N] [--downsample_factor F] [--principal_point center|camera] [--images_dir DIR]
      [--weights_dir DIR] [--init LIFTED.pt] [--loss cosine|l2] [--min_alpha 0.5] [--steps 200] [--views_per_step 4]
      [--lr 0.01] [--seed 0] --out DISTILLED.pt

Inputs, cameras and sizes are lift_gaussian_features.py's: per view <features_dir>/<name>.npy, the LSeg map fp16 [C,h,w],
brought to the render size with upsample_features(keep_dtype=True); --weights_dir: optional <name>_confidence.npy f32 [H,W],
the pixel weights m_p.  A pixel whose map holds a non-finite value is masked out (m_p = 0); their number is printed.
--init: a LIFTED.pt to start from; without it the first pass is the lift of all views (voxproj_host.GaussianFeatureLifter).

Training: the rows are an fp32 parameter of torch Adam; each step draws --views_per_step views with a seeded generator and
takes the mean of their losses, each one fused call (splat_autograd.splat_feature_loss: vp_splat_render, vp_feature_loss,
vp_feature_loss_gradient, vp_splat_lift; no fp32 gradient image, no torch reduction over an image).  Pixels whose rendered
alpha is below --min_alpha take no part (see the scale hazard in include/voxproj.h).  The mean loss over all views is
printed before and after.  Every kernel on the path is deterministic, so two runs with the same arguments write
byte-identical tensors.

Output (--out): LIFTED.pt's schema -- xyz f32 [N,3], avg_feats f16 [N,C] (the trained rows), weight f32 [N] (the init's, or
the lift's), views -- which ``query_voxel_features.py gaussians --gauss_feats``, ``gaussian_views`` and
``render_gaussian_features.py`` read unchanged.  Runs on the GPU only; there is no CPU path.
"""
import argparse
import os

import torch

import gaussian_views
import lift_gaussian_features as lgf


def build_parser():
    ap = argparse.ArgumentParser(description="Distil 2D feature maps into per-Gaussian rows (fused GPU feature loss)")
    gaussian_views.add_view_arguments(ap)
    ap.add_argument("--features_dir", required=True, help="per view <name>.npy: the LSeg map fp16 [C, h, w]")
    ap.add_argument("--weights_dir", default=None, help="optional per view <name>_confidence.npy f32 [H, W]: pixel weights")
    ap.add_argument("--init", default=None, help="LIFTED.pt to start from (default: lift all views first)")
    ap.add_argument("--loss", choices=("cosine", "l2"), default="cosine")
    ap.add_argument("--min_alpha", type=float, default=0.5, help="pixels with a rendered alpha below this take no part")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--views_per_step", type=int, default=4)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True, help="output .pt (LIFTED.pt's schema)")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.steps < 0 or args.views_per_step < 1:
        ap.error("--steps must be >= 0 and --views_per_step >= 1")
    if not 0.0 <= args.min_alpha <= 1.0:
        ap.error(f"--min_alpha must lie in [0, 1], not {args.min_alpha}")
    import splat_autograd
    import voxproj_host
    dev = gaussian_views.require_gpu("distill_gaussian_features")
    g = gaussian_views.load_gaussians(args.gaussians_ply, dev)
    N = int(g["means"].shape[0])
    names, view = gaussian_views.open_views(args)
    if not names:
        raise ValueError("no views to train on")

    def load_view(name):
        """(viewmat, K, W, H, map f16 [H,W,C], pixel weights or None, masked pixels) of one view, as the lift reads it."""
        vm, K, W, H = view(name)
        src = lgf.load_map(os.path.join(args.features_dir, name + ".npy")).to(dev)
        feats = voxproj_host.upsample_features(src, H, W, keep_dtype=True)
        m = None
        if args.weights_dir:
            m = lgf.load_weight(os.path.join(args.weights_dir, name + "_confidence.npy"), W, H).to(dev)
        m, n_masked = lgf.mask_nonfinite(feats, m)
        return vm, K, W, H, feats, m, n_masked

    if args.init:
        _, rows0, weight = lgf.load_lifted(args.init)
        if rows0.shape[0] != N:
            raise ValueError(f"{args.init}: {rows0.shape[0]} rows for {N} Gaussians")
        rows0, weight = rows0.to(dev).float(), weight.to(dev)
    else:
        lifter = None
        for name in names:
            vm, K, W, H, feats, m, _ = load_view(name)
            if lifter is None:
                lifter = voxproj_host.GaussianFeatureLifter(N, feats.shape[2], dev)
            lifter.add_view(g["means"], g["quats"], g["scales"], g["opacities"], feats, vm, K, W, H, m, check=False)
        avg, weight, _ = lifter.finish()
        rows0 = avg.float()
    C = int(rows0.shape[1])
    param = torch.nn.Parameter(rows0.contiguous())
    opt = torch.optim.Adam([param], lr=args.lr)

    def view_loss(name):
        vm, K, W, H, feats, m, n_masked = load_view(name)
        if feats.shape[2] != C:
            raise ValueError(f"{name}: the map has {feats.shape[2]} channels, the rows have {C}")
        loss, _ = splat_autograd.splat_feature_loss(g["means"], g["quats"], g["scales"], g["opacities"], param, vm, K, W, H, feats,
                                                    m, kind=args.loss, reduction="mean", min_alpha=args.min_alpha, check=False)
        return loss, n_masked

    def evaluate():
        with torch.no_grad():
            total, masked = 0.0, 0
            for name in names:
                loss, n_masked = view_loss(name)
                total += float(loss)
                masked += n_masked
        return total / len(names), masked

    l0, masked = evaluate()
    print(f"[DISTILL] {len(names)} view(s), {N} Gaussians, {C} channels, {args.loss} loss, {masked} pixel(s) masked as non-finite")
    print(f"[DISTILL] before: mean loss {l0:.6f}")
    gen = torch.Generator().manual_seed(args.seed)
    k = min(args.views_per_step, len(names))
    for _ in range(args.steps):
        pick = gaussian_views.draw_indices(len(names), k, gen)
        opt.zero_grad(set_to_none=True)
        loss = 0
        for i in pick:
            loss = loss + view_loss(names[i])[0] / k
        loss.backward()
        opt.step()
    l1, _ = evaluate()
    print(f"[DISTILL] after {args.steps} step(s): mean loss {l1:.6f}")
    lgf.save_lifted(args.out, g["means"], param.detach(), weight, names)
    print(f"[DISTILL] -> {args.out}")
    return dict(loss_before=l0, loss_after=l1, masked=masked)


if __name__ == "__main__":
    main()
