"""Render the Gaussians' own wide feature rows into camera views (vp_splat_project + vp_splat_render;
voxproj_host.splat_render_view): per view the blend-weighted sum

    out[p, c] = sum_g w_g(p) F[g, c]

with w_g(p) = a T the weight the splatter blends Gaussian g into pixel p with.  It is the counterpart of
render_voxel_features.py (which copies the first-hit voxel's row) for rows that live on the Gaussians, and the forward of
lift_gaussian_features.py.

Inputs: the 3DGS point cloud (--gaussians_ply), the rows (--gauss_feats LIFTED.pt of lift_gaussian_features.py: avg_feats
f16 [N,C], one row per Gaussian of the point cloud, in its order) and camera_params.json (--cam_params; cameras and image
sizes as lift_gaussian_features.py takes them: the 1600-pixel width rule or --downsample_factor, --principal_point).

Output (--out_dir): per view <name>.npy, fp16 [C,H,W] -- the LSeg layout render_voxel_features.py writes -- and with
--save_alpha <name>_alpha.npy f32 [H,W] (1 - T: 0 where no Gaussian reaches the pixel, whose features are then zeros).
``query_voxel_features.py gaussian_views`` labels the same renders per pixel.  Two runs with the same arguments write
byte-identical files.  Runs on the GPU only; there is no CPU path.
"""
import argparse
import os

import numpy as np
import torch

import gaussian_ply  # noqa: F401  (tests reach the reader through this module)
import gaussian_views
import voxproj_host


def load_scene(args, dev):
    """(the Gaussians' tensors on ``dev``, their rows f16 [N,C] on ``dev``)."""
    import lift_gaussian_features
    g = gaussian_views.load_gaussians(args.gaussians_ply, dev)
    _, feats, _ = lift_gaussian_features.load_lifted(args.gauss_feats)
    n = int(g["means"].shape[0])
    if int(feats.shape[0]) != n:
        raise ValueError(f"{args.gauss_feats} has {int(feats.shape[0])} rows, {args.gaussians_ply} has {n} Gaussians")
    if not 1 <= int(feats.shape[1]) <= 4096:
        raise ValueError(f"{args.gauss_feats}: {int(feats.shape[1])} channels outside [1, 4096]")
    if feats.dtype not in (torch.float16, torch.float32):
        feats = feats.float()
    return g, feats.to(dev).contiguous()


def build_parser():
    ap = argparse.ArgumentParser(description="Render the Gaussians' wide feature rows into camera views (GPU)")
    gaussian_views.add_view_arguments(ap)
    ap.add_argument("--gauss_feats", required=True, help="LIFTED.pt of lift_gaussian_features.py: one feature row per Gaussian")
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--save_alpha", action="store_true", help="also write <name>_alpha.npy f32 [H,W]")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    dev = gaussian_views.require_gpu("render_gaussian_features")
    g, rows = load_scene(args, dev)
    os.makedirs(args.out_dir, exist_ok=True)
    ws = voxproj_host.SplatWorkspace()
    for idx, (name, vm, K, W, H) in enumerate(gaussian_views.iter_views(args)):
        out, alpha, n_isect, bad = voxproj_host.splat_render_view(g["means"], g["quats"], g["scales"], g["opacities"], rows, vm, K,
                                                                  W, H, dtype=torch.float16, want_alpha=args.save_alpha,
                                                                  workspace=ws, check=False)
        n_bad = int(bad.item())
        if n_bad and idx == 0:
            print(f"[RENDER] warning: {n_bad} Gaussian(s) have a non-finite parameter and are not rendered")
        stem = os.path.join(args.out_dir, name)
        np.save(stem + ".npy", out.permute(2, 0, 1).contiguous().cpu().numpy())
        if args.save_alpha:
            np.save(stem + "_alpha.npy", alpha.cpu().numpy())
        print(f"[RENDER] {idx:05d} {name}: {W}x{H}, {n_isect} tile intersections -> {stem}.npy f16 {[int(rows.shape[1]), H, W]}")


if __name__ == "__main__":
    main()
