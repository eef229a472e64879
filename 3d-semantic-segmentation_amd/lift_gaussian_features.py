"""Lift per-view 2D feature maps onto the Gaussians directly: every Gaussian gets the blend-weighted mean of the pixel
features it contributed to, over the views (vp_splat_project + vp_splat_lift; voxproj_host.GaussianFeatureLifter):

    F_g = sum_views sum_p m_p w_g(p) feat_v(p) / sum_views sum_p m_p w_g(p)

with w_g(p) = a T the weight the splatter blends Gaussian g into pixel p with and m_p an optional per-pixel weight.  It is
the direct route beside the voxel hop (aggregate_voxel_features_onthefly.py, then the 1-NN voxel of every Gaussian).

Inputs: the 3DGS point cloud (--gaussians_ply), camera_params.json (--cam_params; cameras and image sizes as
render_semantics_logits.py takes them: the 1600-pixel width rule or --downsample_factor, --principal_point) and per view
<features_dir>/<name>.npy, the LSeg map fp16 [C,h,w], brought to the render size with upsample_features(keep_dtype=True).
--weights_dir: optional <name>_confidence.npy f32 [H,W] at the render size (e.g. render_semantics_logits.py's), the m_p.
A pixel whose map holds a non-finite value is masked out (m_p = 0); their number is printed.

Output (--out LIFTED.pt): xyz f32 [N,3], avg_feats f16 [N,C] (rows of zeros where weight < --min_weight), weight f32 [N],
views (the image names).  ``query_voxel_features.py gaussians --gauss_feats LIFTED.pt`` queries the rows directly.  Two runs
with the same arguments write byte-identical tensors.  Runs on the GPU only; there is no CPU path.
"""
import argparse
import os

import numpy as np
import torch

import gaussian_views
import voxproj_host


def load_map(path):
    """The view's feature map as a CPU fp16 tensor [C,h,w]."""
    a = np.load(path)
    if a.ndim != 3:
        raise ValueError(f"{path}: a feature map must be [C, h, w], not {a.shape}")
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float16)


def load_weight(path, W, H):
    a = np.load(path)
    if a.shape != (H, W):
        raise ValueError(f"{path}: the pixel weights must be [{H}, {W}] (the render size), not {a.shape}")
    w = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
        raise ValueError(f"{path}: the pixel weights must be finite and >= 0")
    return w


def mask_nonfinite(feats, pixel_weight):
    """(pixel_weight with 0 at every pixel of the [H,W,C] map that holds a non-finite value, or the weights as given when
    there is none; the number of such pixels)."""
    bad = ~torch.isfinite(feats).all(dim=2)
    n_bad = int(bad.sum())
    if n_bad:
        base = pixel_weight if pixel_weight is not None else torch.ones(bad.shape, dtype=torch.float32, device=feats.device)
        pixel_weight = torch.where(bad, torch.zeros((), dtype=torch.float32, device=feats.device), base)
    return pixel_weight, n_bad


def save_lifted(path, xyz, avg_feats, weight, views):
    torch.save({"xyz": xyz.float().cpu().contiguous(), "avg_feats": avg_feats.to(torch.float16).cpu().contiguous(),
                "weight": weight.float().cpu().contiguous(), "views": list(views)}, path)


def load_lifted(path):
    """(xyz f32 [N,3], avg_feats f16 [N,C], weight f32 [N]) of a lift_gaussian_features.py result."""
    d = torch.load(path, map_location="cpu")
    for k in ("xyz", "avg_feats", "weight"):
        if k not in d:
            raise KeyError(f"{path}: needs 'xyz', 'avg_feats' and 'weight' (found {list(d)})")
    if d["avg_feats"].dim() != 2 or d["xyz"].shape != (d["avg_feats"].shape[0], 3) or d["weight"].shape != (d["avg_feats"].shape[0],):
        raise ValueError(f"{path}: xyz [N,3], avg_feats [N,C] and weight [N] must agree on N")
    return d["xyz"].float(), d["avg_feats"], d["weight"].float()


def build_parser():
    ap = argparse.ArgumentParser(description="Lift 2D feature maps onto the Gaussians (GPU, splat-weighted means)")
    gaussian_views.add_view_arguments(ap)
    ap.add_argument("--features_dir", required=True, help="per view <name>.npy: the LSeg map fp16 [C, h, w]")
    ap.add_argument("--weights_dir", default=None, help="optional per view <name>_confidence.npy f32 [H, W]: pixel weights")
    ap.add_argument("--min_weight", type=float, default=1e-3, help="Gaussians with less summed weight get a row of zeros")
    ap.add_argument("--out", required=True, help="output LIFTED.pt")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if not (args.min_weight >= 0 and np.isfinite(args.min_weight)):
        ap.error(f"--min_weight must be finite and >= 0, not {args.min_weight}")
    dev = gaussian_views.require_gpu("lift_gaussian_features")
    g = gaussian_views.load_gaussians(args.gaussians_ply, dev)
    names, view = gaussian_views.open_views(args)
    lifter = None
    for idx, name in enumerate(names):
        vm, K, W, H = view(name)
        src = load_map(os.path.join(args.features_dir, name + ".npy")).to(dev)
        feats = voxproj_host.upsample_features(src, H, W, keep_dtype=True)             # fp16 [H,W,C]
        if lifter is None:
            lifter = voxproj_host.GaussianFeatureLifter(g["means"].shape[0], feats.shape[2], dev)
        m = None
        if args.weights_dir:
            m = load_weight(os.path.join(args.weights_dir, name + "_confidence.npy"), W, H).to(dev)
        m, n_masked = mask_nonfinite(feats, m)
        n_isect, bad = lifter.add_view(g["means"], g["quats"], g["scales"], g["opacities"], feats, vm, K, W, H, m, check=False)
        n_bad = int(bad.item())
        if n_bad and idx == 0:
            print(f"[LIFT] warning: {n_bad} Gaussian(s) have a non-finite parameter and are not lifted")
        print(f"[LIFT] {idx:05d} {name}: {W}x{H}, {n_isect} tile intersections, {n_masked} pixel(s) masked as non-finite")
    if lifter is None:
        raise ValueError("no views to lift")
    avg, weight, valid = lifter.finish(args.min_weight)
    save_lifted(args.out, g["means"], avg, weight, names)
    print(f"\n[SUMMARY] {len(names)} view(s), {int(valid.sum())} of {len(valid)} Gaussians with weight >= {args.min_weight} -> {args.out}")


if __name__ == "__main__":
    main()
