"""Render per-Gaussian logits into semantic views: the in-process counterpart of the reference's
voxel_to_gaussian/render_semantics_logits.py (stage 5.2), on the GPU through vp_splat_* (voxproj_host.splat_features).

Inputs: the 3DGS point cloud (--gaussians_ply, binary point_cloud.ply; gaussian_ply.read_gaussian_ply applies the model's
activations), the per-Gaussian logits (--logit_path: the .npz of ``query_voxel_features.py gaussians``, 'logits' [N, P] and
optional 'prompts') and the project's camera_params.json (--cam_params; world-to-camera = [R | tvec] of each image entry).

The reference's choices, kept here (INTEGRATION.md "Gaussian splatting"):
  - the logits are zero-padded or truncated to --channels (32, the reference's NUM_CHANNELS); the argmax runs over all of them;
  - the principal point is the image centre (W/2, H/2): the reference builds K from the field of view; --principal_point
    camera uses the camera's own cx, cy (scaled to the image);
  - the image size follows 3DGS's -r -1 rule: widths above 1600 scale down to 1600 (utils/camera_utils.py);
    --downsample_factor F renders int(W * F) x int(H * F) instead; the focal lengths scale with the image;
  - views in sorted image-name order (or --views), numbered 00000, 00001, ...;
  - gsplat's classic-mode defaults: near 0.01, far 1e10, eps2d 0.3, no background.

Per view, under --out_dir:
  labels/{idx:05d}_labels.pt        {'label_indices': uint8 [H,W]}
  renders/{idx:05d}_mask_color.png  palette PNG of the labels (query_voxel_features.palette over num_classes = logits.shape[1])
  renders/{idx:05d}_logits.npy      f32 [channels, H, W] (not with --no_logits)
  renders/{idx:05d}_confidence.npy  f32 [H,W] softmax top-1 minus top-2 over the channels; the .png too when matplotlib imports
Runs on the GPU only; there is no CPU path.
"""
import argparse
import os

import numpy as np
import torch

import gaussian_ply
import gaussian_views
import voxproj_host
from gaussian_views import camera, render_size  # noqa: F401  (tests and tools/*_example.py reach them here)
from query_voxel_features import palette

NUM_CHANNELS = 32


def pad_logits(logits, channels=NUM_CHANNELS):
    """float32 [N, channels]: zero-padded or truncated like the reference (np.pad / slice)."""
    lg = np.asarray(logits, dtype=np.float32)
    if lg.ndim != 2:
        raise ValueError(f"logits must be [N, P], not {lg.shape}")
    if lg.shape[1] < channels:
        lg = np.pad(lg, ((0, 0), (0, channels - lg.shape[1])), mode="constant")
    return np.ascontiguousarray(lg[:, :channels])


def save_palette_png(path, labels_u8, num_classes):
    from PIL import Image
    img = Image.fromarray(labels_u8)
    img.putpalette(palette(num_classes).reshape(-1).tolist())
    img.save(path)


def save_confidence_png(path, conf):
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return False
    plt.imsave(path, conf, cmap="viridis")
    return True


def load_inputs(args, dev):
    g = gaussian_ply.read_gaussian_ply(args.gaussians_ply)
    d = np.load(args.logit_path)
    if "logits" not in d:
        raise KeyError(f"{args.logit_path}: no 'logits' array")
    raw = d["logits"]
    if raw.shape[0] != g["means"].shape[0]:
        raise ValueError(f"{args.logit_path}: {raw.shape[0]} logit rows for {g['means'].shape[0]} Gaussians")
    prompts = [str(x) for x in d["prompts"]] if "prompts" in d else None
    t = {k: torch.from_numpy(v).to(dev) for k, v in g.items()}
    feats = torch.from_numpy(pad_logits(raw, args.channels)).to(dev)
    return t, feats, int(raw.shape[1]), prompts


def build_parser():
    ap = argparse.ArgumentParser(description="Render per-Gaussian logits into semantic views (GPU Gaussian splatting)")
    gaussian_views.add_view_arguments(ap)
    ap.add_argument("--logit_path", required=True, help=".npz with 'logits' [N, P] (query_voxel_features.py gaussians)")
    ap.add_argument("--out_dir", default="semantic_renders")
    ap.add_argument("--channels", type=int, default=NUM_CHANNELS, help="logit channels rendered (pad / truncate)")
    ap.add_argument("--no_logits", action="store_true", help="skip the _logits.npy files (labels and confidence only)")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if not 1 <= args.channels <= 64:
        ap.error(f"--channels must be in [1, 64], not {args.channels}")
    dev = gaussian_views.require_gpu("render_semantics_logits")
    g, feats, num_classes, prompts = load_inputs(args, dev)
    names, view = gaussian_views.open_views(args)               # an empty list is accepted: the summary is all it prints
    rdir, ldir = os.path.join(args.out_dir, "renders"), os.path.join(args.out_dir, "labels")
    os.makedirs(rdir, exist_ok=True)
    os.makedirs(ldir, exist_ok=True)
    ws = voxproj_host.SplatWorkspace()
    counts = np.zeros(args.channels, np.int64)
    for idx, name in enumerate(names):
        vm, K, W, H = view(name)
        r = voxproj_host.splat_features(g["means"], g["quats"], g["scales"], g["opacities"], feats, vm, K, W, H,
                                        want_logits=not args.no_logits, want_confidence=True, workspace=ws, check=False)
        n_bad = int(r.n_nonfinite.item())
        if n_bad and idx == 0:
            print(f"[RENDER] warning: {n_bad} Gaussian(s) have a non-finite parameter and are not drawn")
        lab = r.labels.to(torch.uint8).cpu()
        torch.save({"label_indices": lab}, os.path.join(ldir, f"{idx:05d}_labels.pt"))
        lab_np = lab.numpy()
        save_palette_png(os.path.join(rdir, f"{idx:05d}_mask_color.png"), lab_np, num_classes)
        if r.logits is not None:
            np.save(os.path.join(rdir, f"{idx:05d}_logits.npy"), r.logits.cpu().numpy())
        conf = r.confidence.cpu().numpy()
        np.save(os.path.join(rdir, f"{idx:05d}_confidence.npy"), conf)
        save_confidence_png(os.path.join(rdir, f"{idx:05d}_confidence.png"), conf)
        counts += np.bincount(lab_np.reshape(-1), minlength=args.channels)[:args.channels]
        print(f"[RENDER] {idx:05d} {name}: {W}x{H}, {r.n_isect} tile intersections")
    print(f"\n[SUMMARY] {len(names)} view(s) -> {args.out_dir}; pixel labels:")
    for i in np.nonzero(counts)[0]:
        nm = prompts[i] if prompts is not None and i < len(prompts) else f"Label {i}"
        print(f"  {nm:20s} (idx={i}): count={counts[i]}")


if __name__ == "__main__":
    main()
