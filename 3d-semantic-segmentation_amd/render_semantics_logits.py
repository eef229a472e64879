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
import voxproj_host
from query_voxel_features import palette

NUM_CHANNELS = 32
MAX_WIDTH = 1600


def pad_logits(logits, channels=NUM_CHANNELS):
    """float32 [N, channels]: zero-padded or truncated like the reference (np.pad / slice)."""
    lg = np.asarray(logits, dtype=np.float32)
    if lg.ndim != 2:
        raise ValueError(f"logits must be [N, P], not {lg.shape}")
    if lg.shape[1] < channels:
        lg = np.pad(lg, ((0, 0), (0, channels - lg.shape[1])), mode="constant")
    return np.ascontiguousarray(lg[:, :channels])


def render_size(W0, H0, downsample_factor=None):
    """(W, H): 3DGS's -r -1 rule (widths above 1600 down to 1600, int() of the scaled size), or int(W0 * f) x int(H0 * f)."""
    if downsample_factor is not None:
        return int(W0 * downsample_factor), int(H0 * downsample_factor)
    scale = W0 / MAX_WIDTH if W0 > MAX_WIDTH else 1.0
    return int(W0 / scale), int(H0 / scale)


def camera(entry, cams, W0, H0, W, H, principal_point="center"):
    """(viewmat f64 [4,4] = [R | tvec], K f64 [3,3]) at the render size: focal lengths scaled by W/W0 and H/H0 (the
    reference's focal = W / (2 tan(FoVx / 2)) with FoVx from the original focal and width); principal point at (W/2, H/2)
    or, with principal_point='camera', the camera's own scaled to the image."""
    params = cams[str(entry["camera_id"])]["params"]
    if len(params) == 4:
        fx, fy, cx, cy = (float(v) for v in params)
    else:
        fx, cx, cy = (float(v) for v in params)
        fy = fx
    sx, sy = W / W0, H / H0
    if principal_point == "camera":
        ppx, ppy = cx * sx, cy * sy
    else:
        ppx, ppy = W / 2.0, H / 2.0
    K = np.array([[fx * sx, 0.0, ppx], [0.0, fy * sy, ppy], [0.0, 0.0, 1.0]])
    vm = np.eye(4)
    vm[:3, :3] = np.asarray(entry["R"], np.float64)
    vm[:3, 3] = np.asarray(entry["tvec"], np.float64)
    return vm, K


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
    ap.add_argument("--gaussians_ply", required=True, help="3DGS point_cloud.ply (binary little-endian)")
    ap.add_argument("--logit_path", required=True, help=".npz with 'logits' [N, P] (query_voxel_features.py gaussians)")
    ap.add_argument("--cam_params", required=True, help="camera_params.json")
    ap.add_argument("--images_dir", default="", help="the images, for their size (else the camera's width / height)")
    ap.add_argument("--views", nargs="*", default=None, help="image names (default: all, sorted)")
    ap.add_argument("--max_images", type=int, default=None)
    ap.add_argument("--out_dir", default="semantic_renders")
    ap.add_argument("--channels", type=int, default=NUM_CHANNELS, help="logit channels rendered (pad / truncate)")
    ap.add_argument("--principal_point", choices=("center", "camera"), default="center")
    ap.add_argument("--downsample_factor", type=float, default=None, help="override the 1600-pixel width rule")
    ap.add_argument("--no_logits", action="store_true", help="skip the _logits.npy files (labels and confidence only)")
    return ap


def main(argv=None):
    import aggregate_voxel_features_onthefly as agg
    import prepare_tensor_data as ptd
    ap = build_parser()
    args = ap.parse_args(argv)
    if not 1 <= args.channels <= 64:
        ap.error(f"--channels must be in [1, 64], not {args.channels}")
    if not torch.cuda.is_available():
        raise RuntimeError("render_semantics_logits runs on the GPU: there is no CPU path")
    dev = torch.device("cuda", torch.cuda.current_device())
    g, feats, num_classes, prompts = load_inputs(args, dev)
    by_name, cams = ptd.load_camera_params(args.cam_params)
    names = args.views if args.views else sorted(by_name)
    if args.max_images is not None:
        names = names[:args.max_images]
    rdir, ldir = os.path.join(args.out_dir, "renders"), os.path.join(args.out_dir, "labels")
    os.makedirs(rdir, exist_ok=True)
    os.makedirs(ldir, exist_ok=True)
    ws = voxproj_host.SplatWorkspace()
    counts = np.zeros(args.channels, np.int64)
    for idx, name in enumerate(names):
        entry = by_name.get(name)
        if entry is None:
            raise KeyError(f"no camera entry for {name}")
        H0, W0 = agg._image_size(entry, cams, args.images_dir, name)
        W, H = render_size(W0, H0, args.downsample_factor)
        vm, K = camera(entry, cams, W0, H0, W, H, args.principal_point)
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
