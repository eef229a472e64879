"""Query the per-voxel feature table with text embeddings: which voxel is a *chair*?

Counterpart of the ``query`` sub-commands of the reference's voxel_to_gaussian/voxeltovoxel_logits.py and
voxeltoGaussian_logits.py (stage 5.1), plus a novel-view segmentation straight from the voxel grid.  Every row of the
table the aggregator writes (ALL_nonzero_voxel_features_*.pt: xyz f32 [n,3], avg_feats f16 [n,C], voxel_coords i32 [n,3]) is
scored against P prompt embeddings with a normalised dot product on the GPU (vp_query_features):

    logit_j = scale * cos(avg_feats, text_j),  label = argmax_j logit_j,  confidence = softmax top-1 minus top-2

Sub-commands (all take --text_emb FILE --prompt NAME ... [--logit_scale S]; one prompt per embedding row):
  voxels     --vox ALL_*.pt --out X.npz: labels int16 [n], logits f32 [n,P], prompts, colors uint8 [n,3] and
             X_colored_voxels.ply (ASCII, the voxel centres coloured by label).
  gaussians  --vox ALL_*.pt --gauss centres.npy [--map g2v.npy] --out X.npz: per Gaussian labels int16 [M], logits f32 [M,P],
             prompts and X_colored_gaussians.ply; the Gaussian -> voxel map is read from --map or computed with
             voxel_to_gaussian_map.map_gaussians_to_voxels (the 1-NN voxel).
             --gauss_feats LIFTED.pt (lift_gaussian_features.py: xyz, avg_feats f16 [M,C], weight) instead of --vox / --gauss /
             --map: the Gaussians' own rows are queried directly; a Gaussian with weight 0 or a row of zeros (below the
             lift's --min_weight, or a mean that rounds to zeros in fp16) gets label -1 and zero logits.  The .npz has the
             same schema either way.
  views      the camera / grid / view arguments of render_voxel_features.py: per view <name>_labels.npy int16 [H,W] (-1 where
             the ray hits nothing or hits an occupied voxel without a feature row), <name>_confidence.npy f32 [H,W] (0 where the
             label is -1) and with --save_logits <name>_logits.npy f16 [P,H,W] (the layout logit_confidence_map.py reads; zeros
             where the label is -1).

The text embeddings are an input (.npy or .pt, [P, C] float): this project does not run the CLIP / LSeg text encoder.
--logit_scale defaults to 1.0 (plain cosine similarity); LSeg's head multiplies by its own logit_scale.  The labels do not
depend on it, the logits and the confidence do.  Runs on the GPU only; there is no CPU path.
"""
import argparse
import os

import numpy as np
import torch

import voxproj_host


def palette(n):
    """uint8 [n,3] colours of labels 0..n-1: bit 3b + c of the label sets bit 7 - b of channel c (1 -> (128,0,0),
    2 -> (0,128,0), 4 -> (0,0,128), 8 -> (64,0,0), ...)."""
    lab = np.arange(n, dtype=np.int64)
    out = np.zeros((n, 3), np.int64)
    for b in range(8):
        for c in range(3):
            out[:, c] |= ((lab >> (3 * b + c)) & 1) << (7 - b)
    return out.astype(np.uint8)


def label_colors(labels, n_labels):
    """uint8 [N,3]: the palette colour of each label, black for label -1."""
    pal = np.concatenate([palette(n_labels), np.zeros((1, 3), np.uint8)])
    lab = np.asarray(labels, dtype=np.int64)
    return pal[np.where(lab < 0, n_labels, lab)]


def load_text(path):
    """float32 [P, C] text embeddings from a .npy array or a .pt tensor."""
    t = torch.from_numpy(np.load(path)) if path.endswith(".npy") else torch.load(path, map_location="cpu")
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{path}: expected one [P, C] tensor, found {type(t).__name__}")
    t = t.float()
    if t.dim() != 2 or t.shape[0] < 1:
        raise ValueError(f"{path}: text embeddings must be [P, C], not {tuple(t.shape)}")
    return t


def load_voxels(path):
    """(xyz float32 [n,3], avg_feats [n,C], voxel_coords int32 [n,3] or None) of an aggregation result."""
    d = torch.load(path, map_location="cpu")
    if "xyz" not in d or "avg_feats" not in d:
        raise KeyError(f"{path}: needs 'xyz' and 'avg_feats' (found {list(d)})")
    return d["xyz"].float(), d["avg_feats"], d.get("voxel_coords")


def query(feats, text, scale, device):
    """(labels int32, logits f32 [n,P], margin f32) of the table on `device`; non-finite rows get label -1 (reported)."""
    rows = feats.to(device)
    if rows.dtype not in (torch.float16, torch.float32):
        rows = rows.float()
    if rows.shape[1] != text.shape[1]:
        raise ValueError(f"the table has {rows.shape[1]} channels, the text embeddings {text.shape[1]}")
    labels, logits, margin = voxproj_host.query_features(rows, text.to(device), scale, check=False)
    n_bad = int((labels < 0).sum())
    if n_bad:
        print(f"[QUERY] warning: {n_bad} feature row(s) hold a non-finite value: label -1, NaN logits")
    return labels, logits, margin


def write_npz(path, labels, logits, prompts, colors=None):
    d = dict(labels=np.asarray(labels).astype(np.int16), logits=np.asarray(logits, dtype=np.float32), prompts=np.array(prompts))
    if colors is not None:
        d["colors"] = np.asarray(colors, dtype=np.uint8)
    np.savez(path, **d)


def write_ply(path, xyz, colors):
    """ASCII PLY: float x y z, uchar red green blue per vertex."""
    xyz = np.asarray(xyz, dtype=np.float32)
    colors = np.asarray(colors, dtype=np.uint8)
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\n")
        f.write(f"element vertex {xyz.shape[0]}\n")
        f.write("property float x\nproperty float y\nproperty float z\n")
        f.write("property uchar red\nproperty uchar green\nproperty uchar blue\n")
        f.write("end_header\n")
        for p, c in zip(xyz.tolist(), colors.tolist()):
            f.write(f"{p[0]} {p[1]} {p[2]} {c[0]} {c[1]} {c[2]}\n")


def summary(labels, logits, prompts):
    """The reference scripts' label histogram and per-class logit statistics."""
    labels = np.asarray(labels)
    print("\n[SUMMARY] Label distribution:")
    unique, counts = np.unique(labels, return_counts=True)
    for i, c in zip(unique.tolist(), counts.tolist()):
        name = prompts[i] if 0 <= i < len(prompts) else f"Label {i}"
        print(f"  {name:20s} (idx={i}): count={c}")
    print("\n[SUMMARY] Logit statistics per class:")
    for i, name in enumerate(prompts):
        v = np.asarray(logits)[:, i]
        v = v[np.isfinite(v)]
        if v.size:
            print(f"  {name:20s} (idx={i}): min={v.min():.4f} max={v.max():.4f} mean={v.mean():.4f} std={v.std():.4f} count={v.size}")


def _stem(out):
    return out[:-4] if out.endswith(".npz") else out


def _cmd_voxels(args, text, dev):
    xyz, feats, _ = load_voxels(args.vox)
    labels, logits, _ = query(feats, text, args.logit_scale, dev)
    lab, lg = labels.cpu().numpy(), logits.cpu().numpy()
    colors = label_colors(lab, len(args.prompt))
    write_npz(args.out, lab, lg, args.prompt, colors)
    ply = _stem(args.out) + "_colored_voxels.ply"
    write_ply(ply, xyz.numpy(), colors)
    print(f"[QUERY] {len(lab)} voxel labels, logits and colors -> {args.out}; coloured voxels -> {ply}")
    summary(lab, lg, args.prompt)


def lifted_labels(feats, weight, labels, logits):
    """Labels and logits of directly lifted rows: a Gaussian without a feature gets -1 and zero logits.  It has none when its
    weight is 0 or its row is all zeros: lift_gaussian_features.py zeroes the rows below --min_weight, and a mean that rounds
    to zeros in fp16 (tiny or cancelling features) has no direction to compare with a text embedding either."""
    valid = ((feats != 0).any(dim=1) & (weight > 0)).to(labels.device)
    return (torch.where(valid, labels, torch.full_like(labels, -1)),
            torch.where(valid[:, None], logits, torch.zeros((), dtype=logits.dtype, device=logits.device)))


def _cmd_gaussians_lifted(args, text, dev):
    import lift_gaussian_features
    mu, feats, weight = lift_gaussian_features.load_lifted(args.gauss_feats)
    labels, logits, _ = query(feats, text, args.logit_scale, dev)
    labels, logits = lifted_labels(feats, weight, labels, logits)
    lab, lg = labels.cpu().numpy(), logits.cpu().numpy()
    colors = label_colors(lab, len(args.prompt))
    write_npz(args.out, lab, lg, args.prompt)
    ply = _stem(args.out) + "_colored_gaussians.ply"
    write_ply(ply, mu.numpy(), colors)
    print(f"[QUERY] {len(lab)} Gaussian labels and logits from lifted rows ({int((lab < 0).sum())} without a feature) -> "
          f"{args.out}; coloured Gaussians -> {ply}")
    summary(lab, lg, args.prompt)


def _cmd_gaussians(args, text, dev):
    if args.gauss_feats:
        return _cmd_gaussians_lifted(args, text, dev)
    xyz, feats, _ = load_voxels(args.vox)
    mu = torch.from_numpy(np.load(args.gauss)).float()
    if mu.dim() != 2 or mu.shape[1] != 3:
        raise ValueError(f"{args.gauss}: Gaussian centres must be [M, 3], not {tuple(mu.shape)}")
    if args.map:
        g2v = torch.from_numpy(np.load(args.map)).long()
        if g2v.shape != (mu.shape[0],) or bool((g2v < 0).any()) or bool((g2v >= xyz.shape[0]).any()):
            raise ValueError(f"{args.map}: the map must hold one voxel index in [0, {xyz.shape[0]}) per Gaussian")
    else:
        import voxel_to_gaussian_map
        g2v = voxel_to_gaussian_map.map_gaussians_to_voxels(xyz, mu, device=dev)
    labels, logits, _ = query(feats, text, args.logit_scale, dev)
    idx = g2v.to(dev)
    lab, lg = labels[idx].cpu().numpy(), logits[idx].cpu().numpy()
    colors = label_colors(lab, len(args.prompt))
    write_npz(args.out, lab, lg, args.prompt)
    ply = _stem(args.out) + "_colored_gaussians.ply"
    write_ply(ply, mu.numpy(), colors)
    print(f"[QUERY] {len(lab)} Gaussian labels and logits -> {args.out}; coloured Gaussians -> {ply}")
    summary(lab, lg, args.prompt)


def _cmd_views(args, text, dev):
    import aggregate_voxel_features_onthefly as agg
    import build_sparse_occupancy as bso
    import prepare_tensor_data as ptd
    voxel_size, grid_origin, _, _ = bso.extract_voxel_params(args.voxel_ply)
    occ3 = bso.build_occupancy(bso.read_voxel_ply(args.voxel_ply), grid_origin, voxel_size, device=dev)
    occ = occ3.unsqueeze(0).long().contiguous()
    n_rows = int(occ3.max().item()) + 1
    _, feats, coords = load_voxels(args.features_pt)
    if coords is None:
        raise KeyError(f"{args.features_pt}: needs 'voxel_coords' to place its rows in the occupancy grid")
    # the occupancy ID of every feature row, with render_voxel_features.load_table's checks (inside the grid, in an occupied cell)
    zyx = coords.to(dev).long()
    if zyx.dim() != 2 or zyx.shape != (len(feats), 3):
        raise ValueError(f"{args.features_pt}: voxel_coords must be [n,3] with one row per avg_feats row")
    if not bool(((zyx >= 0) & (zyx < torch.tensor(occ3.shape, device=dev))).all()):
        raise ValueError(f"{args.features_pt}: voxel_coords lie outside the occupancy grid {tuple(occ3.shape)}")
    row_ids = occ3[zyx[:, 0], zyx[:, 1], zyx[:, 2]].long()
    if bool((row_ids == 0).any()):
        raise ValueError(f"{args.features_pt}: feature rows sit in empty cells of the occupancy grid (is --voxel_ply the grid "
                         "the aggregation used?)")
    labels, logits, margin = query(feats, text, args.logit_scale, dev)        # the file's rows as they are (fp16)
    P = text.shape[0]
    lab_tab = torch.full((n_rows,), -1, dtype=torch.int32, device=dev)
    conf_tab = torch.zeros(n_rows, dtype=torch.float32, device=dev)
    logit_tab = torch.zeros((n_rows, P), dtype=torch.float32, device=dev)
    lab_tab[row_ids] = labels
    conf_tab[row_ids] = torch.where(labels >= 0, margin, torch.zeros((), device=dev))
    logit_tab[row_ids] = torch.where((labels >= 0)[:, None], logits, torch.zeros((), device=dev))
    by_name, cams = ptd.load_camera_params(args.cam_params)
    names = args.views if args.views else sorted(by_name)[:args.max_images]
    os.makedirs(args.out_dir, exist_ok=True)
    all_labels = []
    ws = voxproj_host.Workspace()
    try:
        for name in names:
            entry = by_name.get(name)
            if entry is None:
                raise KeyError(f"no camera entry for {name}")
            H0, W0 = agg._image_size(entry, cams, args.images_dir, name)
            H, W = int(H0 * args.downsample_factor), int(W0 * args.downsample_factor)
            intr, c2w = ptd.camera_for(entry, cams, args.downsample_factor)
            ids = voxproj_host.first_hit_ids(occ, c2w.reshape(-1).to(dev), intr.reshape(1, 4).to(dev),
                                             agg.ray_opts(W, H, voxel_size), grid_origin, voxel_size, H, W, n_rows, workspace=ws)[0, 0]
            lab_img = lab_tab[ids.long()]                                  # ID 0 (a miss): row 0 never has a feature -> -1
            conf_img = conf_tab[ids.long()]
            stem = os.path.join(args.out_dir, name)
            np.save(stem + "_labels.npy", lab_img.to(torch.int16).cpu().numpy())
            np.save(stem + "_confidence.npy", conf_img.cpu().numpy())
            if args.save_logits:
                img = voxproj_host.render_features(ids, logit_tab, dtype=torch.float16)      # [H,W,P]
                np.save(stem + "_logits.npy", img.permute(2, 0, 1).contiguous().cpu().numpy())
            if args.save_ids:
                np.save(stem + "_ids.npy", ids.cpu().numpy())
            all_labels.append(lab_img.reshape(-1).cpu().numpy())
            print(f"[QUERY] {name}: {W}x{H}, {int((lab_img >= 0).sum())} labelled pixels -> {stem}_labels.npy")
    finally:
        ws.release()
    print(f"[QUERY] {len(feats)} voxel rows queried")
    summary(labels.cpu().numpy(), logits.cpu().numpy(), args.prompt)
    if all_labels:
        pix = np.concatenate(all_labels)
        print("\n[SUMMARY] Pixel labels over the views (-1: no feature row):")
        for i, c in zip(*np.unique(pix, return_counts=True)):
            print(f"  {(args.prompt[i] if i >= 0 else 'unlabelled'):20s} (idx={i}): count={c}")


def rendered_labels(img, alpha, labels, margin, logits=None):
    """Labels, confidence and logits of a rendered view: a pixel without a feature gets label -1, confidence 0 and zero
    logits.  It has none where alpha is 0 (no Gaussian reaches it) or its rendered row [C] is all zeros -- the rule
    ``lifted_labels`` applies to the Gaussians.  img [H,W,C], alpha [H,W], labels / margin [H*W], logits [H*W,P] or None."""
    H, W = alpha.shape
    valid = ((img != 0).any(dim=2) & (alpha > 0)).reshape(-1)
    zero = torch.zeros((), dtype=torch.float32, device=labels.device)
    lab = torch.where(valid, labels, torch.full_like(labels, -1)).reshape(H, W)
    conf = torch.where(valid & (labels >= 0), margin, zero).reshape(H, W)
    if logits is not None:
        logits = torch.where((valid & (labels >= 0))[:, None], logits, zero).reshape(H, W, -1)
    return lab, conf, logits


def _cmd_gaussian_views(args, text, dev):
    import gaussian_views
    import render_gaussian_features as rgf
    g, rows = rgf.load_scene(args, dev)
    if rows.shape[1] != text.shape[1]:
        raise ValueError(f"the rows have {rows.shape[1]} channels, the text embeddings {text.shape[1]}")
    os.makedirs(args.out_dir, exist_ok=True)
    ws = voxproj_host.SplatWorkspace()
    t = text.to(dev)
    all_labels = []
    for name, vm, K, W, H in gaussian_views.iter_views(args):
        # the view channels-last in fp16, then the query on the [H W, C] map in place: cosine normalisation per pixel,
        # after the blend
        img, alpha, _, _ = voxproj_host.splat_render_view(g["means"], g["quats"], g["scales"], g["opacities"], rows, vm, K, W, H,
                                                          dtype=torch.float16, want_alpha=True, workspace=ws, check=False)
        labels, logits, margin = voxproj_host.query_features(img.view(H * W, -1), t, args.logit_scale,
                                                             want_logits=args.save_logits, check=False)
        lab_img, conf_img, logit_img = rendered_labels(img, alpha, labels, margin, logits)
        stem = os.path.join(args.out_dir, name)
        np.save(stem + "_labels.npy", lab_img.to(torch.int16).cpu().numpy())
        np.save(stem + "_confidence.npy", conf_img.cpu().numpy())
        if args.save_logits:
            np.save(stem + "_logits.npy", logit_img.permute(2, 0, 1).contiguous().to(torch.float16).cpu().numpy())
        all_labels.append(lab_img.reshape(-1).cpu().numpy())
        print(f"[QUERY] {name}: {W}x{H}, {int((lab_img >= 0).sum())} labelled pixels -> {stem}_labels.npy")
    pix = np.concatenate(all_labels)
    print("\n[SUMMARY] Pixel labels over the views (-1: no rendered feature):")
    for i, c in zip(*np.unique(pix, return_counts=True)):
        print(f"  {(args.prompt[i] if i >= 0 else 'unlabelled'):20s} (idx={i}): count={c}")


def build_parser():
    import aggregate_voxel_features_onthefly as agg
    import gaussian_views
    ap = argparse.ArgumentParser(description="Score voxel features against text embeddings (GPU)")
    sub = ap.add_subparsers(dest="cmd", required=True)

    def common(p):
        p.add_argument("--text_emb", required=True, help="text embeddings [P, C] (.npy or .pt), one row per --prompt")
        p.add_argument("--prompt", nargs="+", required=True, help="the P prompt names, in the order of the embedding rows")
        p.add_argument("--logit_scale", type=float, default=1.0, help="logit multiplier (1.0: cosine; LSeg: its logit_scale)")

    v = sub.add_parser("voxels", help="label every voxel (voxeltovoxel_logits.py query)")
    common(v)
    v.add_argument("--vox", required=True, help="ALL_nonzero_voxel_features_*.pt of the aggregator")
    v.add_argument("--out", required=True, help="output .npz")
    g = sub.add_parser("gaussians", help="label every Gaussian through its 1-NN voxel (voxeltoGaussian_logits.py query)")
    common(g)
    g.add_argument("--vox", default=None, help="ALL_nonzero_voxel_features_*.pt of the aggregator (with --gauss)")
    g.add_argument("--gauss", default=None, help="Gaussian centres [M, 3] (.npy)")
    g.add_argument("--map", default=None, help="Gaussian -> voxel index [M] (.npy); computed when absent")
    g.add_argument("--gauss_feats", default=None,
                   help="LIFTED.pt of lift_gaussian_features.py: query the Gaussians' own rows (instead of --vox / --gauss / --map); "
                        "weight 0 or an all-zero row: label -1")
    g.add_argument("--out", required=True)
    w = sub.add_parser("views", help="semantic segmentation of camera views from the voxel grid")
    common(w)
    w.add_argument("--features_pt", required=True, help="ALL_nonzero_voxel_features_*.pt of the aggregator")
    w.add_argument("--voxel_ply", default=agg.VOXEL_PLY)
    w.add_argument("--cam_params", default=agg.CAM_PARAMS_ORIG)
    w.add_argument("--images_dir", default="")
    w.add_argument("--views", nargs="*", default=None)
    w.add_argument("--max_images", type=int, default=agg.MAX_IMAGES)
    w.add_argument("--downsample_factor", type=float, default=agg.DOWNSAMPLE_FACTOR)
    w.add_argument("--out_dir", default="semantic_views")
    w.add_argument("--save_logits", action="store_true", help="also write <name>_logits.npy f16 [P,H,W]")
    w.add_argument("--save_ids", action="store_true", help="also write <name>_ids.npy: the first-hit voxel ID image")
    # render_gaussian_features.py's arguments (tests/test_splat_render_cpu.py holds the two lists together); gaussian_views
    # imports nothing at module level that the other sub-commands do not need
    r = sub.add_parser("gaussian_views", help="semantic segmentation of camera views from the Gaussians' own rendered rows")
    common(r)
    gaussian_views.add_view_arguments(r)
    r.add_argument("--gauss_feats", required=True, help="LIFTED.pt of lift_gaussian_features.py: one feature row per Gaussian")
    r.add_argument("--out_dir", required=True)
    r.add_argument("--save_logits", action="store_true", help="also write <name>_logits.npy f16 [P,H,W]")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    text = load_text(args.text_emb)
    if len(args.prompt) != text.shape[0]:
        ap.error(f"{len(args.prompt)} prompts for {text.shape[0]} embedding rows in {args.text_emb}")
    if args.cmd == "gaussians":
        if args.gauss_feats and (args.vox or args.map or args.gauss):
            ap.error("--gauss_feats cannot be combined with --vox / --gauss / --map")
        if not args.gauss_feats and not (args.vox and args.gauss):
            ap.error("gaussians needs --vox and --gauss, or --gauss_feats")
    if not (args.logit_scale > 0 and np.isfinite(args.logit_scale)):
        ap.error(f"--logit_scale must be finite and > 0, not {args.logit_scale}")
    if not torch.cuda.is_available():
        raise RuntimeError("query_voxel_features runs on the GPU: there is no CPU path")
    dev = torch.device("cuda", torch.cuda.current_device())
    {"voxels": _cmd_voxels, "gaussians": _cmd_gaussians, "views": _cmd_views,
     "gaussian_views": _cmd_gaussian_views}[args.cmd](args, text, dev)


if __name__ == "__main__":
    main()
