"""Render an aggregation result into camera views: for every pixel, the fused feature of the voxel its ray hits first.

Reads the per-voxel table that aggregate_voxel_features_onthefly.py writes (ALL_nonzero_voxel_features_*.pt: avg_feats f16
[n,C], voxel_coords i32 [n,3] as (z,y,x)) and, per view, writes ``<name>_fused.npy`` -- float16 [C,H,W], the layout of the
LSeg feature maps (script/extract_lseg_features.py:97), so the LSeg text head and any other 2D consumer read it unchanged.

The occupancy grid, the cameras, the image sizes and the ray options are the aggregator's own (bso.build_occupancy,
ptd.camera_for, _image_size, ray_opts), so a view renders the same first-hit assignment the aggregation projected with.
Pixels whose ray hits nothing, and pixels whose voxel has no row in the table (occupied but never seen), are zeros; the ID
image (``--save_ids``: ``<name>_ids.npy``, int32 [H,W], 0 = miss) tells the two apart.

Both steps run on the GPU (vp_first_hit_ids, vp_render_features); there is no CPU path.
"""
import argparse
import os

import numpy as np
import torch

import aggregate_voxel_features_onthefly as agg
import build_sparse_occupancy as bso
import prepare_tensor_data as ptd
import voxproj_host


def load_table(features_pt, occ3, n_rows, device):
    """rows float32 [n_rows, C]: rows[occ[z,y,x]] = avg_feats for every (z,y,x) of the file, zeros elsewhere."""
    d = torch.load(features_pt, map_location="cpu")
    coords = d["voxel_coords"].to(device=device, dtype=torch.long)
    feats = d["avg_feats"].to(device=device, dtype=torch.float32)
    if coords.dim() != 2 or coords.shape[1] != 3 or coords.shape[0] != feats.shape[0]:
        raise ValueError(f"{features_pt}: voxel_coords must be [n,3] with one row per avg_feats row")
    Z, Y, X = occ3.shape
    inside = ((coords >= 0) & (coords < torch.tensor([Z, Y, X], device=device))).all(dim=1)
    if not bool(inside.all()):
        raise ValueError(f"{features_pt}: {int((~inside).sum())} voxel_coords lie outside the occupancy grid {tuple(occ3.shape)}")
    ids = occ3[coords[:, 0], coords[:, 1], coords[:, 2]].long()
    if bool((ids == 0).any()):
        raise ValueError(f"{features_pt}: {int((ids == 0).sum())} feature rows sit in empty cells of the occupancy grid "
                         "(is --voxel_ply the grid the aggregation used?)")
    rows = torch.zeros((n_rows, feats.shape[1]), dtype=torch.float32, device=device)
    rows[ids] = feats
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description="Render fused voxel features into camera views")
    ap.add_argument("--features_pt", required=True, help="ALL_nonzero_voxel_features_*.pt of the aggregator")
    ap.add_argument("--voxel_ply", default=agg.VOXEL_PLY)
    ap.add_argument("--cam_params", default=agg.CAM_PARAMS_ORIG)
    ap.add_argument("--images_dir", default="", help="image sizes are read from here (else the camera JSON's)")
    ap.add_argument("--views", nargs="*", default=None, help="image names to render (default: the first --max_images "
                    "names of the camera file, sorted)")
    ap.add_argument("--max_images", type=int, default=agg.MAX_IMAGES)
    ap.add_argument("--downsample_factor", type=float, default=agg.DOWNSAMPLE_FACTOR)
    ap.add_argument("--out_dir", default="fused_feature_views")
    ap.add_argument("--save_ids", action="store_true", help="also write <name>_ids.npy: the first-hit voxel ID image")
    args = ap.parse_args(argv)

    if not torch.cuda.is_available():
        raise RuntimeError("render_voxel_features runs on the GPU: there is no CPU path")
    dev = torch.device("cuda", torch.cuda.current_device())
    voxel_size, grid_origin, _, _ = bso.extract_voxel_params(args.voxel_ply)
    occ3 = bso.build_occupancy(bso.read_voxel_ply(args.voxel_ply), grid_origin, voxel_size, device=dev)
    occ = occ3.unsqueeze(0).long().contiguous()
    n_rows = int(occ3.max().item()) + 1
    rows = load_table(args.features_pt, occ3, n_rows, dev)
    by_name, cams = ptd.load_camera_params(args.cam_params)
    names = args.views if args.views else sorted(by_name)[:args.max_images]
    os.makedirs(args.out_dir, exist_ok=True)
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
                                             agg.ray_opts(W, H, voxel_size), grid_origin, voxel_size, H, W, n_rows, workspace=ws)
            img = voxproj_host.render_features(ids, rows, dtype=torch.float16)          # [1,1,H,W,C]
            stem = os.path.join(args.out_dir, name)
            np.save(stem + "_fused.npy", img[0, 0].permute(2, 0, 1).contiguous().cpu().numpy())
            if args.save_ids:
                np.save(stem + "_ids.npy", ids[0, 0].cpu().numpy())
            print(f"[RENDER] {name}: {W}x{H}, {int((ids > 0).sum())} pixels hit a voxel -> {stem}_fused.npy")
    finally:
        ws.release()          # drains and forgets the library's record before the memory goes back to torch


if __name__ == "__main__":
    main()
