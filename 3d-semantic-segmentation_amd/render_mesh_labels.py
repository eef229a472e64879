"""Render ground-truth label maps from an annotated mesh (ScanNet++'s mesh_aligned_0.05_semantic.ply) on the GPU: the maps
evaluate_label_maps.py --gt scores predictions against, at the size, camera and pixel centres render_semantics_logits.py and
query_voxel_features.py views give the predictions (gaussian_views.open_views), so the two align pixel for pixel.

The counterpart of the reference's debug_checks_scripts/render_scannetpp.py, which draws flat colours with Open3D's off-screen
renderer and decodes the labels from 8-bit colours.  Here voxproj_host.mesh_render rasterizes the faces themselves (the
contract is in include/voxproj_mesh.h): the label of a pixel is exactly the majority label of the nearest face's vertices,
both sides of a face are drawn, and the near plane is --near (0.01), not Open3D's.

Labels are made dense as the reference's build_dense_map does: the sorted unique raw vertex labels without --ignore_label
become 0 .. K-1, --ignore_label becomes 255; the vote of a face is taken on the dense labels, so the ignore label loses a
three-way tie.  label_mapping.json {raw: dense} is written to --out_dir, or read from --label_mapping so that several scenes
share one map (a raw label the map does not know is ignored, and counted).

Per view, under --out_dir:
  <name>.png            8-bit mode L: the dense class per pixel, 255 where nothing is drawn or the label is ignored
  <name>_depth.npy      f32 [H,W], 0 where nothing is drawn (--save_depth)
  <name>_face_ids.npy   i32 [H,W], -1 where nothing is drawn (--save_ids)
<name> is the view's image name without its extension, or with --index_names its 5-digit position in the run, which is how
render_semantics_logits.py names its files.
"""
import argparse
import json
import os

import numpy as np

import gaussian_views
import mesh_ply

IGNORE_DENSE = 255


def build_dense_map(raw, ignore_label=-100):
    """{raw label: dense index}: the sorted unique labels without ``ignore_label`` -> 0 .. K-1, ``ignore_label`` -> 255."""
    uniq = np.unique(np.asarray(raw))
    uniq = uniq[uniq != ignore_label]
    if len(uniq) > IGNORE_DENSE:
        raise ValueError(f"{len(uniq)} classes: an 8-bit label map holds at most {IGNORE_DENSE}")
    m = {int(lbl): i for i, lbl in enumerate(uniq)}
    m[int(ignore_label)] = IGNORE_DENSE
    return m


def load_dense_map(path):
    with open(path) as f:
        m = {int(k): int(v) for k, v in json.load(f).items()}
    if not all(0 <= v <= IGNORE_DENSE for v in m.values()):
        raise ValueError(f"{path}: dense labels must lie in [0, {IGNORE_DENSE}]")
    return m


def apply_dense_map(raw, m):
    """(dense u8 labels, the number of vertices whose raw label the map does not know: they are ignored)."""
    raw = np.asarray(raw)
    keys = np.array(sorted(m), np.int64)
    vals = np.array([m[k] for k in keys.tolist()], np.uint8)
    pos = np.minimum(np.searchsorted(keys, raw), len(keys) - 1)
    known = keys[pos] == raw
    return np.where(known, vals[pos], IGNORE_DENSE).astype(np.uint8), int((~known).sum())


def build_parser():
    ap = argparse.ArgumentParser(description="Render ground-truth label maps from an annotated mesh (GPU triangle rasterizer)")
    ap.add_argument("--mesh_ply", required=True, help="binary little-endian triangle mesh with an integer vertex property 'label'")
    ap.add_argument("--cam_params", required=True, help="camera_params.json")
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--images_dir", default="", help="the images, for their size (else the camera's width / height)")
    ap.add_argument("--views", nargs="*", default=None, help="image names (default: all, sorted)")
    ap.add_argument("--max_images", type=int, default=None, help="only the first N of those views")
    ap.add_argument("--downsample_factor", type=float, default=None, help="override the 1600-pixel width rule")
    ap.add_argument("--principal_point", choices=("center", "camera"), default="center")
    ap.add_argument("--label_mapping", default="", help="read {raw: dense} from this JSON instead of building it from the mesh")
    ap.add_argument("--ignore_label", type=int, default=-100, help="the raw label that becomes 255")
    ap.add_argument("--save_depth", action="store_true", help="also <name>_depth.npy")
    ap.add_argument("--save_ids", action="store_true", help="also <name>_face_ids.npy")
    ap.add_argument("--index_names", action="store_true", help="name the files 00000, 00001, ... as render_semantics_logits.py does")
    ap.add_argument("--near", type=float, default=0.01)
    ap.add_argument("--far", type=float, default=100.0)
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if not 0 < args.near < args.far:
        ap.error("need 0 < --near < --far")
    dev = gaussian_views.require_gpu("render_mesh_labels")
    import torch
    from PIL import Image

    import voxproj_host
    mesh = mesh_ply.read_mesh_ply(args.mesh_ply)
    if mesh["labels"] is None:
        raise ValueError(f"{args.mesh_ply}: the vertices carry no 'label' property")
    mapping = load_dense_map(args.label_mapping) if args.label_mapping else build_dense_map(mesh["labels"], args.ignore_label)
    dense, unknown = apply_dense_map(mesh["labels"], mapping)
    if unknown:
        print(f"[MESH] warning: {unknown} vertices carry a label that {args.label_mapping} does not know: ignored")
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "label_mapping.json"), "w") as f:
        f.write(json.dumps({str(k): v for k, v in sorted(mapping.items())}, indent=1) + "\n")
    verts, faces = torch.from_numpy(mesh["verts"]).to(dev), torch.from_numpy(mesh["faces"]).to(dev)
    vlab = torch.from_numpy(dense).to(dev)
    names, view = gaussian_views.open_views(args)
    ws = voxproj_host.SplatWorkspace()
    for idx, name in enumerate(names):
        vm, K, W, H = view(name)
        ids, depth, labels, counters = voxproj_host.mesh_render(verts, faces, vlab, vm, K, W, H, near=args.near, far=args.far,
                                                                workspace=ws)
        stem = f"{idx:05d}" if args.index_names else os.path.splitext(os.path.basename(name))[0]
        lab = labels.cpu().numpy()
        Image.fromarray(lab, mode="L").save(os.path.join(args.out_dir, stem + ".png"))
        if args.save_depth:
            np.save(os.path.join(args.out_dir, stem + "_depth.npy"), depth.cpu().numpy())
        if args.save_ids:
            np.save(os.path.join(args.out_dir, stem + "_face_ids.npy"), ids.cpu().numpy())
        uncovered = float((ids < 0).sum().item()) / (W * H)
        bad = counters.tolist()
        print(f"[MESH] {stem} {name}: {W}x{H}, uncovered {100.0 * uncovered:.3f} %, dropped faces: {bad[0]} bad index, "
              f"{bad[1]} non-finite, {bad[2]} beyond the guard band")
    print(f"[MESH] {len(names)} view(s), {len({v for v in mapping.values() if v != IGNORE_DENSE})} classes ->{args.out_dir}")


if __name__ == "__main__":
    main()
