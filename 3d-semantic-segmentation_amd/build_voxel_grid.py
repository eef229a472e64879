"""Stage 2, "sparse voxel grid initialization": point_cloud.ply -> the *_grid.ply that aggregate_voxel_features_onthefly.py
--voxel_ply reads.  Counterpart of the reference's script/minkowski_voxel_grid_from_ply_advanced.py, whole on the GPU: the
ball searches of the normal-consistency and density filters (cKDTree.query_ball_point in Python loops there) are the HIP
kernel vp_ball_count, the voxelisation (np.unique and a per-voxel mask loop there) is vp_voxel_grid; torch only moves,
sorts and compacts the columns.  include/voxproj_grid.h states the arithmetic, tests/voxel_grid_reference.py states it in
NumPy, tests/golden/voxel_grid_golden.npz holds the reference script's own output.

The reference's flags and defaults, and two more:
  --activated  feed the filters read_gaussian_ply's activated scales (exp) and opacities (sigmoid) instead of the columns as
               stored.  The reference (and the default here) takes the stored LOG scales: every negative log is clamped to
               1e-6, so the spikiness filter removes nothing, and the adaptive radius is |mean log scale| clipped to
               [eps / 2, 2 eps].  The opacity rank is the same either way (the sigmoid is monotonic) up to float32 ties.
  --device     the GPU (there is no CPU path).
--scale_threshold is accepted and unused, as in the reference.  Normals: 3DGS writes zero normals, on which the reference's
normal filter (run whenever nx ny nz exist and --normal_consistency < 1) rejects every Gaussian; pass --normal_consistency 1
for such files, as the reference's shipped shell script does.  Ties of the opacity at the cut go to the lowest index (the
reference's argpartition leaves them unspecified).  A filter that leaves nothing raises an error that names it.
"""
import argparse
import os
import re

import numpy as np
import torch

import voxproj_host

DEFAULTS = dict(cell_size=0.05, density_eps=0.05, density_min_neighbors=10, opacity_threshold=0.9, scale_threshold=0.0,
                spikiness_threshold=10.0, adaptive_density=False, normal_consistency=0.9, normal_consistency_eps=0.05,
                normal_consistency_min_neighbors=5)


def load_columns(path, activated=False):
    """dict(xyz f32 [N,3], opacity f32 [N], scales f32 [N,3] or None, f_dc f32 [N,3], normals f32 [N,3] or None) of a
    point_cloud.ply, the columns as stored; ``activated``: scales and opacity from read_gaussian_ply instead."""
    import gaussian_ply
    v = gaussian_ply.read_vertex_records(path)
    names = v.dtype.names
    for need in ("x", "y", "z", "opacity", "f_dc_0", "f_dc_1", "f_dc_2"):
        if need not in names:
            raise ValueError(f"{path}: no '{need}' property")
    col = lambda keys: np.stack([v[k] for k in keys], axis=1).astype(np.float32)  # noqa: E731
    scale_f = [f"scale_{i}" for i in range(3) if f"scale_{i}" in names]
    out = dict(xyz=col("xyz"), opacity=v["opacity"].astype(np.float32), scales=col(scale_f) if scale_f else None,
               f_dc=col(("f_dc_0", "f_dc_1", "f_dc_2")), normals=col(("nx", "ny", "nz")) if all(k in names for k in ("nx", "ny", "nz")) else None)
    if out["scales"] is not None and out["scales"].shape[1] != 3:
        raise ValueError(f"{path}: needs scale_0..2 or no scale column (found {scale_f})")
    if activated:
        g = gaussian_ply.read_gaussian_ply(path)
        out.update(scales=g["scales"], opacity=g["opacities"])
    return out


def _f32_quotient(a, b):
    """a / b of float32 tensors, correctly rounded: the float64 quotient rounded once more is the float32 one (53 >= 2 24 + 2)."""
    return (a.double() / b.double()).float()


def _scalar32(v, dev):
    return torch.tensor(float(v), dtype=torch.float32, device=dev)


@torch.no_grad()
def build_voxel_grid(ply_or_dict, *, cell_size=0.05, density_eps=0.05, density_min_neighbors=10, opacity_threshold=0.9,
                     scale_threshold=0.0, spikiness_threshold=10.0, adaptive_density=False, normal_consistency=0.9,
                     normal_consistency_eps=0.05, normal_consistency_min_neighbors=5, activated=False, device="cuda",
                     log=None):
    """The whole stage on ``device``.  ``ply_or_dict``: a point_cloud.ply path, or the dict load_columns returns (NumPy
    arrays or tensors).  Returns dict(centers f32 [V,3], colors uint8 [V,3], counts int32 [V], voxel_index int32 [V,3],
    grid_origin f32 [3], all on the device; voxel_size; survivors {stage: count}; kept int64 [n]: the rows of the input
    that reach the grid, ascending).  ``log``: a function for the reference's [INFO] lines (the command line prints them)."""
    del scale_threshold                                   # accepted and unused, as in the reference
    say = log if log is not None else (lambda s: None)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("build_voxel_grid needs a GPU: there is no CPU path")
    cols = load_columns(ply_or_dict, activated) if isinstance(ply_or_dict, (str, os.PathLike)) else ply_or_dict
    t = lambda a: None if a is None else torch.as_tensor(a).to(dev, torch.float32).contiguous()  # noqa: E731
    xyz, opacity, scales, f_dc, normals = (t(cols.get(k)) for k in ("xyz", "opacity", "scales", "f_dc", "normals"))
    N = int(xyz.shape[0])
    say(f"[INFO] Loaded input PLY with {N} points.")
    if N == 0:
        raise ValueError("the input holds no Gaussian")
    colors = (f_dc.clamp(_scalar32(0, dev), _scalar32(1, dev)) * _scalar32(255, dev)).to(torch.uint8)
    if normals is not None:
        sq = (normals[:, 0] * normals[:, 0] + normals[:, 1] * normals[:, 1]) + normals[:, 2] * normals[:, 2]
        norm = torch.sqrt(sq.double()).float()            # the float32 root, correctly rounded (as _f32_quotient)
        normals = _f32_quotient(normals, (norm + _scalar32(1e-8, dev))[:, None])
    alive = torch.arange(N, device=dev)
    surv = {"loaded": N}
    mean_scale = None
    if scales is not None:
        clamped = torch.maximum(scales, _scalar32(1e-6, dev))
        keep = _f32_quotient(clamped.max(1).values, clamped.min(1).values) < _scalar32(spikiness_threshold, dev)
        n_spiky = int((~keep).sum())
        if n_spiky:
            say(f"Filtered out {n_spiky} spiky Gaussians (ratio > {spikiness_threshold})")
        alive = alive[keep]
        mean_scale = _f32_quotient((scales[:, 0] + scales[:, 1]) + scales[:, 2], _scalar32(3, dev))
    surv["spikiness"] = int(alive.numel())
    if not alive.numel():
        raise ValueError("the spikiness filter left no Gaussian")
    keep_fraction = 1.0 - float(opacity_threshold)
    n_total = int(alive.numel())
    n_keep = max(1, int(n_total * keep_fraction))
    order = torch.sort(opacity[alive], descending=True, stable=True).indices[:n_keep]      # ties: the lowest index first
    alive = alive[torch.sort(order).values]
    surv["opacity"] = int(alive.numel())
    say(f"[INFO] Filtered to {alive.numel()} points with top {int(100 * keep_fraction)}% opacity (N={n_keep} of {n_total})")
    if normals is not None and normal_consistency < 1.0:
        say(f"[INFO] Filtering by normal consistency: min_dot={normal_consistency}, eps={normal_consistency_eps}, "
            f"min_neighbors={normal_consistency_min_neighbors}")
        cnt, con = voxproj_host.ball_count(xyz[alive], float(normal_consistency_eps), normals=normals[alive],
                                           min_dot=float(normal_consistency))
        m = int(normal_consistency_min_neighbors)
        alive = alive[(cnt >= m) & (con >= m)]
        surv["normal_consistency"] = int(alive.numel())
        say(f"[INFO] Kept {alive.numel()} / {n_total} gaussians after normal consistency filtering.")
        if not alive.numel():
            raise ValueError("the normal consistency filter left no Gaussian (3DGS writes zero normals: pass normal_consistency=1.0)")
    before = int(alive.numel())
    if adaptive_density and mean_scale is not None:
        radii = torch.clamp(mean_scale[alive].abs(), _scalar32(float(density_eps) / 2, dev), _scalar32(float(density_eps) * 2, dev))
        cnt, _ = voxproj_host.ball_count(xyz[alive], radii)
        alive = alive[cnt > int(density_min_neighbors)]
        say(f"[INFO] Adaptive density: Kept {alive.numel()} / {before} gaussians after density filtering.")
    else:
        say(f"[INFO] Filtering by local density: eps={density_eps}, min_neighbors={density_min_neighbors}")
        cnt, _ = voxproj_host.ball_count(xyz[alive], float(density_eps))
        alive = alive[cnt > int(density_min_neighbors)]
        say(f"[INFO] Kept {alive.numel()} / {before} gaussians after density filtering.")
    surv["density"] = int(alive.numel())
    if not alive.numel():
        raise ValueError("the density filter left no Gaussian")
    say(f"Using specified voxel size: {float(cell_size):.6f}")
    g = voxproj_host.voxel_grid(xyz[alive], colors[alive], float(cell_size))
    if int(g["status"].item()):
        raise ValueError("the voxel grid has a cell index above 2^21 - 1 or a non-finite point: no grid written")
    say(f"[INFO] Sparse voxel grid: {g['centers'].shape[0]} voxels")
    surv["voxels"] = int(g["centers"].shape[0])
    return dict(centers=g["centers"], colors=g["colors"], counts=g["counts"], voxel_index=g["voxel_index"],
                grid_origin=g["min_corner"], voxel_size=float(cell_size), survivors=surv, kept=alive)


def grid_file_name(ply_path, n_voxels, opacity_threshold, cell_size, density_eps, density_min_neighbors):
    """The reference's naming rule: {scene}_minkowski_{V}vox_iter{iter}_opac{..}_cell{..}_eps{..}_neig{..}_grid.ply, the scene
    the directory above 'point_cloud' (or the third path part from the end), iter from 'iteration_<n>' in the file's base name."""
    parts = ply_path.split(os.sep)
    try:
        scene = parts[parts.index("point_cloud") - 1]
    except Exception:
        scene = parts[-3] if len(parts) > 3 else parts[0]
    m = re.search(r"iteration_(\d+)", os.path.splitext(os.path.basename(ply_path))[0])
    return (f"{scene}_minkowski_{n_voxels}vox_iter{m.group(1) if m else ''}_opac{opacity_threshold}_cell{cell_size}"
            f"_eps{density_eps}_neig{density_min_neighbors}_grid.ply")


def write_grid_ply(path, centers, colors, voxel_size, grid_origin):
    """The reference's ASCII grid file: comment voxel_size / grid_origin, x y z red green blue.  Every float32 is printed as
    the Python float of its value (17 significant digits at most), so it reads back as the same float32."""
    xyz = np.asarray(centers, np.float32)
    rgb = np.asarray(colors, np.uint8)
    o = [float(v) for v in np.asarray(grid_origin, np.float32)]
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\n"
                f"comment voxel_size {voxel_size}\n"
                f"comment grid_origin {o[0]} {o[1]} {o[2]}\n"
                f"element vertex {xyz.shape[0]}\n"
                "property float x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
        f.write("".join(f"{x} {y} {z} {r} {g} {b}\n" for (x, y, z), (r, g, b) in zip(xyz.astype(np.float64).tolist(), rgb.tolist())))


def build_parser():
    p = argparse.ArgumentParser(description="Sparse voxel grid from a Gaussian .ply with adaptive filtering, on the GPU")
    p.add_argument("--ply", required=True, help="Input .ply file with Gaussian properties")
    p.add_argument("--output_dir", default="output/minkowski_grid", help="Output directory")
    p.add_argument("--cell_size", type=float, default=0.05, help="Base size of voxel grid cells")
    p.add_argument("--density_eps", type=float, default=0.05, help="Epsilon radius for density filtering")
    p.add_argument("--density_min_neighbors", type=int, default=10, help="Minimum neighbors for density filtering")
    p.add_argument("--opacity_threshold", type=float, default=0.9, help="Keep the top (1 - threshold) fraction by opacity")
    p.add_argument("--scale_threshold", type=float, default=0.0, help="Accepted and unused, as in the reference")
    p.add_argument("--spikiness_threshold", type=float, default=10.0, help="Maximum ratio of largest to smallest scale")
    p.add_argument("--adaptive_density", action="store_true", help="Density radius from the local scale")
    p.add_argument("--normal_consistency", type=float, default=0.9, help="Minimum dot product for normal consistency filtering")
    p.add_argument("--normal_consistency_eps", type=float, default=0.05, help="Neighborhood radius for normal consistency filtering")
    p.add_argument("--normal_consistency_min_neighbors", type=int, default=5, help="Minimum neighbors for normal consistency filtering")
    p.add_argument("--activated", action="store_true", help="Filter on activated scales and opacities (not in the reference)")
    p.add_argument("--device", default="cuda", help="The GPU to run on (there is no CPU path)")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    os.makedirs(args.output_dir, exist_ok=True)
    g = build_voxel_grid(args.ply, **{k: getattr(args, k) for k in DEFAULTS}, activated=args.activated, device=args.device, log=print)
    centers, colors = g["centers"].cpu().numpy(), g["colors"].cpu().numpy()
    path = os.path.join(args.output_dir, grid_file_name(args.ply, centers.shape[0], args.opacity_threshold, args.cell_size,
                                                        args.density_eps, args.density_min_neighbors))
    write_grid_ply(path, centers, colors, args.cell_size, g["grid_origin"].cpu().numpy())
    print(f"[INFO] Saved sparse voxel grid to {path}")
    return path


if __name__ == "__main__":
    main()
