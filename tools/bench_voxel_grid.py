"""Time stage 2 (vp_ball_count, vp_voxel_grid, build_voxel_grid) on synthetic_gaussians surfaces of 1 000 000 and 3 000 000
Gaussians at the settings of the reference's shipped shell script (cell 0.03, eps 0.10, 4 neighbours, adaptive density,
opacity 0.5), and beside it, in the same run on the same machine's CPUs, the reference's method at the same inputs.

One JSON line per size, device-event times (median of --reps windows after --warmup):
  ball_count_ms          voxproj_host.ball_count on the opacity survivors with the adaptive radii: bucketing (torch), the
                         kernel, and putting the rows back;  ball_kernel_ms: the kernel alone on a prepared bucketing
  candidate_pairs        the exact float64 tests the kernel makes (the points of every query's cell box), and per second
  voxel_grid_ms          voxproj_host.voxel_grid on the density survivors; grid_min_bytes = what the call must move at least
                         (points and colours in, every output out), copy_ms = a device copy that reads and writes that many
                         bytes in all, timed in this run
  build_voxel_grid_ms    the whole stage from columns on the device to the grid (one call per window)
  cpu_*                  scipy.spatial.cKDTree: query_ball_point(return_length=True, workers=16) at the fixed radius, the
                         reference's per-point Python loop at the adaptive radii on a stated subsample and SCALED to all
                         queries (cpu_adaptive_loop_scaled_s), np.unique(axis=0) plus a vectorised mean for the grid.
                         Without scipy the cpu_ball_* fields are null and "scipy" is false.
GPU only: without a device the program fails, it does not fall back.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-semantic-segmentation_amd"))

OPTS = dict(cell_size=0.03, density_eps=0.10, density_min_neighbors=4, opacity_threshold=0.5, adaptive_density=True,
            normal_consistency=1.0)


def timed(fn, warmup, reps, calls=1):
    import torch
    out = None
    for _ in range(warmup):
        out = fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            out = fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / calls)
    return float(np.median(times)), out


def candidate_pairs(q, radii, start, origin, h, dims):
    """The number of points in every query's cell box, summed: k_ball_count's box arithmetic in torch, box sums from a 3D
    integral image of the cell counts."""
    import torch
    dev = q.device
    cnt = (start[1:] - start[:-1]).double().reshape(dims[2], dims[1], dims[0])
    integral = torch.zeros((dims[2] + 1, dims[1] + 1, dims[0] + 1), dtype=torch.float64, device=dev)
    integral[1:, 1:, 1:] = cnt.cumsum(0).cumsum(1).cumsum(2)
    lo = torch.tensor(origin, dtype=torch.float64, device=dev)
    r = radii.double().abs()[:, None]
    c0 = torch.floor((q.double() - r - lo) / h).long() - 1
    c1 = torch.floor((q.double() + r - lo) / h).long() + 1
    top = torch.tensor(dims, device=dev) - 1
    c0, c1 = torch.maximum(c0, torch.zeros_like(c0)), torch.minimum(c1, top) + 1           # [c0, c1) per axis
    total = torch.zeros(len(q), dtype=torch.float64, device=dev)
    for sx, x in ((1, c1[:, 0]), (-1, c0[:, 0])):
        for sy, y in ((1, c1[:, 1]), (-1, c0[:, 1])):
            for sz, z in ((1, c1[:, 2]), (-1, c0[:, 2])):
                total += sx * sy * sz * integral[z, y, x]
    return int(total.sum().item())


def cpu_baseline(xyz, radii, eps, kept_xyz, kept_rgb, cell, subsample):
    out = dict(scipy=False, cpu_ball_fixed_s=None, cpu_adaptive_loop_scaled_s=None, cpu_adaptive_subsample=None)
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    if cKDTree is not None:
        p = xyz.astype(np.float64)
        t0 = time.perf_counter()
        tree = cKDTree(p)
        t_tree = time.perf_counter() - t0
        t0 = time.perf_counter()
        tree.query_ball_point(p, r=eps, return_length=True, workers=16)
        t_fixed = time.perf_counter() - t0
        pick = np.random.default_rng(0).permutation(len(p))[:subsample]
        t0 = time.perf_counter()
        for i in pick:                                       # the reference's loop: one Python call per point
            len(tree.query_ball_point(xyz[i], r=radii[i]))
        t_loop = (time.perf_counter() - t0) * len(p) / len(pick)
        out.update(scipy=True, cpu_tree_build_s=t_tree, cpu_ball_fixed_s=t_fixed, cpu_adaptive_loop_scaled_s=t_loop,
                   cpu_adaptive_subsample=int(len(pick)))
    t0 = time.perf_counter()
    mc = kept_xyz.min(axis=0)
    idx = np.floor((kept_xyz - mc) / cell).astype(int)
    uniq, inverse, counts = np.unique(idx, axis=0, return_inverse=True, return_counts=True)
    sums = np.stack([np.bincount(inverse.reshape(-1), weights=kept_rgb[:, c], minlength=len(uniq)) for c in range(3)], 1)
    (sums / counts[:, None]).astype(np.float32).astype(np.uint8)
    out["cpu_grid_unique_mean_s"] = time.perf_counter() - t0
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="Time stage 2 on the GPU beside the reference's CPU method")
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 3_000_000])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu_subsample", type=int, default=2000, help="points of the adaptive CPU loop (scaled to all)")
    ap.add_argument("--no_cpu", action="store_true", help="skip the CPU baseline")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    args = ap.parse_args(argv)
    import torch

    import build_voxel_grid as bvg
    import gaussian_views
    import synthetic_gaussians as sg
    import voxel_to_gaussian_map
    import voxproj_host as vh
    dev = gaussian_views.require_gpu("bench_voxel_grid")
    for n in args.sizes:
        g = sg.make_gaussians(n, seed=28)
        op, ls, _ = sg.to_ply_fields(g)
        f_dc = np.random.default_rng(28).uniform(-0.2, 1.2, (n, 3)).astype(np.float32)
        cols = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)
                for k, v in dict(xyz=g["means"], opacity=op, scales=ls, f_dc=f_dc).items()}
        t_all, res = timed(lambda: bvg.build_voxel_grid(cols, device=dev, **OPTS), 1, max(args.reps // 2, 1))
        # the two calls on their own inputs: the opacity survivors with their radii, the density survivors
        order = torch.sort(cols["opacity"], descending=True, stable=True).indices[:max(1, int(n * 0.5))]
        alive = torch.sort(order).values
        xyz = cols["xyz"][alive].contiguous()
        mean = ((cols["scales"][:, 0] + cols["scales"][:, 1]) + cols["scales"][:, 2]).double().div(3.0).float()[alive]
        radii = mean.abs().clamp(0.05, 0.2)
        t_ball, (cnt, _) = timed(lambda: vh.ball_count(xyz, radii), args.warmup, args.reps)
        pts, perm, start, origin, h, dims = voxel_to_gaussian_map._bucket(xyz, dev, min_cell=float(radii.max()))
        rs = radii[perm.long()].contiguous()
        out_cnt = torch.empty(len(xyz), dtype=torch.int32, device=dev)
        origin_c = (ctypes.c_double * 3)(*origin)

        def kernel():
            vh._call(dev, "vp_ball_count", pts.data_ptr(), perm.data_ptr(), start.data_ptr(), origin_c, ctypes.c_double(h), dims[0],
                     dims[1], dims[2], pts.data_ptr(), len(xyz), ctypes.c_double(0.0), rs.data_ptr(), None, None,
                     ctypes.c_double(0.0), out_cnt.data_ptr(), None)

        t_kernel, _ = timed(kernel, args.warmup, args.reps)
        pairs = candidate_pairs(pts, rs, start, origin, h, dims)
        keep = cnt > OPTS["density_min_neighbors"]
        kx = xyz[keep].contiguous()
        kc = (cols["f_dc"][alive][keep].clamp(0, 1) * 255).to(torch.uint8).contiguous()
        ws = vh.SplatWorkspace()
        t_grid, grid = timed(lambda: vh.voxel_grid(kx, kc, OPTS["cell_size"], workspace=ws), args.warmup, args.reps)
        V, nk = int(grid["centers"].shape[0]), int(kx.shape[0])
        assert V == res["survivors"]["voxels"] and nk == res["survivors"]["density"]
        min_bytes = nk * (12 + 3 + 4) + V * (12 + 3 + 4 + 12)
        src = torch.empty(min_bytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        t_copy, _ = timed(lambda: dst.copy_(src), args.warmup, args.reps, calls=10)
        line = dict(gaussians=n, settings=OPTS, survivors=res["survivors"], bucket_cell=h, bucket_dims=dims, ball_queries=len(xyz),
                    radius_min=float(radii.min()), radius_max=float(radii.max()), mean_count=float(cnt.float().mean()),
                    ball_count_ms=t_ball, ball_kernel_ms=t_kernel, candidate_pairs=pairs,
                    candidate_pairs_per_s=pairs / (t_kernel * 1e-3), voxel_grid_ms=t_grid, grid_points=nk, voxels=V,
                    grid_min_bytes=min_bytes, copy_ms=t_copy, grid_bytes_per_s=min_bytes / (t_grid * 1e-3),
                    copy_bytes_per_s=min_bytes / (t_copy * 1e-3), build_voxel_grid_ms=t_all,
                    ball_kernel_shape="one lane per query in cell order (the only shape built)")
        if not args.no_cpu:
            line.update(cpu_baseline(xyz.cpu().numpy(), radii.cpu().numpy(), OPTS["density_eps"], kx.cpu().numpy(), kc.cpu().numpy(),
                                     OPTS["cell_size"], args.cpu_subsample))
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
