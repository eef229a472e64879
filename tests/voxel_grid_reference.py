"""The contract of include/voxproj_grid.h in NumPy: stage 2 of the pipeline, the sparse voxel grid of a Gaussian cloud (the
reference: script/minkowski_voxel_grid_from_ply_advanced.py).  Brute force and float64 where the contract says float64,
float32 where it says float32; the device path (vp_ball_count, vp_voxel_grid, build_voxel_grid.py) equals this twin value for
value, and this twin equals the reference script's output on tests/golden/voxel_grid_golden.npz."""
import numpy as np


def colors_of(f_dc):
    """uint8(clip(f_dc, 0, 1) * 255) in float32, truncating."""
    return (np.clip(np.asarray(f_dc, np.float32), np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)


def unit_normals(n):
    """n / (|n| + 1e-8) in float32, |n| = sqrt((x x + y y) + z z)."""
    n = np.asarray(n, np.float32)
    norm = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    return n / (norm[:, None] + np.float32(1e-8))


def ball_stats(points, radius, queries=None, normals=None, query_normals=None, min_dot=None, want_gap=False):
    """(count int32 [M], consistent int32 [M] or None): per query the points with d2 <= r r, d2 = (dx dx + dy dy) + dz dz in
    float64 on the float64-converted fp32 differences; with normals those of them whose float64 dot product with the query's
    normal is > min_dot.  ``radius``: a scalar (taken as a double) or float32 [M].  ``want_gap`` adds min |d2 - r r|."""
    p = np.asarray(points, np.float32).astype(np.float64)
    q = p if queries is None else np.asarray(queries, np.float32).astype(np.float64)
    M = len(q)
    r = np.asarray(radius, np.float32).astype(np.float64) if np.ndim(radius) else np.full(M, float(radius))
    count = np.zeros(M, np.int32)
    consistent = None
    if normals is not None:
        pn = np.asarray(normals, np.float32).astype(np.float64)
        qn = pn if queries is None else np.asarray(query_normals, np.float32).astype(np.float64)
        consistent = np.zeros(M, np.int32)
    gap = np.inf
    for b in range(0, M, 512):
        e = min(b + 512, M)
        d = q[b:e, None, :] - p[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        r2 = (r[b:e] * r[b:e])[:, None]
        within = d2 <= r2
        count[b:e] = within.sum(axis=1)
        if want_gap and within.size:
            gap = min(gap, float(np.abs(d2 - r2).min()))
        if normals is not None:
            m = qn[b:e]
            dot = (m[:, None, 0] * pn[None, :, 0] + m[:, None, 1] * pn[None, :, 1]) + m[:, None, 2] * pn[None, :, 2]
            consistent[b:e] = (within & (dot > float(min_dot))).sum(axis=1)
    return (count, consistent, gap) if want_gap else (count, consistent)


def spikiness_keep(scales, threshold):
    s = np.asarray(scales, np.float32).copy()
    s[s < np.float32(1e-6)] = np.float32(1e-6)
    return (s.max(axis=1) / s.min(axis=1)) < np.float32(threshold)


def opacity_rank(opacity, threshold):
    """The indices (ascending) of the N_keep = max(1, int(N (1 - threshold))) largest opacities, ties to the lowest index."""
    n = len(opacity)
    n_keep = max(1, int(n * (1.0 - float(threshold))))
    order = np.argsort(-np.asarray(opacity, np.float32), kind="stable")
    return np.sort(order[:n_keep]), n_keep


def adaptive_radii(scales, eps):
    s = np.asarray(scales, np.float32)
    mean = ((s[:, 0] + s[:, 1]) + s[:, 2]) / np.float32(3)
    return np.clip(np.abs(mean), np.float32(eps / 2), np.float32(eps * 2)).astype(np.float32)


def voxelize(points, colors, voxel_size, keep=None):
    """dict(centers f32 [V,3], colors u8 [V,3], counts i32 [V], voxel_index i32 [V,3], point_voxel i32 [N], min_corner f32 [3],
    status): np.unique(axis=0) order.  status 1 (a non-finite kept point or a cell index above 2^21 - 1): V = 0."""
    p = np.asarray(points, np.float32)
    c = np.asarray(colors, np.uint8)
    n = len(p)
    sel = np.arange(n) if keep is None else np.flatnonzero(np.asarray(keep))
    empty = dict(centers=np.zeros((0, 3), np.float32), colors=np.zeros((0, 3), np.uint8), counts=np.zeros(0, np.int32),
                 voxel_index=np.zeros((0, 3), np.int32), point_voxel=np.full(n, -1, np.int32),
                 min_corner=np.full(3, np.inf, np.float32), status=0)
    if len(sel) == 0:
        return empty
    pk = p[sel]
    if not np.isfinite(pk).all():
        return dict(empty, status=1)
    mc = pk.min(axis=0)
    with np.errstate(over="ignore", invalid="ignore"):
        idx_f = np.floor((pk - mc) / np.float32(voxel_size))
    if not (np.isfinite(idx_f).all() and idx_f.max() <= 2 ** 21 - 1):
        return dict(empty, status=1)
    idx = idx_f.astype(np.int64)
    uniq, inverse, counts = np.unique(idx, axis=0, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    centers = (uniq.astype(np.float64) * float(voxel_size) + mc.astype(np.float64)).astype(np.float32)
    sums = np.zeros((len(uniq), 3), np.int64)
    np.add.at(sums, inverse, c[sel].astype(np.int64))
    vcol = (sums.astype(np.float64) / counts[:, None].astype(np.float64)).astype(np.float32).astype(np.uint8)
    point_voxel = np.full(n, -1, np.int32)
    point_voxel[sel] = inverse
    return dict(centers=centers, colors=vcol, counts=counts.astype(np.int32), voxel_index=uniq.astype(np.int32),
                point_voxel=point_voxel, min_corner=mc, status=0)


def pipeline(xyz, opacity, scales, f_dc, normals=None, *, cell_size=0.05, density_eps=0.05, density_min_neighbors=10,
             opacity_threshold=0.9, spikiness_threshold=10.0, adaptive_density=False, normal_consistency=0.9,
             normal_consistency_eps=0.05, normal_consistency_min_neighbors=5):
    """The whole stage on the columns as stored: dict(centers, colors, min_corner, survivors {stage: count})."""
    xyz, opacity, f_dc = np.asarray(xyz, np.float32), np.asarray(opacity, np.float32), np.asarray(f_dc, np.float32)
    colors = colors_of(f_dc)
    unit = unit_normals(normals) if normals is not None else None
    alive = np.arange(len(xyz))
    surv = {"loaded": len(xyz)}
    if scales is not None:
        scales = np.asarray(scales, np.float32)
        alive = alive[spikiness_keep(scales, spikiness_threshold)]
    surv["spikiness"] = len(alive)
    top, _ = opacity_rank(opacity[alive], opacity_threshold)
    alive = alive[top]
    surv["opacity"] = len(alive)
    if unit is not None and normal_consistency < 1.0:
        cnt, con = ball_stats(xyz[alive], normal_consistency_eps, normals=unit[alive], min_dot=normal_consistency)
        alive = alive[(cnt >= normal_consistency_min_neighbors) & (con >= normal_consistency_min_neighbors)]
        surv["normal_consistency"] = len(alive)
        if not len(alive):
            raise ValueError("the normal consistency filter left no Gaussian")
    if adaptive_density and scales is not None:
        cnt, _ = ball_stats(xyz[alive], adaptive_radii(scales[alive], density_eps))
    else:
        cnt, _ = ball_stats(xyz[alive], density_eps)
    alive = alive[cnt > density_min_neighbors]
    surv["density"] = len(alive)
    if not len(alive):
        raise ValueError("the density filter left no Gaussian")
    g = voxelize(xyz[alive], colors[alive], cell_size)
    return dict(g, survivors=surv, kept=alive)
