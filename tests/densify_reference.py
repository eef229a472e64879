"""Adaptive density control (include/voxproj.h, vp_densify_*) in NumPy, shared by test_densify_cpu.py and the
test_gpu_densify_*.py files.  Written from the contract, not from the kernels.

  plan_fused     the per-Gaussian rule and the fixed output order, as vp_densify_plan states them
  plan_literal   the reference's literal sequence (clone-append, split-append, remove the split sources, prune) with the
                 screen radius kept for original rows and 0 for new ones; test_densify_cpu.py holds the two to each other
  philox4x32_10, split_normals, split_geometry   the children's generator and geometry in float64
  accumulate     the per-view statistic applied to a grad_screen
  screen_radius  3 sqrt(lambda_max) from splat_reference._project's float64 cov2d
"""
import numpy as np

F32 = np.float32
CHILD_SCALE = F32(0.625)                       # 1 / (0.8 * 2), exact
CHILD_LOG = F32(np.log(0.625))                 # the fp32 nearest to ln 0.625


def _decide(grad_accum, denom, max_radius, scales, opacities, grad_threshold, size_threshold, min_opacity, max_screen_size,
            max_world_size):
    ga = np.asarray(grad_accum, F32)
    dn = np.asarray(denom, np.int32)
    sc = np.asarray(scales, F32).reshape(-1, 3)
    op = np.asarray(opacities, F32)
    thr, size, lo, scr, world = (F32(v) for v in (grad_threshold, size_threshold, min_opacity, max_screen_size, max_world_size))
    with np.errstate(all="ignore"):
        gm = np.where(dn != 0, ga / np.where(dn != 0, dn, 1).astype(F32), F32(0)).astype(F32)
        gm = np.where(np.isnan(gm), F32(0), gm)
        smax = np.fmax(np.fmax(sc[:, 0], sc[:, 1]), sc[:, 2]) if len(sc) else np.zeros(0, F32)
        sel = gm >= thr
        clone, split = sel & (smax <= size), sel & (smax > size)
        low = op < lo
        on = bool(scr > 0)
        bigw = on & (smax > world)
        bigw_child = on & ((smax * CHILD_SCALE).astype(F32) > world)
        bigv = (on & (np.asarray(max_radius, F32) > scr)) if max_radius is not None else np.zeros(len(ga), bool)
    return clone, split, low, bigw, bigw_child, bigv


def plan_fused(grad_accum, denom, max_radius, scales, opacities, *, grad_threshold, size_threshold, min_opacity,
               max_screen_size=0.0, max_world_size):
    """(src int32 [total], kind uint8 [total], counts int64 [4] = {total, kept, clones, splitting sources})."""
    clone, split, low, bigw, bigw_child, bigv = _decide(grad_accum, denom, max_radius, scales, opacities, grad_threshold,
                                                       size_threshold, min_opacity, max_screen_size, max_world_size)
    keep = ~split & ~low & ~bigv & ~bigw
    one = clone & ~low & ~bigw
    two = split & ~low & ~bigw_child
    k, c, s = np.nonzero(keep)[0], np.nonzero(one)[0], np.nonzero(two)[0]
    src = np.concatenate([k, c, s, s]).astype(np.int32)
    kind = np.concatenate([np.zeros(len(k)), np.ones(len(c)), np.full(len(s), 2), np.full(len(s), 3)]).astype(np.uint8)
    return src, kind, np.array([len(src), len(k), len(c), len(s)], np.int64)


def plan_literal(grad_accum, denom, max_radius, scales, opacities, *, grad_threshold, size_threshold, min_opacity,
                 max_screen_size=0.0, max_world_size):
    """The reference's sequence on explicit row lists (gaussian_model.py densify_and_clone, densify_and_split,
    densify_and_prune): every row carries (source, kind, its largest scale, its opacity, its screen radius)."""
    clone, split, _, _, _, _ = _decide(grad_accum, denom, max_radius, scales, opacities, grad_threshold, size_threshold,
                                       min_opacity, max_screen_size, max_world_size)
    sc = np.asarray(scales, F32).reshape(-1, 3)
    op = np.asarray(opacities, F32)
    n = len(op)
    with np.errstate(all="ignore"):
        smax = np.fmax(np.fmax(sc[:, 0], sc[:, 1]), sc[:, 2]) if n else np.zeros(0, F32)
    rad = np.asarray(max_radius, F32) if max_radius is not None else np.zeros(n, F32)
    rows = [(g, 0, smax[g], op[g], rad[g]) for g in range(n)]
    # densify_and_clone: append a copy of every selected small Gaussian; new rows have no radius yet
    rows += [(g, 1, smax[g], op[g], F32(0)) for g in range(n) if clone[g]]
    # densify_and_split: the mask is padded with False for the clones; two children per selected large Gaussian (all first
    # children, then all second children: the reference's repeat(2, 1)), scales / (0.8 * 2); then the sources are removed
    first = [(g, 2, F32(smax[g] * CHILD_SCALE), op[g], F32(0)) for g in range(n) if split[g]]
    second = [(g, 3, F32(smax[g] * CHILD_SCALE), op[g], F32(0)) for g in range(n) if split[g]]
    rows = [r for r in rows if not (r[1] == 0 and split[r[0]])] + first + second
    # prune: low opacity; with a screen size, big in view or big in the world
    lo, scr, world = F32(min_opacity), F32(max_screen_size), F32(max_world_size)
    out = []
    for g, kind, s, o, r in rows:
        bad = bool(o < lo)
        if scr > 0:
            bad = bad or bool(r > scr) or bool(s > world)
        if not bad:
            out.append((g, kind))
    src = np.array([g for g, _ in out], np.int32)
    kind = np.array([k for _, k in out], np.uint8)
    return src, kind, np.array([len(out), int((kind == 0).sum()), int((kind == 1).sum()), int((kind == 2).sum())], np.int64)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11).  counter uint32 [..., 4], key uint32 [..., 2] -> uint32 [..., 4]."""
    c = np.array(np.broadcast_arrays(*[np.asarray(counter, np.uint64)[..., i] for i in range(4)]), np.uint64)
    k = [np.uint64(v) for v in np.asarray(key, np.uint64).reshape(-1)[:2]]
    M0, M1, W0, W1, MASK = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85), \
        np.uint64(0xFFFFFFFF)
    sh = np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = np.array([(p1 >> sh) ^ c[1] ^ k[0], p1 & MASK, (p0 >> sh) ^ c[3] ^ k[1], p0 & MASK], np.uint64)
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return np.moveaxis(c, 0, -1).astype(np.uint32)


def split_normals(g, child, seed):
    """xi float64 [n, 3] of the children (source g, child 0 / 1): Box-Muller on Philox words, counter (g, c, 0, 0), key
    (seed & 0xffffffff, seed >> 32)."""
    g = np.asarray(g, np.uint64)
    ctr = np.stack([g, np.asarray(child, np.uint64), np.zeros_like(g), np.zeros_like(g)], -1)
    r = philox4x32_10(ctr, [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]).astype(np.float64)
    u = (r + 0.5) * 2.0 ** -32
    two_pi = 6.283185307179586
    r0, r2 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    return np.stack([r0 * np.cos(two_pi * u[:, 1]), r0 * np.sin(two_pi * u[:, 1]), r2 * np.cos(two_pi * u[:, 3])], 1)


def quat_to_rot(q):
    q = np.asarray(q, np.float32).astype(np.float64)
    q = q * (1.0 / np.sqrt((q * q).sum(1, keepdims=True)))
    w, x, y, z = q.T
    return np.stack([
        np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
        np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
        np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)


def split_geometry(means, quats, log_scales, src, kind, seed):
    """(out_means f32 [n,3], out_log_scales f32 [n,3], bound f64 [n,3]): bound is |mean_c| + sum_j |R_cj| s_j |xi_j| for the
    children (0 for copies), the magnitude the mean's tolerance is stated against."""
    means, quats, ls = np.asarray(means, F32), np.asarray(quats, F32), np.asarray(log_scales, F32)
    src, kind = np.asarray(src, np.int64), np.asarray(kind, np.uint8)
    om, ol = means[src].copy(), ls[src].copy()
    bound = np.zeros((len(src), 3))
    ch = np.nonzero(kind >= 2)[0]
    if len(ch):
        g = src[ch]
        xi = split_normals(g, kind[ch] - 2, seed)
        R = quat_to_rot(quats[g])
        v = np.exp(ls[g].astype(np.float64)) * xi
        off = (R[:, :, 0] * v[:, None, 0] + R[:, :, 1] * v[:, None, 1]) + R[:, :, 2] * v[:, None, 2]
        om[ch] = (means[g].astype(np.float64) + off).astype(F32)
        ol[ch] = (ls[g] + CHILD_LOG).astype(F32)
        bound[ch] = np.abs(means[g].astype(np.float64)) + (np.abs(R) * np.abs(v)[:, None, :]).sum(2)
    return om, ol, bound


def accumulate(grad_accum, denom, grad_screen, visible, W, H, scale=1.0):
    """The statistic after one more view: (grad_accum f32 [N], denom i32 [N]); untouched where not visible."""
    gs = np.asarray(grad_screen, F32)
    gx, gy = gs[:, 0].astype(np.float64), gs[:, 1].astype(np.float64)
    hw, hh = 0.5 * W, 0.5 * H
    with np.errstate(all="ignore"):
        norm = (np.sqrt(gx * gx * (hw * hw) + gy * gy * (hh * hh)) * float(F32(scale))).astype(F32)
        ga = np.where(visible, np.asarray(grad_accum, F32) + norm, grad_accum).astype(F32)
    dn = np.where(visible, np.asarray(denom, np.int32) + 1, denom).astype(np.int32)
    return ga, dn


def screen_radius(cov2d):
    """float64 [N]: 3 sqrt(mid + sqrt(max(0.1, ((s00 - s11) / 2)^2 + s01^2))) from cov2d [N,3] = (s00, s01, s11)."""
    s00, s01, s11 = np.asarray(cov2d, np.float64).T
    mid, hd = 0.5 * (s00 + s11), 0.5 * (s00 - s11)
    with np.errstate(all="ignore"):
        return 3.0 * np.sqrt(mid + np.sqrt(np.maximum(0.1, hd * hd + s01 * s01)))


def camera_extent(viewmats):
    """1.1 max |c_i - mean c| over the camera centres c = -R^T t (the reference's cameras_extent)."""
    vm = np.asarray(viewmats, np.float64).reshape(-1, 4, 4)
    c = -np.einsum("nji,nj->ni", vm[:, :3, :3], vm[:, :3, 3])
    return float(1.1 * np.linalg.norm(c - c.mean(0), axis=1).max())


def random_case(rng, n, ties=True):
    """(dict(grad_accum, denom, max_radius, scales, opacities), grad_threshold, size_threshold): statistics, scales and
    opacities around the thresholds, with denom = 0 rows and, with ``ties``, mean gradients exactly at the threshold (the
    denominators are powers of two, so the division gives the threshold back) and largest scales exactly at theirs."""
    thr, size = F32(0.0002), F32(0.05)
    denom = rng.choice(np.array([0, 1, 2, 4], np.int32), n)
    gm = (thr * np.exp(rng.normal(0, 1.0, n))).astype(F32)
    scales = (size * np.exp(rng.normal(0, 1.0, (n, 3)))).astype(F32)
    if ties and n:
        gm = np.where(rng.uniform(size=n) < 0.15, thr, gm).astype(F32)
        tie = np.nonzero(rng.uniform(size=n) < 0.15)[0]
        scales[tie] = np.minimum(scales[tie], size)
        scales[tie, rng.integers(0, 3, len(tie))] = size
    ga = (gm * np.maximum(denom, 1).astype(F32)).astype(F32)
    op = np.where(rng.uniform(size=n) < 0.2, rng.uniform(0.0, 0.01, n), rng.uniform(0.01, 1.0, n)).astype(F32)
    rad = rng.uniform(0.0, 40.0, n).astype(F32)
    return dict(grad_accum=ga, denom=denom.astype(np.int32), max_radius=rad, scales=scales, opacities=op), thr, size
