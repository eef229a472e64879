"""The Gaussian splatting contract (include/voxproj.h, vp_splat_*) in float64 NumPy, shared by test_splat_cpu.py and
test_gpu_splat.py.  No tiles: every Gaussian is tried at every pixel, in (fp32 z, index) order.

Only the depth is replayed in fp32 (((r20 mx + r21 my) + r22 mz) + t2, the sort key and the near / far test); mean2d and the
conic are computed in float64 and rounded to fp32 once, as the kernel stores them; everything after is float64.

Besides the images, splat64 returns a fragile mask: pixels where some decision of some Gaussian lies within a relative
FRAGILE_REL band of its threshold (alpha vs 1/255, Tn vs 1e-4, o exp(-sigma) vs the 0.999 clamp, sigma vs 0), where an
fp32 evaluation may decide the other way and change the pixel's sum by a whole term.
"""
import numpy as np

ALPHA_MIN = 1.0 / 255.0
T_MIN = 1e-4
ALPHA_MAX = 0.999
FRAGILE_REL = 1e-5


def depth32(means, viewmat):
    """fp32 depth in the contract's operation order (numpy float32 arithmetic rounds every operation)."""
    m = np.asarray(means, np.float32)
    r = np.asarray(viewmat, np.float32)
    return ((r[2, 0] * m[:, 0] + r[2, 1] * m[:, 1]) + r[2, 2] * m[:, 2]) + r[2, 3]


def quat_to_rot(q):
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([
        np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
        np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
        np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)


def project(means, quats, scales, opacities, viewmat, K, W, H, near=0.01, far=1e10, eps2d=0.3):
    """Per Gaussian: (keep bool [N], z32 [N], mean2d [N,2], conic [N,3] (A, B, C), cov2d [N,3] (s00, s01, s11), bad [N]);
    mean2d and conic already rounded to fp32 (values float64)."""
    means = np.asarray(means, np.float32)
    quats = np.asarray(quats, np.float32)
    scales = np.asarray(scales, np.float32)
    op = np.asarray(opacities, np.float32)
    N = len(means)
    bad = ~(np.isfinite(means).all(1) & np.isfinite(quats).all(1) & np.isfinite(scales).all(1) & np.isfinite(op))
    with np.errstate(all="ignore"):
        z32 = depth32(means, viewmat)
        qn = (quats.astype(np.float64) ** 2).sum(1)
        keep = ~bad & (z32 >= np.float32(near)) & (z32 <= np.float32(far)) & (qn > 0) & (op.astype(np.float64) >= ALPHA_MIN)
        vm = np.asarray(viewmat, np.float32).astype(np.float64)
        Rw, t = vm[:3, :3], vm[:3, 3]
        fx, fy, cx, cy = (float(np.float32(K[0][0])), float(np.float32(K[1][1])), float(np.float32(K[0][2])),
                          float(np.float32(K[1][2])))
        q = np.where(keep[:, None], quats.astype(np.float64), [1.0, 0.0, 0.0, 0.0])
        M = quat_to_rot(q) * np.where(keep[:, None], scales, 0.0)[:, None, :]
        V = Rw[None] @ M
        S = V @ V.transpose(0, 2, 1)
        p = np.where(keep[:, None], means, 0.0) @ Rw.T + t
        z = np.where(keep, p[:, 2], 1.0)
        limxp, limxn = (W - cx) / fx + 0.3 * (0.5 * W) / fx, cx / fx + 0.3 * (0.5 * W) / fx
        limyp, limyn = (H - cy) / fy + 0.3 * (0.5 * H) / fy, cy / fy + 0.3 * (0.5 * H) / fy
        ux, uy = p[:, 0] / z, p[:, 1] / z
        tx, ty = z * np.clip(ux, -limxn, limxp), z * np.clip(uy, -limyn, limyp)
        J = np.zeros((N, 2, 3))
        J[:, 0, 0], J[:, 0, 2] = fx / z, -fx * tx / (z * z)
        J[:, 1, 1], J[:, 1, 2] = fy / z, -fy * ty / (z * z)
        S2 = J @ S @ J.transpose(0, 2, 1)
        s00, s01, s11 = S2[:, 0, 0] + eps2d, S2[:, 0, 1], S2[:, 1, 1] + eps2d
        det = s00 * s11 - s01 * s01
        keep &= det > 0
        mean2d = np.stack([fx * ux + cx, fy * uy + cy], 1)
        keep &= np.isfinite(mean2d).all(1)
        conic = np.stack([s11 / det, -s01 / det, s00 / det], 1)
    r32 = lambda a: np.where(keep[:, None] if a.ndim == 2 else keep, a, 0.0).astype(np.float32).astype(np.float64)  # noqa: E731
    return keep, z32, r32(mean2d), r32(conic), np.stack([s00, s01, s11], 1), bad


def half_extents(opacity, cov2d):
    """(rx, ry): the axis-aligned half-extents of the support sigma <= ln(255 o)."""
    ext = 2.0 * np.maximum(np.log(255.0 * np.asarray(opacity, np.float64)), 0.0)
    return np.sqrt(ext * cov2d[..., 0]), np.sqrt(ext * cov2d[..., 2])


def _near(v, thr, rel=FRAGILE_REL):
    return np.abs(v - thr) <= rel * abs(thr)


def splat64(means, quats, scales, opacities, features, viewmat, K, W, H, near=0.01, far=1e10, eps2d=0.3, value_tol=0.0):
    """dict(logits f64 [D,H,W], alpha [H,W], label int64 [H,W], confidence [H,W], fragile bool [H,W], bad bool [N],
    order (the kept Gaussians in blend order), visits int [H,W] (Gaussians added per pixel)).  value_tol: a pixel whose top-1
    minus top-2 logit gap is <= value_tol is fragile too (its label may go either way within the value bound)."""
    f = np.asarray(features, np.float64)
    D = f.shape[1]
    keep, z32, m2, con, _, bad = project(means, quats, scales, opacities, viewmat, K, W, H, near, far, eps2d)
    op = np.asarray(opacities, np.float32).astype(np.float64)
    idx = np.nonzero(keep)[0]
    order = idx[np.lexsort((idx, z32[idx]))]
    jj, ii = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    T = np.ones((H, W))
    out = np.zeros((D, H, W))
    live = np.ones((H, W), bool)
    fragile = np.zeros((H, W), bool)
    visits = np.zeros((H, W), np.int64)
    for g in order:
        if not live.any():
            break
        dx, dy = m2[g, 0] - jj, m2[g, 1] - ii
        A, B, C = con[g]
        sig = 0.5 * (A * dx * dx + C * dy * dy) + B * dx * dy
        raw = op[g] * np.exp(-sig)
        a = np.minimum(ALPHA_MAX, raw)
        tn = T * (1.0 - a)
        fragile |= live & (_near(raw, ALPHA_MAX) | _near(a, ALPHA_MIN) | (np.abs(sig) <= FRAGILE_REL) |
                           ((sig >= 0) & (a >= ALPHA_MIN) & _near(tn, T_MIN)))
        use = live & (sig >= 0) & (a >= ALPHA_MIN)
        stop = use & (tn <= T_MIN)
        add = use & ~stop
        w = np.where(add, a * T, 0.0)
        out += f[g][:, None, None] * w[None]
        T = np.where(add, tn, T)
        visits += add
        live &= ~stop
    label = out.argmax(axis=0)
    if D == 1:
        conf = np.ones((H, W))
    else:
        e = np.exp(out - out.max(axis=0, keepdims=True))
        p = e / e.sum(axis=0, keepdims=True)
        ps = np.sort(p, axis=0)
        conf = ps[-1] - ps[-2]
        srt = np.sort(out, axis=0)
        # a near tie: the label may go either way (an exact tie of two exact zeros, as padded channels give, may not)
        fragile |= ((srt[-1] - srt[-2]) <= value_tol) & ~((srt[-1] == 0) & (srt[-2] == 0))
    return dict(logits=out, alpha=1.0 - T, label=label, confidence=conf, fragile=fragile, bad=bad, order=order,
                visits=visits)


def value_bound(features, rel=1e-4, abs_=1e-6):
    """The bound test_gpu_splat.py holds every non-fragile logit to: rel * max_g |f_g| + abs_.  A pixel's logit is
    sum_g f_g w_g with sum_g w_g = 1 - T <= 1; the kernel's weights carry a relative error of a few 1e-6 (fp32 conic and
    exp, T as a running fp32 product), so rel = 1e-4 leaves a margin of more than 10x."""
    f = np.asarray(features, np.float64)
    return rel * (np.abs(f).max() if f.size else 0.0) + abs_
