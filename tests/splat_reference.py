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
    return _project(means, quats, scales, opacities, viewmat, K, W, H, near, far, eps2d)[:6]


def _project(means, quats, scales, opacities, viewmat, K, W, H, near, far, eps2d):
    """project's tuple followed by the float64 mean2d before its rounding (0 where culled), which the support box uses."""
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
    return keep, z32, r32(mean2d), r32(conic), np.stack([s00, s01, s11], 1), bad, np.where(keep[:, None], mean2d, 0.0)


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
    sum_g f_g w_g with sum_g w_g = 1 - T <= 1; on well-conditioned Gaussians (test_gpu_splat.py's scenes) the kernel's
    weights carry a relative error of a few 1e-6 (fp32 conic and exp, T as a running fp32 product), so rel = 1e-4 leaves a
    margin of more than 10x.  Thin Gaussians across the pixel axes lose far more to the cancellation in fp32 sigma (up to
    3e-3 measured): value_bound_at below adds the derived term for them."""
    f = np.asarray(features, np.float64)
    return rel * (np.abs(f).max() if f.size else 0.0) + abs_


# ------------------------------------------------------------------------------------------------------------------------
# Sampled pixels and the conditioning-aware bound.
#
# splat64 is dense (every Gaussian at every pixel of the image) and cannot reach the sizes the path ships at; splat64_at is
# the same contract with the same decisions at a list of (row, col) pixels: one pixel against all kept Gaussians in blend
# order, the transmittance as an exclusive running product, cut at the first stop.  No tiles and no support box.
#
# The fp32 error of sigma.  The kernel evaluates, without contraction (-ffp-contract=off: no FMA),
#     dx = mx - sx;  dy = my - sy;  sigma = 0.5f * (A * dx * dx + C * dy * dy) + B * dx * dy
# on the fp32 records the oracle shares.  sx = px + 0.5 is exact.  Counting roundings (each a factor 1 + delta, |delta| <= u
# = 2^-24):  A dx dx carries dx twice (1 rounding each) and two products: 4; so does C dy dy; their sum adds 1 and the exact
# 0.5 none: 5; B dx dy carries dx, dy and two products: 4; the last sum adds 1 to both sides: 6 and 5.  So
#     |sigma32 - sigma64| <= gamma_6 (0.5 (A dx^2 + C dy^2) + |B dx dy|) = SIGMA_GAMMA u m,   SIGMA_GAMMA = 6 / (1 - 6 u).
# For a round Gaussian m ~ sigma <= ln 255 where it matters and the error is a few 1e-7.  For a thin Gaussian across the axes
# the three terms cancel: m reaches 1e4 .. 1e6 at a sigma of order 1, and the weight e^-sigma is off by SIGMA_GAMMA u m,
# 1e-3 .. 1e-1 relative.  (The factored form 0.5 (A (dx + (B/A) dy)^2 + dy^2 / s11) has no cancellation; it needs another
# record layout and is not what the kernel evaluates.)
#
# Carried through, with d = SIGMA_GAMMA u m of a pair:
#   a = min(0.999, o e^-sigma) is off by a factor within e^+-d (not at all on the clamp): the bands of a against 1/255, of
#   o e^-sigma against 0.999 and of sigma against 0 widen by d;
#   1 - a is off by at most x = a (e^d - 1) / (1 - a) relative, y = x / (1 - x) in the logarithm (x >= 1/2 makes the pixel
#   fragile); T before Gaussian k by a factor within e^+-D_k, D_k = sum of y over the Gaussians added before k; the band of
#   Tn against 1e-4 widens by D_k + y_k;
#   the weight w_k = a_k T_k by at most E_k = e^(d_k + D_k) - 1 relative, so a logit by extra_c = sum_k w_k |f_kc| E_k and
#   alpha by sum_k w_k E_k, on top of the flat bound that covers the roundings that do not depend on the conditioning
#   (exp, the products, the running sums).  Where m is small E is a few 1e-7 and the flat bound stands as it is.
# ------------------------------------------------------------------------------------------------------------------------
U32 = 2.0 ** -24
SIGMA_ROUNDINGS = 6
SIGMA_GAMMA = SIGMA_ROUNDINGS / (1.0 - SIGMA_ROUNDINGS * U32)
TILE = 16


def records(means, quats, scales, opacities, viewmat, K, W, H, near=0.01, far=1e10, eps2d=0.3):
    """The kept Gaussians' fp32 records in blend order (values float64): dict(order, mx, my, A, B, C, o, lo = ln(255 o), and
    per input Gaussian keep, z32, cov2d, mean2d64, bad)."""
    keep, z32, m2, con, cov, bad, m2d = _project(means, quats, scales, opacities, viewmat, K, W, H, near, far, eps2d)
    op = np.asarray(opacities, np.float32).astype(np.float64)
    idx = np.nonzero(keep)[0]
    order = idx[np.lexsort((idx, z32[idx]))]
    return dict(order=order, mx=m2[order, 0], my=m2[order, 1], A=con[order, 0], B=con[order, 1], C=con[order, 2],
                o=op[order], lo=np.log(255.0 * op[order]), keep=keep, z32=z32, cov2d=cov, mean2d64=m2d, bad=bad, W=W, H=H)


def tile_counts(rec, opacities, edge_tol=1e-9):
    """(count int64 [N], close bool [N]): the 16x16 tiles of each Gaussian's support box as the contract states it (the
    half_extents box around the float64 mean2d, one pixel wider on each side, clipped to the image); close marks the
    Gaussians with a box edge within edge_tol of an integer where that integer can change the tiles."""
    W, H, keep = rec["W"], rec["H"], rec["keep"]
    op = np.asarray(opacities, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        rx, ry = half_extents(np.where(keep, op, 1.0), rec["cov2d"])
    mx, my = rec["mean2d64"].T
    e = [mx - rx - 1.5, mx + rx + 0.5, my - ry - 1.5, my + ry + 0.5]
    jlo, jhi, ilo, ihi = np.floor(e[0]), np.ceil(e[1]), np.floor(e[2]), np.ceil(e[3])
    on = keep & np.isfinite(rx) & np.isfinite(ry) & (jhi >= 0) & (ilo <= H - 1) & (ihi >= 0) & (jlo <= W - 1)
    t = lambda v, hi: (np.clip(np.where(on, v, 0.0), 0, hi - 1).astype(np.int64)) // TILE  # noqa: E731
    count = np.where(on, (t(jhi, W) - t(jlo, W) + 1) * (t(ihi, H) - t(ilo, H) + 1), 0)
    close = np.zeros(len(keep), bool)
    for v, hi in zip(e, (W, W, H, H)):
        close |= keep & (v >= -2) & (v <= hi + 1) & (np.abs(v - np.round(v)) <= edge_tol)
    return count, close


def _band(v, thr, d, rel=FRAGILE_REL):
    """v e^+-d reaches the relative ``rel`` band of thr (d = 0: |v - thr| <= rel thr)."""
    d = np.minimum(d, 700.0)
    return (v * np.exp(-d) <= thr * (1.0 + rel)) & (v * np.exp(d) >= thr * (1.0 - rel))


def pixel64(rec, i, j, cond=True):
    """Pixel (row i, col j) against every kept Gaussian.  dict(sel: positions in rec['order'] of the added Gaussians, in
    order; a, T (before each), w = a T, e = e^-sigma, raw = o e, dx, dy, sig, m, E (the weight's relative error bound) per
    added Gaussian; T_final; S (the log-error of any product of the pixel's factors is within 2 S); fragile)."""
    with np.errstate(all="ignore"):
        dx, dy = rec["mx"] - (j + 0.5), rec["my"] - (i + 0.5)
        qa, qc, qb = rec["A"] * dx * dx, rec["C"] * dy * dy, rec["B"] * dx * dy
        sig = 0.5 * (qa + qc) + qb
        m = 0.5 * (qa + qc) + np.abs(qb)
        d = SIGMA_GAMMA * U32 * m if cond else np.zeros_like(m)
        # every Gaussian is tried; only those that can be used or lie in a band go on (the rest have o e^-sigma < e^-1 / 255)
        c = np.nonzero(sig - d <= rec["lo"] + 1.0)[0]
        sig, d, m, dx, dy = sig[c], d[c], m[c], dx[c], dy[c]
        e = np.exp(-sig)
        raw = rec["o"][c] * e
        a = np.minimum(ALPHA_MAX, raw)
        use = (sig >= 0) & (a >= ALPHA_MIN)
        fac = np.where(use, 1.0 - a, 1.0)
        cp = np.cumprod(fac)
        T = np.concatenate(([1.0], cp[:-1]))
        tn = T * (1.0 - a)
        stop = use & (tn <= T_MIN)
        k = np.arange(len(c))
        first = int(np.argmax(stop)) if stop.any() else len(c)
        live, add = k <= first, use & (k < first)
        if cond:
            dc = np.where(raw >= ALPHA_MAX, 0.0, d)                 # on the clamp a carries no error
            x = np.where(use, a * np.expm1(np.minimum(dc, 700.0)) / (1.0 - a), 0.0)
            y = np.where(x < 0.5, x / (1.0 - np.minimum(x, 0.5)), 0.0)
            ya = np.where(add, y, 0.0)
            D = np.cumsum(ya) - ya
            frag = live & (_band(raw, ALPHA_MAX, d) | _band(raw, ALPHA_MIN, d) | (np.abs(sig) <= FRAGILE_REL + d) |
                           (use & (_band(tn, T_MIN, D + y) | (x >= 0.5))))
            E = np.expm1(np.minimum(dc + D, 700.0))[add]
            S = float((dc + y)[add].sum())
        else:
            frag = live & (_near(raw, ALPHA_MAX) | _near(a, ALPHA_MIN) | (np.abs(sig) <= FRAGILE_REL) |
                           (use & _near(tn, T_MIN)))
            E, S = np.zeros(int(add.sum())), 0.0
    return dict(sel=c[add], a=a[add], T=T[add], w=a[add] * T[add], e=e[add], raw=raw[add], dx=dx[add], dy=dy[add],
                sig=sig[add], m=m[add], E=E, S=S, T_final=float(cp[first - 1]) if first > 0 else 1.0, fragile=bool(frag.any()))


def _label_conf(out):
    """(label, confidence) of one pixel's logits [D], as splat64's epilogue."""
    if len(out) == 1:
        return 0, 1.0
    e = np.exp(out - out.max())
    ps = np.sort(e / e.sum())
    return int(out.argmax()), float(ps[-1] - ps[-2])


def splat64_at(means, quats, scales, opacities, features, viewmat, K, W, H, pixels, near=0.01, far=1e10, eps2d=0.3,
               value_tol=0.0, cond=True, rec=None):
    """splat64 at the (row, col) ``pixels`` [P,2] only: dict(logits f64 [P,D], alpha [P], label int64 [P], confidence [P],
    fragile bool [P], visits int [P], bad, order, and extra [P,D], extra_alpha [P] (the conditioning terms of the bound),
    scale [P,D] = sum_g w_g |f_gc|).  ``cond`` False keeps splat64's flat bands (extra = 0): then fragile and label equal
    splat64's.  A pixel whose top-1 minus top-2 gap is <= value_tol + 2 max_c extra is fragile too.  ``rec``: records()
    of the same scene, to share the projection between calls."""
    f = np.asarray(features, np.float64)
    D = f.shape[1]
    rec = rec if rec is not None else records(means, quats, scales, opacities, viewmat, K, W, H, near, far, eps2d)
    pixels = np.asarray(pixels, np.int64).reshape(-1, 2)
    P = len(pixels)
    out, extra, scale = np.zeros((P, D)), np.zeros((P, D)), np.zeros((P, D))
    alpha, xalpha, conf = np.zeros(P), np.zeros(P), np.zeros(P)
    label, visits, fragile = np.zeros(P, np.int64), np.zeros(P, np.int64), np.zeros(P, bool)
    for p, (i, j) in enumerate(pixels):
        r = pixel64(rec, int(i), int(j), cond)
        fs = f[rec["order"][r["sel"]]]
        out[p] = r["w"] @ fs
        scale[p] = r["w"] @ np.abs(fs)
        extra[p] = (r["w"] * r["E"]) @ np.abs(fs)
        alpha[p], xalpha[p] = 1.0 - r["T_final"], float((r["w"] * r["E"]).sum())
        visits[p], fragile[p] = len(r["sel"]), r["fragile"]
        label[p], conf[p] = _label_conf(out[p])
        if D > 1:
            srt = np.sort(out[p])
            fragile[p] |= bool((srt[-1] - srt[-2]) <= value_tol + 2.0 * extra[p].max()) and \
                not (srt[-1] == 0 and srt[-2] == 0)
    return dict(logits=out, alpha=alpha, label=label, confidence=conf, fragile=fragile, visits=visits, bad=rec["bad"],
                order=rec["order"], extra=extra, extra_alpha=xalpha, scale=scale)


def value_bound_at(features, o, rel=1e-4, abs_=1e-6):
    """The conditioning-aware bound of every sampled logit, [P,D]: value_bound's flat rel * max|f| + abs_ plus splat64_at's
    extra = sum_g w_g |f_gc| E_g.  Equal to value_bound where the Gaussians a pixel adds are well conditioned."""
    return value_bound(features, rel, abs_) + o["extra"]


def sigma_pair(rec, i, j):
    """(sigma64, sigma32, m) of pixel (i, j) against every kept Gaussian: the float64 value, NumPy float32 replaying the
    kernel's expression, and the magnitude m of the bound |sigma32 - sigma64| <= SIGMA_GAMMA u m."""
    dx, dy = rec["mx"] - (j + 0.5), rec["my"] - (i + 0.5)
    qa, qc, qb = rec["A"] * dx * dx, rec["C"] * dy * dy, rec["B"] * dx * dy
    f32 = np.float32
    A, B, C = rec["A"].astype(f32), rec["B"].astype(f32), rec["C"].astype(f32)
    with np.errstate(all="ignore"):
        dx32, dy32 = rec["mx"].astype(f32) - f32(j + 0.5), rec["my"].astype(f32) - f32(i + 0.5)
        s32 = f32(0.5) * (A * dx32 * dx32 + C * dy32 * dy32) + B * dx32 * dy32
    return 0.5 * (qa + qc) + qb, s32.astype(np.float64), 0.5 * (qa + qc) + np.abs(qb)


def splat32_at(rec, features, pixels, flip_b=False):
    """The fp32 twin: the kernel's blend loop at the sampled pixels in NumPy float32, operation by operation in the kernel's
    order (np.exp on float32 stands in for __expf, a product and a sum for the accumulators' fmaf).  dict(logits f32 [P,D],
    alpha [P], label [P], confidence [P]).  It reads the records only: what it shows about the bound owes nothing to the GPU.
    ``flip_b`` negates the conic's B (a deliberately wrong twin, for the tests of the tests)."""
    f32 = np.float32
    f = np.asarray(features, f32)
    D = f.shape[1]
    mx, my, A, B, C, o = (rec[k].astype(f32) for k in ("mx", "my", "A", "B", "C", "o"))
    if flip_b:
        B = -B
    pixels = np.asarray(pixels, np.int64).reshape(-1, 2)
    P = len(pixels)
    out, alpha, conf, label = np.zeros((P, D), f32), np.zeros(P, f32), np.zeros(P, f32), np.zeros(P, np.int64)
    with np.errstate(all="ignore"):
        for p, (i, j) in enumerate(pixels):
            dx, dy = mx - f32(j + 0.5), my - f32(i + 0.5)
            sig = f32(0.5) * (A * dx * dx + C * dy * dy) + B * dx * dy
            c = np.nonzero(sig >= 0)[0]
            a = np.minimum(f32(ALPHA_MAX), o[c] * np.exp(-sig[c]))
            u = a >= f32(1.0) / f32(255.0)
            c, a = c[u], a[u]
            cp = np.cumprod(f32(1.0) - a, dtype=f32)              # sequential fp32 products, as T = T * (1 - a)
            T = np.concatenate((np.ones(1, f32), cp[:-1]))
            stop = cp <= f32(T_MIN)
            n = int(np.argmax(stop)) if stop.any() else len(c)
            w = (a * T)[:n]
            terms = f[rec["order"][c[:n]]] * w[:, None]
            out[p] = np.add.accumulate(terms, axis=0, dtype=f32)[-1] if n else 0
            alpha[p] = f32(1.0) - (cp[n - 1] if n else f32(1.0))
            label[p] = int(out[p].argmax())
            if D == 1:
                conf[p] = 1
            else:
                m1 = out[p].max()
                m2 = np.delete(out[p], label[p]).max()
                conf[p] = (f32(1.0) - np.exp(m2 - m1)) / np.add.accumulate(np.exp(out[p] - m1), dtype=f32)[-1]
    return dict(logits=out, alpha=alpha, label=label, confidence=conf)
