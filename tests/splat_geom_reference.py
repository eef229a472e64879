"""The geometry backward's contract (include/voxproj.h, vp_splat_rasterize_backward_geometry) in float64 NumPy, shared by
test_splat_geom_cpu.py and test_gpu_splat_geom.py.  It extends splat_grad_reference.splat_grad64's sweep (same decisions,
same dL/da) with the five screen-space sums per Gaussian and the per-Gaussian chain to the means, quaternions and scales.

For a pixel that added Gaussian g: d = mean2d - sample, q = dL/da * raw where raw = o e^-sigma < 0.999, else 0;
  g_mx = -sum q (A dx + B dy)   g_my = -sum q (B dx + C dy)   g_A = -sum q dx^2/2   g_B = -sum q dx dy   g_C = -sum q dy^2/2.
The chain is the adjoint of splat_reference.project's float64 projection (the clamped Jacobian branch is differentiated
where it is taken; the fp32 depth carries no gradient).  It is linear in the five sums, so it is returned as a Jacobian
jac [N,5,10] = d(mean2d x, y, conic A, B, C) / d(means 3, quats 4, scales 3) and grad_theta = sum_k grad_screen[k] jac[k].

Magnitude scales M_*: the same sums with every product replaced by its absolute value (per pair |A dx| + |B dy| and so on,
|dL/da| as in splat_grad_reference's M_o).

``round_records``: True keeps the contract's records (mean2d and conic rounded to fp32 once, as the kernel stores them);
False leaves them in float64, which makes the loss a smooth function of the geometry: the finite-difference target
(with rounded records a small geometric step moves the loss in fp32 stairs).  ``project64`` takes float64 geometry as it is.
"""
import numpy as np

import splat_reference as ref

THETA = 10           # means 3, quats 4, scales 3


def project64(means, quats, scales, opacities, viewmat, K, W, H, near=0.01, far=1e10, eps2d=0.3):
    """The float64 projection with its intermediates, nothing rounded but the depth: dict(keep, z32, mean2d [N,2],
    conic [N,3], and Rw, Rq, n, qn, s, V, S, J, JS, z, ux, uy, cux, cuy, inx, iny, fx, fy for the chain).  Culled Gaussians
    hold harmless values and keep = False."""
    m = np.asarray(means, np.float64)
    q = np.asarray(quats, np.float64)
    s = np.asarray(scales, np.float64)
    op = np.asarray(opacities, np.float64)
    N = len(m)
    bad = ~(np.isfinite(m).all(1) & np.isfinite(q).all(1) & np.isfinite(s).all(1) & np.isfinite(op))
    with np.errstate(all="ignore"):
        z32 = ref.depth32(m.astype(np.float32), viewmat)
        qn = np.sqrt((q ** 2).sum(1))
        keep = ~bad & (z32 >= np.float32(near)) & (z32 <= np.float32(far)) & (qn > 0) & (op >= ref.ALPHA_MIN)
        vm = np.asarray(viewmat, np.float32).astype(np.float64)
        Rw, t = vm[:3, :3], vm[:3, 3]
        fx, fy, cx, cy = (float(np.float32(K[0][0])), float(np.float32(K[1][1])), float(np.float32(K[0][2])),
                          float(np.float32(K[1][2])))
        q = np.where(keep[:, None], q, [1.0, 0.0, 0.0, 0.0])
        qn = np.where(keep, qn, 1.0)
        s = np.where(keep[:, None], s, 0.0)
        m = np.where(keep[:, None], m, 0.0)
        n = q / qn[:, None]
        Rq = ref.quat_to_rot(q)
        V = Rw[None] @ (Rq * s[:, None, :])
        S = V @ V.transpose(0, 2, 1)
        p = m @ Rw.T + t
        z = np.where(keep, p[:, 2], 1.0)
        limxp, limxn = (W - cx) / fx + 0.3 * (0.5 * W) / fx, cx / fx + 0.3 * (0.5 * W) / fx
        limyp, limyn = (H - cy) / fy + 0.3 * (0.5 * H) / fy, cy / fy + 0.3 * (0.5 * H) / fy
        ux, uy = p[:, 0] / z, p[:, 1] / z
        cux, cuy = np.clip(ux, -limxn, limxp), np.clip(uy, -limyn, limyp)
        J = np.zeros((N, 2, 3))
        J[:, 0, 0], J[:, 0, 2] = fx / z, -fx * (z * cux) / (z * z)
        J[:, 1, 1], J[:, 1, 2] = fy / z, -fy * (z * cuy) / (z * z)
        JS = J @ S
        S2 = JS @ J.transpose(0, 2, 1)
        s00, s01, s11 = S2[:, 0, 0] + eps2d, S2[:, 0, 1], S2[:, 1, 1] + eps2d
        det = s00 * s11 - s01 * s01
        mean2d = np.stack([fx * ux + cx, fy * uy + cy], 1)
        keep = keep & (det > 0) & np.isfinite(mean2d).all(1)
        conic = np.stack([s11 / det, -s01 / det, s00 / det], 1)
    zero = lambda a: np.where(keep.reshape((-1,) + (1,) * (a.ndim - 1)), a, 0.0)  # noqa: E731
    return dict(keep=keep, z32=z32, mean2d=zero(mean2d), conic=zero(conic), Rw=Rw, Rq=Rq, n=n, qn=qn, s=s, V=V, S=S, J=J, JS=JS,
                z=z, ux=ux, uy=uy, cux=cux, cuy=cuy, inx=(ux > -limxn) & (ux < limxp), iny=(uy > -limyn) & (uy < limyp),
                fx=fx, fy=fy)


def chain(P, g5):
    """The adjoint of project64: g5 [N,5] (dL/d mean2d x, y, dL/d conic A, B, C) -> (grad_means [N,3], grad_quats [N,4],
    grad_scales [N,3]); rows of culled Gaussians are 0."""
    g5 = np.asarray(g5, np.float64)
    A, B, C = P["conic"].T
    X = np.stack([np.stack([A, B], -1), np.stack([B, C], -1)], 1)
    GX = np.stack([np.stack([g5[:, 2], 0.5 * g5[:, 3]], -1), np.stack([0.5 * g5[:, 3], g5[:, 4]], -1)], 1)
    GZ = -X @ GX @ X                                       # dL/d Sigma2
    J, JS, Rw, Rq, s, n = P["J"], P["JS"], P["Rw"], P["Rq"], P["s"], P["n"]
    GJ = 2.0 * GZ @ JS
    GS = J.transpose(0, 2, 1) @ GZ @ J
    U = Rw[None] @ Rq
    Hl = U.transpose(0, 2, 1) @ GS @ U                      # dL/dSigma in the Gaussian's own frame, where Sigma = diag(s^2)
    Hl = 0.5 * (Hl + Hl.transpose(0, 2, 1))
    gs = 2.0 * s * np.stack([Hl[:, 0, 0], Hl[:, 1, 1], Hl[:, 2, 2]], 1)
    d2 = lambda i, j: (s[:, i] - s[:, j]) * (s[:, i] + s[:, j])  # noqa: E731
    # a rotation R -> R exp([d]x): exactly 0 between equal scales
    gd = 2.0 * np.stack([Hl[:, 1, 2] * d2(1, 2), Hl[:, 0, 2] * d2(2, 0), Hl[:, 0, 1] * d2(0, 1)], 1)
    w, x, y, z = n.T
    # n -> n (1, d/2): the gradient in the quaternion's tangent space, then the 1 / |q| of the normalisation
    gq = 2.0 * np.stack([-x * gd[:, 0] - y * gd[:, 1] - z * gd[:, 2], w * gd[:, 0] - z * gd[:, 1] + y * gd[:, 2],
                         z * gd[:, 0] + w * gd[:, 1] - x * gd[:, 2], -y * gd[:, 0] + x * gd[:, 1] + w * gd[:, 2]], 1) \
        / P["qn"][:, None]
    fx, fy, zz, ux, uy, cux, cuy = P["fx"], P["fy"], P["z"], P["ux"], P["uy"], P["cux"], P["cuy"]
    g_ux = g5[:, 0] * fx + np.where(P["inx"], -GJ[:, 0, 2] * fx / zz, 0.0)
    g_uy = g5[:, 1] * fy + np.where(P["iny"], -GJ[:, 1, 2] * fy / zz, 0.0)
    g_z = (-GJ[:, 0, 0] * fx + GJ[:, 0, 2] * fx * cux - GJ[:, 1, 1] * fy + GJ[:, 1, 2] * fy * cuy) / (zz * zz) \
        - (g_ux * ux + g_uy * uy) / zz
    gm = np.stack([g_ux / zz, g_uy / zz, g_z], 1) @ Rw
    k = P["keep"][:, None]
    return np.where(k, gm, 0.0), np.where(k, gq, 0.0), np.where(k, gs, 0.0)


def chain_jacobian(P):
    """jac [N,5,10]: row k is the chain of the k-th unit screen gradient, (means, quats, scales) side by side."""
    N = len(P["keep"])
    jac = np.zeros((N, 5, THETA))
    for k in range(5):
        e = np.zeros((N, 5))
        e[:, k] = 1.0
        jac[:, k] = np.concatenate(chain(P, e), 1)
    return jac


def _records(means, quats, scales, opacities, viewmat, K, W, H, near, far, eps2d, round_records):
    P = project64(means, quats, scales, opacities, viewmat, K, W, H, near, far, eps2d)
    m2, con = P["mean2d"], P["conic"]
    if round_records:
        m2, con = m2.astype(np.float32).astype(np.float64), con.astype(np.float32).astype(np.float64)
    idx = np.nonzero(P["keep"])[0]
    order = idx[np.lexsort((idx, P["z32"][idx]))]
    return P, m2, con, order


def _sweep(m2, con, op, order, W, H, fragile_rel):
    """Yields (g, add, a, e, raw, T before g, fragile pixels of this step, dx, dy) in blend order."""
    jj, ii = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    near_ = lambda v, thr: np.abs(v - thr) <= fragile_rel * abs(thr)  # noqa: E731
    T = np.ones((H, W))
    live = np.ones((H, W), bool)
    for g in order:
        if not live.any():
            break
        dx, dy = m2[g, 0] - jj, m2[g, 1] - ii
        A, B, C = con[g]
        sig = 0.5 * (A * dx * dx + C * dy * dy) + B * dx * dy
        e = np.exp(-sig)
        raw = op[g] * e
        a = np.minimum(ref.ALPHA_MAX, raw)
        tn = T * (1.0 - a)
        frag = live & (near_(raw, ref.ALPHA_MAX) | near_(a, ref.ALPHA_MIN) | (np.abs(sig) <= fragile_rel) |
                       ((sig >= 0) & (a >= ref.ALPHA_MIN) & near_(tn, ref.T_MIN)))
        use = live & (sig >= 0) & (a >= ref.ALPHA_MIN)
        stop = use & (tn <= ref.T_MIN)
        add = use & ~stop
        yield g, add, a, e, raw, T, frag, dx, dy
        T = np.where(add, tn, T)
        live &= ~stop


def forward64(means, quats, scales, opacities, features, viewmat, K, W, H, G, G_alpha, near=0.01, far=1e10, eps2d=0.3,
              round_records=False):
    """(loss, pairs): loss = sum G * logits + sum G_alpha * alpha of the float64 forward, pairs bool [N,H,W] = the (Gaussian,
    pixel) pairs it added.  The finite-difference target (records not rounded unless asked)."""
    f = np.asarray(features, np.float64)
    op = np.asarray(opacities, np.float64)
    _, m2, con, order = _records(means, quats, scales, opacities, viewmat, K, W, H, near, far, eps2d, round_records)
    out = np.zeros((f.shape[1], H, W))
    T_final = np.ones((H, W))
    pairs = np.zeros((len(f), H, W), bool)
    for g, add, a, e, raw, T, frag, dx, dy in _sweep(m2, con, op, order, W, H, 0.0):
        out += f[g][:, None, None] * np.where(add, a * T, 0.0)[None]
        T_final = np.where(add, T * (1.0 - a), T_final)
        pairs[g] = add
    loss = (np.asarray(G, np.float64) * out).sum() + (np.asarray(G_alpha, np.float64) * (1.0 - T_final)).sum()
    return float(loss), pairs


def splat_geom64(means, quats, scales, opacities, features, viewmat, K, W, H, G=None, G_alpha=None, near=0.01, far=1e10,
                 eps2d=0.3, fragile_rel=ref.FRAGILE_REL, round_records=True):
    """dict(grad_f [N,D], grad_o [N], grad_screen [N,5], grad_means [N,3], grad_quats [N,4], grad_scales [N,3], their
    magnitude scales M_f, M_o, M_screen, M_means, M_quats, M_scales, jac [N,5,10], fragile bool [H,W], visits int [H,W],
    added int [N], clamped bool [N] (on a clamped Jacobian branch))."""
    f = np.asarray(features, np.float64)
    N, D = f.shape
    G = np.zeros((D, H, W)) if G is None else np.asarray(G, np.float64)
    Ga = np.zeros((H, W)) if G_alpha is None else np.asarray(G_alpha, np.float64)
    op = np.asarray(opacities, np.float64)
    P, m2, con, order = _records(means, quats, scales, opacities, viewmat, K, W, H, near, far, eps2d, round_records)
    sweep = lambda: _sweep(m2, con, op, order, W, H, fragile_rel)  # noqa: E731
    CG = np.zeros((H, W))
    CGabs = np.zeros((H, W))
    T_final = np.ones((H, W))
    fragile = np.zeros((H, W), bool)
    visits = np.zeros((H, W), np.int64)
    absG = np.abs(G)
    for g, add, a, e, raw, T, frag, dx, dy in sweep():
        fragile |= frag
        w = np.where(add, a * T, 0.0)
        CG += w * np.tensordot(f[g], G, 1)
        CGabs += w * np.tensordot(np.abs(f[g]), absG, 1)
        T_final = np.where(add, T * (1.0 - a), T_final)
        visits += add
    grad_f, M_f = np.zeros((N, D)), np.zeros((N, D))
    grad_o, M_o = np.zeros(N), np.zeros(N)
    grad_s, M_s = np.zeros((N, 5)), np.zeros((N, 5))
    added = np.zeros(N, np.int64)
    Pfx = np.zeros((H, W))
    for g, add, a, e, raw, T, frag, dx, dy in sweep():
        if not add.any():
            continue
        w = np.where(add, a * T, 0.0)
        fG = np.tensordot(f[g], G, 1)
        fGabs = np.tensordot(np.abs(f[g]), absG, 1)
        Pfx += w * fG
        inv = 1.0 / (1.0 - a)
        dLda = T * fG - (CG - Pfx) * inv + Ga * T_final * inv
        dLda_abs = T * fGabs + CGabs * inv + np.abs(Ga) * T_final * inv
        live = add & (raw < ref.ALPHA_MAX)
        dado = np.where(live, e, 0.0)
        grad_f[g] = (G * w[None]).sum(axis=(1, 2))
        M_f[g] = (absG * w[None]).sum(axis=(1, 2))
        grad_o[g] = (dLda * dado).sum()
        M_o[g] = (dado * dLda_abs).sum()
        A, B, C = con[g]
        q = np.where(live, dLda * raw, 0.0)
        qa = np.where(live, dLda_abs * raw, 0.0)
        grad_s[g] = [-(q * (A * dx + B * dy)).sum(), -(q * (B * dx + C * dy)).sum(), -(q * 0.5 * dx * dx).sum(),
                     -(q * dx * dy).sum(), -(q * 0.5 * dy * dy).sum()]
        M_s[g] = [(qa * (np.abs(A * dx) + np.abs(B * dy))).sum(), (qa * (np.abs(B * dx) + np.abs(C * dy))).sum(),
                  (qa * 0.5 * dx * dx).sum(), (qa * np.abs(dx * dy)).sum(), (qa * 0.5 * dy * dy).sum()]
        added[g] = add.sum()
    jac = chain_jacobian(P)
    theta = np.einsum("nk,nkt->nt", grad_s, jac)
    M_theta = np.einsum("nk,nkt->nt", M_s, np.abs(jac))
    return dict(grad_f=grad_f, grad_o=grad_o, grad_screen=grad_s, grad_means=theta[:, :3], grad_quats=theta[:, 3:7],
                grad_scales=theta[:, 7:], M_f=M_f, M_o=M_o, M_screen=M_s, M_means=M_theta[:, :3], M_quats=M_theta[:, 3:7],
                M_scales=M_theta[:, 7:], jac=jac, fragile=fragile, visits=visits, added=added,
                clamped=P["keep"] & ~(P["inx"] & P["iny"]))


def theta_bound(jac, screen_bound, grad64):
    """The bound the GPU tests hold grad_means / grad_quats / grad_scales to, [N,10]: the chain is float64, so the error is
    the screen sums' error carried through the chain's Jacobian plus one fp32 rounding of the result,
    sum_k |d s_k / d theta| bound(s_k) + 2^-23 |grad64|."""
    return np.einsum("nk,nkt->nt", screen_bound, np.abs(jac)) + 2.0 ** -23 * np.abs(grad64)
