"""The splatting backward's contract (include/voxproj.h, vp_splat_rasterize_backward) in float64 NumPy, shared by
test_splat_grad_cpu.py and test_gpu_splat_grad.py.  It keeps splat_reference.splat64's decisions: every Gaussian is tried
at every pixel in (fp32 z, index) order, skipped when sigma < 0 or a < 1/255, and a pixel stops before the Gaussian that
would take T to <= 1e-4.

For a loss L = sum G * logits + sum G_alpha * alpha it returns grad_f [N,D], grad_o [N] and per-entry magnitude scales
M_f, M_o: the same sums with every product replaced by its absolute value.  The kernel derives the behind-sum S_g . G from
the pixel's C . G minus a running prefix, so M_o carries |C . G| through sum_k w_k sum_c |f_kc G_c|.
"""
import numpy as np

import splat_reference as ref


def splat_grad64(means, quats, scales, opacities, features, viewmat, K, W, H, G=None, G_alpha=None, near=0.01, far=1e10,
                 eps2d=0.3, fragile_rel=ref.FRAGILE_REL):
    """dict(grad_f, grad_o, M_f, M_o, fragile bool [H,W] (a decision within a relative ``fragile_rel`` of its threshold),
    visits int [H,W], added int [N] (pixels that added each Gaussian)).  G: [D,H,W] or None (0); G_alpha: [H,W] or None."""
    f = np.asarray(features, np.float64)
    N, D = f.shape
    G = np.zeros((D, H, W)) if G is None else np.asarray(G, np.float64)
    Ga = np.zeros((H, W)) if G_alpha is None else np.asarray(G_alpha, np.float64)
    keep, z32, m2, con, _, _ = ref.project(means, quats, scales, opacities, viewmat, K, W, H, near, far, eps2d)
    op = np.asarray(opacities, np.float32).astype(np.float64)
    idx = np.nonzero(keep)[0]
    order = idx[np.lexsort((idx, z32[idx]))]
    jj, ii = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    near_ = lambda v, thr: np.abs(v - thr) <= fragile_rel * abs(thr)  # noqa: E731

    def sweep():
        """Yields (g, add, a, e, raw, T before g, fragile pixels of this step) in blend order."""
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
            yield g, add, a, e, raw, T, frag
            T = np.where(add, tn, T)
            live &= ~stop

    # pass 1: T_final, C . G and its magnitude sum_k w_k sum_c |f_kc G_c|
    CG = np.zeros((H, W))
    CGabs = np.zeros((H, W))
    T_final = np.ones((H, W))
    fragile = np.zeros((H, W), bool)
    visits = np.zeros((H, W), np.int64)
    absG = np.abs(G)
    for g, add, a, e, raw, T, frag in sweep():
        fragile |= frag
        w = np.where(add, a * T, 0.0)
        CG += w * np.tensordot(f[g], G, 1)
        CGabs += w * np.tensordot(np.abs(f[g]), absG, 1)
        T_final = np.where(add, T * (1.0 - a), T_final)
        visits += add
    # pass 2: the gradients
    grad_f = np.zeros((N, D))
    grad_o = np.zeros(N)
    M_f = np.zeros((N, D))
    M_o = np.zeros(N)
    added = np.zeros(N, np.int64)
    P = np.zeros((H, W))
    for g, add, a, e, raw, T, frag in sweep():
        if not add.any():
            continue
        w = np.where(add, a * T, 0.0)
        fG = np.tensordot(f[g], G, 1)
        fGabs = np.tensordot(np.abs(f[g]), absG, 1)
        P += w * fG
        inv = 1.0 / (1.0 - a)
        dLda = T * fG - (CG - P) * inv + Ga * T_final * inv
        dado = np.where(add & (raw < ref.ALPHA_MAX), e, 0.0)
        grad_f[g] = (G * w[None]).sum(axis=(1, 2))
        M_f[g] = (absG * w[None]).sum(axis=(1, 2))
        grad_o[g] = (dLda * dado).sum()
        M_o[g] = (dado * (T * fGabs + CGabs * inv + np.abs(Ga) * T_final * inv)).sum()
        added[g] = add.sum()
    return dict(grad_f=grad_f, grad_o=grad_o, M_f=M_f, M_o=M_o, fragile=fragile, visits=visits, added=added)


def loss64(means, quats, scales, opacities, features, viewmat, K, W, H, G, G_alpha, **kw):
    """sum G * logits + sum G_alpha * alpha of the float64 forward (the finite-difference target)."""
    o = ref.splat64(means, quats, scales, opacities, features, viewmat, K, W, H, **kw)
    return float((np.asarray(G, np.float64) * o["logits"]).sum() + (np.asarray(G_alpha, np.float64) * o["alpha"]).sum())


def grad_bound(M, Gs, rel=1e-4, abs_=1e-6):
    """The bound the GPU tests hold every gradient entry to: rel * M + abs_ * max|G| over the upstream gradients ``Gs``."""
    gmax = max((float(np.abs(np.asarray(x)).max()) for x in Gs if x is not None and np.asarray(x).size), default=0.0)
    return rel * np.asarray(M) + abs_ * gmax


def splat_grad64_at(means, quats, scales, opacities, features, viewmat, K, W, H, pixels, G, G_alpha=None, near=0.01, far=1e10,
                    eps2d=0.3, cond=True, rec=None):
    """splat_grad64 for a loss whose upstream gradients are nonzero only at the (row, col) ``pixels`` [P,2]: G [P,D] and
    G_alpha [P] (None: 0) are their values there.  Built on splat_reference.pixel64 (one pixel against every kept Gaussian,
    no tiles).  dict(grad_f [N,D], grad_o [N], grad_screen [N,5] (the five sums of splat_geom_reference: dL/d mean2d x, y,
    dL/d conic A, B, C), M_f, M_o, M_screen, X_f, X_o, X_screen, fragile bool [P], visits int [P], added int [N]).

    X_*: the conditioning terms of the bound, to be added to grad_bound(M_*, ...).  grad_f sums G w, and w is off by at most
    E relative (splat_reference's derivation): X_f = sum_p |G| w E.  Every term of dL/da e^-sigma and of dL/da o e^-sigma (A dx
    + B dy) is a product of factors a, 1 - a, 1 / (1 - a) and e^-sigma of the Gaussians the pixel added, each at most twice, so
    it is off by at most e^(2 S) - 1 relative, S = sum_k (d_k + y_k) over them: X_o and X_screen are M_o's and M_screen's
    sums with every pixel's term times that factor (coarse on purpose; 0 where the pixel's Gaussians are well conditioned)."""
    f = np.asarray(features, np.float64)
    N, D = f.shape
    rec = rec if rec is not None else ref.records(means, quats, scales, opacities, viewmat, K, W, H, near, far, eps2d)
    pixels = np.asarray(pixels, np.int64).reshape(-1, 2)
    P = len(pixels)
    G = np.asarray(G, np.float64).reshape(P, D)
    Ga = np.zeros(P) if G_alpha is None else np.asarray(G_alpha, np.float64).reshape(P)
    out = {k: np.zeros((N, D)) for k in ("grad_f", "M_f", "X_f")}
    out.update({k: np.zeros(N) for k in ("grad_o", "M_o", "X_o")})
    out.update({k: np.zeros((N, 5)) for k in ("grad_screen", "M_screen", "X_screen")})
    added = np.zeros(N, np.int64)
    fragile, visits = np.zeros(P, bool), np.zeros(P, np.int64)
    for p, (i, j) in enumerate(pixels):
        r = ref.pixel64(rec, int(i), int(j), cond)
        fragile[p], visits[p] = r["fragile"], len(r["sel"])
        g = rec["order"][r["sel"]]
        added[g] += 1
        if not len(g) or (not G[p].any() and Ga[p] == 0):
            continue
        a, T, w, e, raw, dx, dy = (r[k] for k in ("a", "T", "w", "e", "raw", "dx", "dy"))
        fG, fGabs = f[g] @ G[p], np.abs(f[g]) @ np.abs(G[p])
        CG, CGabs = float((w * fG).sum()), float((w * fGabs).sum())
        Pfx = np.cumsum(w * fG)
        inv = 1.0 / (1.0 - a)
        dLda = T * fG - (CG - Pfx) * inv + Ga[p] * r["T_final"] * inv
        dLda_abs = T * fGabs + CGabs * inv + abs(Ga[p]) * r["T_final"] * inv
        live = raw < ref.ALPHA_MAX
        X = np.expm1(min(2.0 * r["S"], 700.0))
        out["grad_f"][g] += w[:, None] * G[p][None]
        out["M_f"][g] += w[:, None] * np.abs(G[p])[None]
        out["X_f"][g] += (w * r["E"])[:, None] * np.abs(G[p])[None]
        dado = np.where(live, e, 0.0)
        out["grad_o"][g] += dLda * dado
        out["M_o"][g] += dLda_abs * dado
        out["X_o"][g] += dLda_abs * dado * X
        A, B, C = rec["A"][r["sel"]], rec["B"][r["sel"]], rec["C"][r["sel"]]
        q, qa = np.where(live, dLda * raw, 0.0), np.where(live, dLda_abs * raw, 0.0)
        s = np.stack([-q * (A * dx + B * dy), -q * (B * dx + C * dy), -q * 0.5 * dx * dx, -q * dx * dy, -q * 0.5 * dy * dy], 1)
        ms = np.stack([qa * (np.abs(A * dx) + np.abs(B * dy)), qa * (np.abs(B * dx) + np.abs(C * dy)), qa * 0.5 * dx * dx,
                       qa * np.abs(dx * dy), qa * 0.5 * dy * dy], 1)
        out["grad_screen"][g] += s
        out["M_screen"][g] += ms
        out["X_screen"][g] += ms * X
    out.update(fragile=fragile, visits=visits, added=added)
    return out
