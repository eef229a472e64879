"""The fused splatting cross-entropy's contract (include/voxproj.h, vp_splat_rasterize_loss / vp_splat_loss_backward) in
float64 NumPy, shared by test_splat_loss_cpu.py and test_gpu_splat_loss.py.  Built on splat_reference (the forward and its
fragile mask), splat_grad_reference (the sampled backward) and splat_geom_reference (the dense backward with geometry).

With C_p the D blended logits of pixel p, t_p its target (valid when 0 <= t_p < D, anything else ignored) and w_p its weight:
  l_p = logsumexp_c C_pc - C_p,t_p,   stats = (sum_p w_p l_p, sum_p w_p) over the valid pixels,
  loss = stats[0] for "sum" and stats[0] / stats[1] for "mean" (0 when sum w = 0),
  G[c,p] = s w_p (softmax_c(C_p) - [c = t_p]) on valid pixels, 0 elsewhere; s = grad_loss for "sum", grad_loss / sum w for
  "mean" (0 when sum w = 0).  From G on the gradients are splat_geom_reference.splat_geom64's.

The bounds the GPU tests hold the kernel to, derived here (u = 2^-24, the fp32 unit roundoff):

  Logits.  delta_C = splat_reference.value_bound(features): the bound test_gpu_splat.py holds every non-fragile logit to.

  Per-pixel loss.  l is 2-Lipschitz in max_c |dC_c| (logsumexp is 1-Lipschitz in the max norm, and so is C_t), which gives
  2 delta_C.  The fp32 evaluation l = (m + logf(sum_c expf(C_c - m))) - C_t adds, per step:
    x_c = C_c - m         one rounding, |x_c| u: e^x moves by |x| e^x u <= u / e per term relative to the sum (>= 1)
    expf                  1 ulp (2 u relative) per term
    the sum               D - 1 additions, gamma_(D-1) relative
      => the sum is off by at most (D + 2) u relative, its logarithm by (D + 2) u absolute
    logf                  1 ulp: 2 u |log sum| <= 2 u log D
    m + log sum           one rounding: u (|m| + log D)
    ... - C_t             one rounding: u |l|
  lse_rounding(C, l) = u (D + 2 + 3 log D + |m| + |l|).  (expf and logf at 1 ulp are the documented accuracy of the
  device library's single-precision functions; -fno-fast-math keeps the precise versions.)
  pixel_loss = w l adds one more rounding, u |w l|; a weight of exactly 0 gives exactly 0 whatever l is.

  loss_stats.  The float64 sums add nothing visible: stats[0] within the sum of the pixel bounds, stats[1] within
  2^-50 sum w of the float64 sum of the fp32 weights.

  Gradients.  The sweep that follows G is the existing backward: grad_bound(M, G) with M the reference's magnitude scale.
  G itself is computed from the kernel's C, off by delta_C: d softmax_c = p_c (dC_c - sum_k p_k dC_k), so |dp_c| <= 2 delta_C
  p_c for c != t and |dp_t| <= 2 delta_C p_t (1 - p_t): in both cases |dG_c| <= 2 delta_C |G_c| to first order.  Every
  gradient is linear in G and M is the same sum over |G|, so G's own error adds 2 delta_C M.  The fp32 roundings inside G
  (the softmax, the scale) are (D + 6) u relative and lie under grad_bound's 1e-4.
"""
import numpy as np

import splat_geom_reference as geom
import splat_grad_reference as gref
import splat_reference as ref

U32 = ref.U32


def upstream64(logits, target, weight=None, reduction="mean", grad_loss=1.0, channel_axis=0):
    """The loss of a logits image and its upstream gradient.  logits [D,...] (or [...,D] with channel_axis=-1), target and
    weight shaped like one channel.  dict(pixel_loss (w l, 0 where ignored), l (unweighted, 0 where ignored), stats (2,),
    loss, G (shaped as logits), valid, scale s)."""
    C = np.moveaxis(np.asarray(logits, np.float64), channel_axis, 0)
    D = C.shape[0]
    t = np.asarray(target, np.int64)
    valid = (t >= 0) & (t < D)
    w = np.where(valid, 1.0 if weight is None else np.asarray(weight, np.float64), 0.0)
    m = C.max(axis=0)
    e = np.exp(C - m[None])
    lse = m + np.log(e.sum(axis=0))
    tc = np.where(valid, t, 0)
    ct = np.take_along_axis(C, tc[None], 0)[0]
    l = np.where(valid, lse - ct, 0.0)
    with np.errstate(invalid="ignore"):
        wl = np.where(w != 0, w * l, 0.0)                       # weight 0 contributes nothing, whatever l is
    stats = np.array([wl.sum(), w.sum()])
    if reduction == "mean":
        loss = stats[0] / stats[1] if stats[1] > 0 else 0.0
        s = grad_loss / stats[1] if stats[1] > 0 else 0.0
    elif reduction == "sum":
        loss, s = stats[0], grad_loss
    else:
        raise ValueError(reduction)
    onehot = np.arange(D).reshape((D,) + (1,) * t.ndim) == tc[None]
    G = np.where(valid[None], s * w[None] * (e / e.sum(axis=0)[None] - onehot), 0.0)
    return dict(pixel_loss=wl, l=l, stats=stats, loss=float(loss), G=np.moveaxis(G, 0, channel_axis), valid=valid, scale=s,
                w=w)


def logits64(means, quats, scales, opacities, features, viewmat, K, W, H, near=0.01, far=1e10, eps2d=0.3,
             round_records=True):
    """The float64 forward's logits [D,H,W] on float64 geometry (splat_geom_reference's records and sweep).  With
    ``round_records`` they are splat_reference.splat64's; without, a smooth function of the geometry (the finite-difference
    target)."""
    f = np.asarray(features, np.float64)
    op = np.asarray(opacities, np.float64)
    _, m2, con, order = geom._records(means, quats, scales, opacities, viewmat, K, W, H, near, far, eps2d, round_records)
    out = np.zeros((f.shape[1], H, W))
    for g, add, a, e, raw, T, frag, dx, dy in geom._sweep(m2, con, op, order, W, H, 0.0):
        out += f[g][:, None, None] * np.where(add, a * T, 0.0)[None]
    return out


def loss64(means, quats, scales, opacities, features, viewmat, K, W, H, target, weight=None, reduction="mean", grad_loss=1.0,
           G_alpha=None, round_records=True, grads=True, **kw):
    """The contract end to end: upstream64's dict on the float64 forward's logits plus, with ``grads``, the analytic
    gradients and magnitude scales of splat_geom_reference.splat_geom64 driven with G (grad_f, grad_o, grad_screen,
    grad_means, grad_quats, grad_scales, M_*, jac, fragile, visits, added).  G_alpha adds sum G_alpha * alpha to what is
    differentiated (not to ``loss``)."""
    C = logits64(means, quats, scales, opacities, features, viewmat, K, W, H, round_records=round_records, **kw)
    out = upstream64(C, target, weight, reduction, grad_loss)
    out["logits"] = C
    if grads:
        out.update(geom.splat_geom64(means, quats, scales, opacities, features, viewmat, K, W, H, G=out["G"], G_alpha=G_alpha,
                                     round_records=round_records, **kw))
    return out


def lse_rounding(logits, l, channel_axis=0):
    """The fp32 rounding of one pixel's l (the derivation above)."""
    C = np.moveaxis(np.asarray(logits, np.float64), channel_axis, 0)
    D = C.shape[0]
    return U32 * (D + 2 + 3.0 * np.log(D) + np.abs(C).max(axis=0) + np.abs(l))


def pixel_loss_bound(o, delta_C):
    """Per pixel: w (2 delta_C + lse_rounding) + u |w l|; ``o``: upstream64's dict with its logits; delta_C scalar or per pixel."""
    return o["w"] * (2.0 * delta_C + lse_rounding(o["logits"], o["l"])) + U32 * np.abs(o["pixel_loss"])


def loss_grad_bound(M, Gs, delta_C):
    """grad_bound(M, Gs) + 2 delta_C M: the existing sweep's bound plus the first-order term of G's own error."""
    return gref.grad_bound(M, Gs) + 2.0 * delta_C * np.asarray(M)
