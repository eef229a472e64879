"""Differentiable Gaussian splatting: the splatting forward (vp_splat_project + vp_splat_rasterize) as a
``torch.autograd.Function``, with vp_splat_rasterize_backward as its backward.

Gradients flow from the logits [D,H,W] and alpha [H,W] to the per-Gaussian features [N,D] and the activated opacities [N],
through the branch the forward took (include/voxproj.h states the contract).  Labels and confidence are returned but not
differentiable.  ``splat_features`` keeps the geometry fixed: a call whose geometry requires grad raises instead of dropping
the gradient.  ``splat_gaussians`` is differentiable in the means, the quaternions and the activated scales as well, through
vp_splat_rasterize_backward_geometry (one fused tile sweep for every gradient asked for).  No gradient for the camera, no
double backward.  ``splat_cross_entropy`` is the fused softmax cross-entropy of the splatted logits against a per-pixel target
map (vp_splat_rasterize_loss / vp_splat_loss_backward): no logits or gradient image crosses torch.
``splat_wide_features`` renders rows of up to 4096 channels channels-last (vp_splat_render) and is differentiable in the rows
only, with the lift (vp_splat_lift) as its backward.  ``splat_feature_loss`` is the fused cosine / L2 loss of that render
against a 2D feature map (vp_feature_loss / vp_feature_loss_gradient): the gradient image is written in binary16 once, and no
fp32 gradient image or torch reduction over an image appears on the path.  ``splat_contrastive`` is the prototype-contrastive
loss of the splatted identity features against one view's instance mask (vp_proto_contrast / vp_proto_contrast_gradient
between the rasterizer and its backward): no torch pass over an image.  ``splat_photometric`` is the photometric loss, L1 +
D-SSIM, of the splatted colour rows against a photograph (vp_photo_loss / vp_photo_loss_gradient in the same place).
``sh_colors`` makes those colour rows view-dependent: spherical harmonics of degree 0 .. 3 evaluated per Gaussian for one
camera (vp_sh_colors), differentiable in the coefficients and, through the view direction, in the means
(vp_sh_colors_backward).

Each call keeps its own SplatWorkspace until its backward has run (the backward reads the forward's sorted intersections),
so calls from several threads or views share no state.  The workspace is freed after the backward, or with the graph.
"""
import math

import torch
from torch.autograd.function import once_differentiable

import voxproj_host as _host

__all__ = ["splat_features", "SplatFeatures", "splat_gaussians", "SplatGaussians", "splat_cross_entropy", "SplatCrossEntropy",
           "splat_wide_features", "SplatWideFeatures", "quantize_gradient_map", "splat_feature_loss", "SplatFeatureLoss",
           "splat_contrastive", "SplatContrastive", "splat_photometric", "SplatPhotometric", "sh_colors", "SHColors"]


def _require_f32(means, quats, scales, opacities, **more):
    """The four tensors every call takes, and what else is named, must be torch.float32 tensors on a GPU."""
    named = dict(means=means, quats=quats, scales=scales, opacities=opacities, **more)
    _host._require_tensors(*((t, name, (torch.float32,)) for name, t in named.items()))


def _refuse_grad(differentiable_in, **tensors):
    """Raise instead of dropping a gradient: none of ``tensors`` may require grad; the text says what the call is
    differentiable in, and what to do."""
    for name, t in tensors.items():
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise ValueError(f"{name} requires grad, but {differentiable_in}")


def _reduce(stats, reduction):
    """stats = (total, weight, ...) on the device: total / weight for "mean" (0 when the weight is 0), the total for "sum"."""
    total, weight = stats[0], stats[1]
    return torch.where(weight > 0, total / weight, torch.zeros_like(total)) if reduction == "mean" else total


def _take(ctx, *names):
    """What the forward left on ``ctx`` under ``names`` (workspaces, maps), handed to the backward: ``ctx`` lets go of it, so
    it is freed when the backward returns, not with the graph."""
    held = tuple(getattr(ctx, name) for name in names)
    for name in names:
        setattr(ctx, name, None)
    return held


def _rasterize_backward(saved, view, ws, grad_logits, grad_alpha, needs, want_screen=False):
    """The backward of one splatted view, asked only for what is needed.  ``saved`` = (means, quats, scales, features) of
    the forward, ``view`` = (viewmat, K, W, H, eps2d, capacity), ``ws`` the forward's workspace, ``needs`` =
    needs_input_grad of (means, quats, scales, opacities, features).  A geometry gradient or the screen-space sums take
    vp_splat_rasterize_backward_geometry (one fused tile sweep), features and opacities alone vp_splat_rasterize_backward
    (which reads only the features of ``saved`` and W, H, capacity of ``view``), nothing asked for launches nothing.
    Returns ((means, quats, scales, opacities, features) gradients, None where not asked for; screen sums [N,5] or None)."""
    m, q, s, f = saved
    viewmat, K, W, H, eps2d, cap = view
    want_m, want_q, want_s, want_o, want_f = needs
    gl = grad_logits.float() if grad_logits is not None else None
    ga = grad_alpha.float() if grad_alpha is not None else None
    g = dict(means=None, quats=None, scales=None, opacities=None, features=None, screen=None)
    if want_m or want_q or want_s or want_screen:
        g = _host.splat_rasterize_backward_geometry(m, q, s, f, viewmat, K, W, H, cap, ws, gl, ga, eps2d=eps2d,
                                                    want_means=want_m, want_quats=want_q, want_scales=want_s,
                                                    want_features=want_f, want_opacities=want_o, want_screen=want_screen)
    elif want_f or want_o:
        g["features"], g["opacities"] = _host.splat_rasterize_backward(f, int(f.shape[0]), W, H, cap, ws, grad_logits=gl,
                                                                       grad_alpha=ga, want_features=want_f,
                                                                       want_opacities=want_o)
    return (g["means"], g["quats"], g["scales"], g["opacities"], g["features"]), g["screen"]


class SplatFeatures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, opacities, means, quats, scales, viewmat, K, W, H, near, far, eps2d, check):
        ws = _host.SplatWorkspace()
        f = features.detach()
        r = _host.splat_features(means.detach(), quats.detach(), scales.detach(), opacities.detach(), f, viewmat, K, W, H,
                                 want_logits=True, want_alpha=True, want_confidence=True, near=near, far=far, eps2d=eps2d,
                                 workspace=ws, check=check)
        ctx.ws = ws
        ctx.shape = (int(W), int(H), int(r.n_isect))
        ctx.save_for_backward(f)
        ctx.mark_non_differentiable(r.labels, r.confidence)
        return r.logits, r.alpha, r.labels, r.confidence

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_logits, grad_alpha, _grad_labels, _grad_confidence):
        f, = ctx.saved_tensors
        ws, = _take(ctx, "ws")
        W, H, cap = ctx.shape
        want_f, want_o = ctx.needs_input_grad[:2]
        (_, _, _, go, gf), _ = _rasterize_backward((None, None, None, f), (None, None, W, H, None, cap), ws, grad_logits,
                                                   grad_alpha, (False, False, False, want_o, want_f))
        return (gf, go) + (None,) * 11


def splat_features(means, quats, scales, opacities, features, viewmat, K, W, H, *, near=0.01, far=1e10, eps2d=0.3,
                   check=True):
    """Differentiable splatting of D-channel per-Gaussian features into one W x H view.

      means f32 [N,3], quats f32 [N,4], scales f32 [N,3]   the geometry, on the GPU; must not require grad
      opacities f32 [N] (activated), features f32 [N,D]   D <= 64, on the same GPU; either may require grad
      viewmat [4,4] world-to-camera, K [3,3]               any device, read on the host

    Returns (logits f32 [D,H,W], alpha f32 [H,W], labels int32 [H,W], confidence f32 [H,W]); only logits and alpha are
    differentiable.  The images are bit-identical to voxproj_host.splat_features(..., want_logits=True, want_alpha=True).
    ``check``: raise when a Gaussian has a non-finite parameter (it is culled either way).
    For gradients of the means, quats and scales use ``splat_gaussians``."""
    _refuse_grad("geometry gradients are not implemented: only the features and the opacities are differentiable (detach "
                 "the geometry)", means=means, quats=quats, scales=scales)
    _require_f32(means, quats, scales, opacities, features=features)
    return SplatFeatures.apply(features, opacities, means, quats, scales, viewmat, K, int(W), int(H), float(near), float(far),
                               float(eps2d), bool(check))


class SplatGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, quats, scales, opacities, features, viewmat, K, W, H, near, far, eps2d, check):
        ws = _host.SplatWorkspace()
        m, q, s, f = means.detach(), quats.detach(), scales.detach(), features.detach()
        r = _host.splat_features(m, q, s, opacities.detach(), f, viewmat, K, W, H, want_logits=True, want_alpha=True,
                                 want_confidence=True, near=near, far=far, eps2d=eps2d, workspace=ws, check=check)
        ctx.ws = ws
        ctx.view = (viewmat, K, int(W), int(H), float(eps2d), int(r.n_isect))
        ctx.save_for_backward(m, q, s, f)
        ctx.mark_non_differentiable(r.labels, r.confidence)
        return r.logits, r.alpha, r.labels, r.confidence

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_logits, grad_alpha, _grad_labels, _grad_confidence):
        ws, = _take(ctx, "ws")
        grads, _ = _rasterize_backward(ctx.saved_tensors, ctx.view, ws, grad_logits, grad_alpha, ctx.needs_input_grad[:5])
        return grads + (None,) * 8


def splat_gaussians(means, quats, scales, opacities, features, viewmat, K, W, H, *, near=0.01, far=1e10, eps2d=0.3,
                    check=True):
    """Splatting of D-channel per-Gaussian features into one W x H view, differentiable in every Gaussian parameter.

      means f32 [N,3], quats f32 [N,4] (w, x, y, z; any norm), scales f32 [N,3] (activated),
      opacities f32 [N] (activated), features f32 [N,D]     D <= 64, all on one GPU; any of the five may require grad
      viewmat [4,4] world-to-camera, K [3,3]                 any device, read on the host; no gradient

    Returns (logits f32 [D,H,W], alpha f32 [H,W], labels int32 [H,W], confidence f32 [H,W]), bit-identical to
    ``splat_features``'s; only logits and alpha are differentiable.  The gradient of the quaternions is with respect to the
    tensor as passed (orthogonal to it), the scales' and the opacities' with respect to the activated values.  The backward
    runs the fused vp_splat_rasterize_backward_geometry once and asks only for what requires grad; without a geometry
    gradient it is ``splat_features``'s backward.  ``check``: raise when a Gaussian has a non-finite parameter."""
    _require_f32(means, quats, scales, opacities, features=features)
    return SplatGaussians.apply(means, quats, scales, opacities, features, viewmat, K, int(W), int(H), float(near), float(far),
                                float(eps2d), bool(check))


class SplatCrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, quats, scales, opacities, features, viewmat, K, W, H, target, pixel_weight, reduction,
                keep_logits, near, far, eps2d, check):
        ws = _host.SplatWorkspace()
        m, q, s, f = means.detach(), quats.detach(), scales.detach(), features.detach()
        r = _host.splat_loss(m, q, s, opacities.detach(), f, viewmat, K, W, H, target, pixel_weight, want_alpha=True,
                             want_logits=keep_logits, near=near, far=far, eps2d=eps2d, workspace=ws, check=check)
        loss = _reduce(r.loss_stats, reduction)
        ctx.ws = ws
        ctx.view = (viewmat, K, int(W), int(H), float(eps2d), int(r.n_isect), reduction)
        ctx.maps = (target, pixel_weight, r.loss_stats, r.logits)
        ctx.save_for_backward(m, q, s, f)
        ctx.mark_non_differentiable(r.labels, r.confidence, r.alpha)
        return loss.float(), r.labels, r.confidence, r.alpha

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _grad_labels, _grad_confidence, _grad_alpha):
        m, q, s, f = ctx.saved_tensors
        ws, (target, weight, stats, logits) = _take(ctx, "ws", "maps")
        viewmat, K, W, H, eps2d, cap, reduction = ctx.view
        want_m, want_q, want_s, want_o, want_f = ctx.needs_input_grad[:5]
        g = dict(means=None, quats=None, scales=None, opacities=None, features=None)
        if want_m or want_q or want_s or want_o or want_f:
            # the scale stays on the device: the kernel reads it
            g = _host.splat_loss_backward(m, q, s, f, viewmat, K, W, H, cap, ws, target, weight, stats, logits=logits,
                                          reduction=reduction, grad_loss=grad_loss.float().reshape(1).contiguous(),
                                          eps2d=eps2d, want_means=want_m, want_quats=want_q, want_scales=want_s,
                                          want_features=want_f, want_opacities=want_o)
        return (g["means"], g["quats"], g["scales"], g["opacities"], g["features"]) + (None,) * 12


# True: the saved arm, the faster one at 1 M Gaussians, D = 32, 1600x1067 (7.15 ms a step against the replay arm's 8.64 ms,
# profiles/r12_splat_loss.jsonl); False trades that for memory: no [D,H,W] image is allocated
KEEP_LOGITS_DEFAULT = True


def splat_cross_entropy(means, quats, scales, opacities, features, viewmat, K, W, H, target, pixel_weight=None, *,
                        reduction="mean", keep_logits=KEEP_LOGITS_DEFAULT, near=0.01, far=1e10, eps2d=0.3, check=True):
    """Softmax cross-entropy of the splatted features (the per-Gaussian logits) of one W x H view against a target map,
    fused into the splatting kernels (include/voxproj.h states the contract).

      means, quats, scales, opacities, features, viewmat, K   as ``splat_gaussians``; any of the five tensors may require grad
      target int32 [H,W] on the GPU                           the class of every pixel; a value outside [0, D) ignores the pixel
      pixel_weight f32 [H,W] or None                          per-pixel weights (None: 1)
      reduction "mean" (sum w l / sum w; 0 when sum w = 0) or "sum"
      keep_logits   True: the forward writes the [D,H,W] logits and the backward reads them back; False: the backward blends
                    each pixel again and nothing of that size is allocated.  The gradients are the same bits either way.

    Returns (loss f32 0-dim, labels int32 [H,W], confidence f32 [H,W], alpha f32 [H,W]); only the loss is differentiable,
    and the backward asks only for what requires grad.  The gradient flowing into the loss is read by the kernel on the
    device.  No double backward, no gradient for the camera."""
    _host._require(reduction in ("mean", "sum"), f"reduction must be 'mean' or 'sum', not {reduction!r}")
    _require_f32(means, quats, scales, opacities, features=features)
    return SplatCrossEntropy.apply(means, quats, scales, opacities, features, viewmat, K, int(W), int(H), target, pixel_weight,
                                   reduction, bool(keep_logits), float(near), float(far), float(eps2d), bool(check))


def quantize_gradient_map(G):
    """The rule that brings an fp32 gradient map to the binary16 map the lift reads: with m = max |G|,
    s = 2^(14 - ceil(log2 m)) and Gq = f16(G s), so the largest element lands in (2^13, 2^14] whatever the loss's scale and
    the small gradients of a mean loss stay out of the binary16 subnormals; s is a power of two, so G s is exact in fp32 and
    the only rounding is the one to binary16.  The exponent is capped at 126 (m below 2^-112), and an all-zero map gives
    s = 1 and a zero Gq.  Returns (Gq f16, k int32 0-dim with s = 2^k), both on G's device; no host synchronisation."""
    _host._require(isinstance(G, torch.Tensor) and G.dtype == torch.float32, "the gradient map must be a torch.float32 tensor")
    m = G.abs().max() if G.numel() else G.new_zeros(())
    mant, ex = torch.frexp(m)                                # m = mant 2^ex with mant in [0.5, 1)
    ceil_log2 = torch.where(mant == 0.5, ex - 1, ex)
    k = torch.where(m > 0, (14 - ceil_log2).clamp(max=126), torch.zeros_like(ex)).to(torch.int32)
    return torch.ldexp(G, k).to(torch.float16), k


class SplatWideFeatures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rows, means, quats, scales, opacities, viewmat, K, W, H, dtype, near, far, eps2d, check):
        ws = _host.SplatWorkspace()
        out, alpha, cap, _ = _host.splat_render_view(means.detach(), quats.detach(), scales.detach(), opacities.detach(),
                                                     rows.detach(), viewmat, K, W, H, dtype=dtype, want_alpha=True, near=near,
                                                     far=far, eps2d=eps2d, workspace=ws, check=check)
        ctx.ws = ws
        ctx.shape = (int(W), int(H), int(cap), int(rows.shape[0]), int(rows.shape[1]), rows.dtype)
        ctx.mark_non_differentiable(alpha)
        return out, alpha

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _grad_alpha):
        ws, = _take(ctx, "ws")
        W, H, cap, N, C, dtype = ctx.shape
        if not ctx.needs_input_grad[0] or grad_out is None:
            return (None,) * 14
        Gq, k = quantize_gradient_map(grad_out.float())
        total = torch.zeros((N, C), dtype=torch.float32, device=grad_out.device)
        _host.splat_lift(Gq, N, W, H, cap, ws, total, None, sorted=True)
        return (torch.ldexp(total, -k).to(dtype),) + (None,) * 13


def splat_wide_features(means, quats, scales, opacities, rows, viewmat, K, W, H, *, dtype=torch.float32, near=0.01, far=1e10,
                        eps2d=0.3, check=True):
    """Differentiable rendering of wide per-Gaussian feature rows into one W x H view, channels-last (vp_splat_render).

      means f32 [N,3], quats f32 [N,4], scales f32 [N,3], opacities f32 [N]   on the GPU; must not require grad
      rows f16 or f32 [N,C], 1 <= C <= 4096, on the same GPU                  may require grad
      viewmat [4,4] world-to-camera, K [3,3]                                  any device, read on the host

    Returns (out ``dtype`` [H,W,C], alpha f32 [H,W]), bit-identical to voxproj_host.splat_render_view's.  Differentiable IN
    THE ROWS ONLY: alpha is not differentiable, and a call whose geometry or opacities require grad raises instead of
    dropping the gradient (use ``splat_gaussians`` for <= 64 channels).

    The backward is the lift (vp_splat_lift with sorted = 1 on the forward's workspace), which reads a binary16 map: the
    upstream gradient G [H,W,C] is brought to binary16 by ``quantize_gradient_map`` (s = 2^(14 - ceil(log2 max|G|)),
    Gq = f16(G s)) and the lifted sums are divided by s.  The gradient returned is therefore the exact adjoint of the forward
    applied to Gq / s (every element of G rounded to 11 bits relative to the map's largest, not to its own magnitude), within
    the lift's stated accuracy.  An all-zero G gives zero gradients.  No double backward."""
    _refuse_grad("splat_wide_features is differentiable in the rows only (detach it)", means=means, quats=quats, scales=scales,
                 opacities=opacities)
    _require_f32(means, quats, scales, opacities)
    _host._require_tensors((rows, "rows", (torch.float16, torch.float32)))
    return SplatWideFeatures.apply(rows, means, quats, scales, opacities, viewmat, K, int(W), int(H), dtype, float(near),
                                   float(far), float(eps2d), bool(check))


class SplatFeatureLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rows, means, quats, scales, opacities, viewmat, K, W, H, target, pixel_weight, kind, reduction, min_alpha,
                dtype, near, far, eps2d, check):
        ws = _host.SplatWorkspace()
        image, alpha, cap, _ = _host.splat_render_view(means.detach(), quats.detach(), scales.detach(), opacities.detach(),
                                                       rows.detach(), viewmat, K, W, H, dtype=dtype, want_alpha=True, near=near,
                                                       far=far, eps2d=eps2d, workspace=ws, check=check)
        stats, _, lws = _host.feature_loss(image, target, pixel_weight, alpha, kind=kind, min_alpha=min_alpha)
        loss = _reduce(stats, reduction)
        ctx.ws, ctx.lws = ws, lws
        ctx.maps = (image, target, stats)
        ctx.shape = (int(W), int(H), int(cap), int(rows.shape[0]), int(rows.shape[1]), rows.dtype, reduction)
        ctx.mark_non_differentiable(alpha)
        return loss.float(), alpha

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _grad_alpha):
        ws, lws, (image, target, stats) = _take(ctx, "ws", "lws", "maps")
        W, H, cap, N, C, dtype, reduction = ctx.shape
        if not ctx.needs_input_grad[0] or grad_loss is None:
            return (None,) * 19
        # the scale stays on the device: the kernel reads it, and writes the exponent the lifted sums are divided by
        Gq, k = _host.feature_loss_gradient(image, target, stats, lws, reduction=reduction,
                                            grad_loss=grad_loss.float().reshape(1).contiguous())
        total = torch.zeros((N, C), dtype=torch.float32, device=Gq.device)
        _host.splat_lift(Gq, N, W, H, cap, ws, total, None, sorted=True)
        return (torch.ldexp(total, -k).to(dtype),) + (None,) * 18


def splat_feature_loss(means, quats, scales, opacities, rows, viewmat, K, W, H, target, pixel_weight=None, *, kind="cosine",
                       reduction="mean", min_alpha=0.0, dtype=torch.float16, near=0.01, far=1e10, eps2d=0.3, check=True):
    """The cosine or L2 loss between the wide rows rendered into one W x H view and a 2D feature map, fused
    (include/voxproj.h states the contract of vp_feature_loss and vp_feature_loss_gradient).

      means, quats, scales, opacities, rows, viewmat, K   as ``splat_wide_features``: differentiable IN THE ROWS ONLY
      target f16 [H,W,C] on the GPU, channels-last         the view's feature map (upsample_features(keep_dtype=True))
      pixel_weight f32 [H,W] or None                       per-pixel weights (None: 1; not > 0 excludes the pixel)
      kind "cosine" (1 - cos per pixel) or "l2" (mean squared difference per pixel)
      reduction "mean" (sum m l / sum m; 0 when sum m = 0) or "sum"
      min_alpha   pixels whose rendered alpha is below it are excluded: a near-empty pixel has a tiny rendered row, and its
                  cosine gradient, proportional to 1 / |row|, would set the one exponent the binary16 gradient map has
      dtype       of the rendered image the loss reads: torch.float16 (half the traffic) or torch.float32

    Returns (loss f32 0-dim, alpha f32 [H,W]); only the loss is differentiable.  Forward: vp_splat_render into a ``dtype``
    image, then vp_feature_loss.  Backward: vp_feature_loss_gradient (the upstream scalar is read on the device) writes the
    binary16 gradient map and its exponent k, vp_splat_lift (sorted = 1, on the forward's workspace) lifts it, and the sums
    are divided by 2^k.  No double backward."""
    _host._require(kind in _host.FEATURE_LOSS_KINDS, f"kind must be 'cosine' or 'l2', not {kind!r}")
    _host._require(reduction in ("mean", "sum"), f"reduction must be 'mean' or 'sum', not {reduction!r}")
    _host._require(dtype in (torch.float16, torch.float32), "dtype must be torch.float16 or torch.float32")
    _refuse_grad("splat_feature_loss is differentiable in the rows only (detach it)", means=means, quats=quats, scales=scales,
                 opacities=opacities)
    _require_f32(means, quats, scales, opacities)
    _host._require_tensors((rows, "rows", (torch.float16, torch.float32)), (target, "target", (torch.float16,)))
    return SplatFeatureLoss.apply(rows, means, quats, scales, opacities, viewmat, K, int(W), int(H), target, pixel_weight, kind,
                                  reduction, float(min_alpha), dtype, float(near), float(far), float(eps2d), bool(check))


class SplatContrastive(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, quats, scales, opacities, features, viewmat, K, W, H, ids, count, weights, proto, near, far, eps2d,
                check):
        ws = _host.SplatWorkspace()
        m, q, s, f = means.detach(), quats.detach(), scales.detach(), features.detach()
        r = _host.splat_features(m, q, s, opacities.detach(), f, viewmat, K, W, H, want_logits=True, want_alpha=False,
                                 want_confidence=False, near=near, far=far, eps2d=eps2d, workspace=ws, check=check)
        stats, _, _, lws = _host.proto_contrast(r.logits, ids, count, **proto)
        # four numbers, on the device: weight_contrast (sum m l) / K (0 when K = 0) + weight_norm (sum (r - 1)^2) / (W H)
        contrast = torch.where(stats[1] > 0, stats[0] / stats[1].clamp(min=1.0), torch.zeros_like(stats[0]))
        loss = weights[0] * contrast + weights[1] * stats[2] / float(int(W) * int(H))
        ctx.ws, ctx.lws = ws, lws
        ctx.view = (viewmat, K, int(W), int(H), float(eps2d), int(r.n_isect))
        ctx.weights = weights
        ctx.maps = (r.logits, ids, count)
        ctx.save_for_backward(m, q, s, f)
        ctx.mark_non_differentiable(stats)
        return loss.float(), stats

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _grad_stats):
        ws, lws, (image, ids, count) = _take(ctx, "ws", "lws", "maps")
        needs = ctx.needs_input_grad[:5]
        if not any(needs):
            return (None,) * 17
        # the scale stays on the device: the kernel reads it
        G = _host.proto_contrast_gradient(image, ids, count, lws, weight_contrast=ctx.weights[0], weight_norm=ctx.weights[1],
                                          grad_loss=grad_loss.float().reshape(1).contiguous())
        grads, _ = _rasterize_backward(ctx.saved_tensors, ctx.view, ws, G, None, needs)
        return grads + (None,) * 12


def splat_contrastive(means, quats, scales, opacities, features, viewmat, K, W, H, ids, count=None, *, weight_contrast=1.0,
                      weight_norm=1.0, min_count=20, ignore_id=-1, phi_scale=10.0, phi_min=0.5, phi_max=1.0, near=0.01, far=1e10,
                      eps2d=0.3, check=True):
    """The prototype-contrastive loss of the splatted identity features of one W x H view against the view's instance mask,
    whose ids mean nothing in any other view (include/voxproj.h states the contract of vp_proto_contrast).

      means, quats, scales, opacities, features, viewmat, K   as ``splat_gaussians``; any of the five tensors may require grad
      ids int32 [H,W] on the GPU      the mask; ids outside [0, 256) and ``ignore_id`` are left out
      count int32 [H,W] or None       how many times each pixel was drawn (torch.bincount of a draw with replacement); None: once
      min_count, phi_*                an id takes part with more than min_count drawn pixels; its temperature is
                                      clip(phi_scale spread, phi_min, phi_max)

    Returns (loss f32 0-dim = weight_contrast (sum m l) / K + weight_norm mean (|f| - 1)^2, stats f64 [4] = {sum m l, K,
    sum (|f| - 1)^2, sum m}, detached).  Forward: vp_splat_project, vp_splat_rasterize (the image is kept), vp_proto_contrast.
    Backward: vp_proto_contrast_gradient writes the gradient image (the upstream scalar is read on the device), then
    vp_splat_rasterize_backward_geometry, or vp_splat_rasterize_backward when no geometry gradient is asked for.  No torch
    pass over an image, no double backward, no gradient for the camera."""
    _require_f32(means, quats, scales, opacities, features=features)
    weights = (float(weight_contrast), float(weight_norm))
    proto = dict(ignore_id=int(ignore_id), min_count=int(min_count), phi_scale=float(phi_scale), phi_min=float(phi_min),
                 phi_max=float(phi_max))
    return SplatContrastive.apply(means, quats, scales, opacities, features, viewmat, K, int(W), int(H), ids, count, weights,
                                  proto, float(near), float(far), float(eps2d), bool(check))


class SplatPhotometric(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, quats, scales, opacities, colors, viewmat, K, W, H, target, lambda_dssim, near, far, eps2d, check,
                densify_stats, stats_scale):
        ws = _host.SplatWorkspace()
        m, q, s, f = means.detach(), quats.detach(), scales.detach(), colors.detach()
        r = _host.splat_features(m, q, s, opacities.detach(), f, viewmat, K, W, H, want_logits=True, want_alpha=False,
                                 want_confidence=False, near=near, far=far, eps2d=eps2d, workspace=ws, check=check)
        ctx.densify = (densify_stats, float(stats_scale))
        stats, _, lws = _host.photo_loss(r.logits, target)
        # three numbers, on the device: (1 - lambda) sum |x - y| / n + lambda (1 - sum m / n)
        n = float(r.logits.numel())
        loss = (1.0 - lambda_dssim) * stats[0] / n + lambda_dssim * (1.0 - stats[2] / n)
        ctx.ws, ctx.lws = ws, lws
        ctx.view = (viewmat, K, int(W), int(H), float(eps2d), int(r.n_isect))
        ctx.lambda_dssim = lambda_dssim
        ctx.maps = (r.logits, target)
        ctx.save_for_backward(m, q, s, f)
        ctx.mark_non_differentiable(stats)
        return loss.float(), stats

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _grad_stats):
        ws, lws, (image, target) = _take(ctx, "ws", "lws", "maps")
        needs = ctx.needs_input_grad[:5]
        if not any(needs):
            return (None,) * 17
        # the scale stays on the device: the kernel reads it
        G = _host.photo_loss_gradient(image, target, lws, lambda_dssim=ctx.lambda_dssim,
                                      grad_loss=grad_loss.float().reshape(1).contiguous())
        dstats, dscale = ctx.densify
        # with statistics the same sweep also hands out the screen-space sums (its world-space outputs may all be NULL)
        grads, screen = _rasterize_backward(ctx.saved_tensors, ctx.view, ws, G, None, needs, want_screen=dstats is not None)
        if dstats is not None:
            m, q, s, _ = ctx.saved_tensors
            viewmat, K, W, H, eps2d, _ = ctx.view
            _host.densify_accumulate(dstats, screen, ws, W, H, scale=dscale, geometry=(m, q, s, viewmat, K, eps2d))
        return grads + (None,) * 12


def splat_photometric(means, quats, scales, opacities, colors, viewmat, K, W, H, target, *, lambda_dssim=0.2, near=0.01,
                      far=1e10, eps2d=0.3, check=True, densify_stats=None, stats_scale=1.0):
    """The photometric loss of the splatted colour rows of one W x H view against the view's photograph: L1 + D-SSIM with
    the 11 x 11 Gaussian window (include/voxproj.h states the contract of vp_photo_loss).

      means, quats, scales, opacities, viewmat, K   as ``splat_gaussians``
      colors f32 [N,C]                the view-independent colour rows (C = 3 for RGB; up to 64); any of the five tensors may
                                      require grad
      target f32 [C,H,W] on the GPU   the photograph, planar; no gradient flows to it

    Returns (loss f32 0-dim = (1 - lambda_dssim) mean |x - y| + lambda_dssim (1 - mean SSIM), stats f64 [3] = {sum |x - y|,
    sum (x - y)^2, sum SSIM}, detached; voxproj_host.image_metrics turns them into l1 / psnr / ssim).  Forward:
    vp_splat_project, vp_splat_rasterize (the image is kept), vp_photo_loss.  Backward: vp_photo_loss_gradient writes the
    gradient image (the upstream scalar is read on the device), then vp_splat_rasterize_backward_geometry, or
    vp_splat_rasterize_backward when no geometry gradient is asked for.  No torch pass over an image, no double backward, no
    gradient for the camera.

    ``densify_stats``: a voxproj_host.DensifyStats.  The backward then runs the geometry backward (also when only the colours
    or opacities require grad), asks it for the screen-space sums as well and adds the view to the statistics
    (vp_densify_accumulate) with ``stats_scale``, which undoes the 1 / k of a step that averages k views.  The loss and the
    gradients are bit-identical with and without it; with None the call sequence is unchanged."""
    _require_f32(means, quats, scales, opacities, colors=colors, target=target)
    lam = float(lambda_dssim)
    _host._require(0.0 <= lam <= 1.0, f"lambda_dssim = {lambda_dssim} outside [0, 1]")
    _refuse_grad("no gradient flows to the photograph (detach it)", target=target)
    _host._require(densify_stats is None or
                   (isinstance(densify_stats, _host.DensifyStats) and densify_stats.n == int(means.shape[0])),
                   "densify_stats must be a voxproj_host.DensifyStats of the cloud's size")
    return SplatPhotometric.apply(means, quats, scales, opacities, colors, viewmat, K, int(W), int(H), target, lam, float(near),
                                  float(far), float(eps2d), bool(check), densify_stats, float(stats_scale))


class SHColors(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f_dc, f_rest, means, viewmat, degree):
        d, r, m = f_dc.detach(), f_rest.detach(), means.detach()
        colors, clamped = _host.sh_colors(d, r, m, viewmat, degree, want_clamped=True)
        ctx.view = (viewmat, degree)
        ctx.save_for_backward(d, r, m, clamped)
        return colors

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_colors):
        d, r, m, clamped = ctx.saved_tensors
        viewmat, degree = ctx.view
        need_dc, need_rest, need_means = ctx.needs_input_grad[:3]
        if not (need_dc or need_rest or need_means):
            return (None,) * 5
        g_dc, g_rest, g_means = _host.sh_colors_backward(d, r, m, viewmat, degree, grad_colors.float().contiguous(), clamped,
                                                         want_dc=need_dc, want_rest=need_rest, want_means=need_means)
        return g_dc, g_rest, g_means, None, None


def sh_colors(f_dc, f_rest, means, viewmat, degree):
    """The view-dependent colour rows f32 [N,3] of Gaussians whose appearance is a spherical-harmonics expansion, for the
    camera of ``viewmat`` (include/voxproj_ext.h states the contract of vp_sh_colors):

      f_dc f32 [N,3], f_rest f32 [N,Kr,3]   the reference's parameter layout, Kr = (Dmax + 1)^2 - 1 for a Dmax in 0 .. 3
      means f32 [N,3]                       the direction is (mean - campos) / |mean - campos|, campos = -R^T t of viewmat
      degree                                the active degree, 0 <= degree <= Dmax; coefficients beyond it are not read

    colour = max(0.5 + sum_k Y_k(dir) sh[k], 0).  The result is what ``splat_photometric(colors=...)`` and ``splat_gaussians``
    take as their rows.  Differentiable in f_dc, f_rest and means (the gradient passes the clamp where the value before it
    is >= 0; f_rest receives exact zeros beyond the active degree); a mean that also feeds the rasterizer receives the sum of
    both gradients through autograd's own accumulation.  No double backward, no gradient for the camera."""
    _host._require_tensors((f_dc, "f_dc", (torch.float32,)), (f_rest, "f_rest", (torch.float32,)), (means, "means", (torch.float32,)))
    _refuse_grad("sh_colors has no gradient for the camera (detach viewmat)", viewmat=viewmat)
    return SHColors.apply(f_dc, f_rest, means, viewmat, int(degree))


class CodebookLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, codebook, image, ids, conf, assign, weights, conf_min, ignore_id):
        K = int(codebook.shape[0])
        stats, g_cls, g_clu, _, _ = _host.codebook_loss(image, ids, conf, codebook.detach(), assign, conf_min=conf_min,
                                                         ignore_id=ignore_id)
        n = stats[2].clamp(min=1.0)
        zero = torch.zeros_like(stats[0])
        # "never reinforce correct labels": the cross-entropy and its gradient are off when no pixel's argmax misses its
        # label; log K = 0 at K = 1, where the cross-entropy is identically 0 anyway: it is taken as 0
        on = (stats[3] > 0) & (stats[2] > 0) if K > 1 else torch.zeros_like(stats[0], dtype=torch.bool)
        scale_cls = torch.where(on, weights[0] / (n * math.log(max(K, 2))), zero)
        scale_clu = torch.where(stats[2] > 0, weights[1] / n, zero)
        loss = scale_cls * stats[0] + scale_clu * stats[1]
        ctx.save_for_backward(g_cls, g_clu, scale_cls.float(), scale_clu.float())
        ctx.mark_non_differentiable(stats)
        return loss.float(), stats

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _grad_stats):
        g_cls, g_clu, scale_cls, scale_clu = ctx.saved_tensors
        grad = None
        if ctx.needs_input_grad[0]:
            grad = grad_loss.float() * (scale_cls * g_cls + scale_clu * g_clu)
        return (grad,) + (None,) * 7


def codebook_loss(image, ids, conf, codebook, assign, *, weight_cls=1.0, weight_cluster=1.0, conf_min=0.2, ignore_id=-1):
    """The loss that ties one view's mask ids to a code book of global instance labels (include/voxproj.h states the
    contract of vp_codebook_loss), differentiable IN THE CODE BOOK ONLY: the image is a constant, as in the method this
    follows, where it is detached.

      image f32 [D,H,W] on the GPU    the rendered identity rows (splat_features' logits)
      ids int32 [H,W]                 the view's mask; conf f32 [H,W] or None: pixels with conf <= conf_min take no part
      codebook f32 [K,D]              the parameter
      assign int32 [256] on the GPU   id -> code (voxproj_host.assign_view_ids), -1: the id takes no part

    L = weight_cls cls + weight_cluster stats[1] / n with n = stats[2] the participating pixels and
    cls = stats[0] / (n log K).  cls and its gradient are 0 when stats[3] = 0 (every pixel's argmax already is its label),
    L is 0 when n = 0; both switches are torch.where on device scalars, without a synchronisation.  At K = 1, log K = 0 and
    the cross-entropy of a single code is identically 0: cls is defined as 0 there.
    Returns (loss f32 0-dim, stats f64 [4], detached).  Forward: vp_codebook_loss, which also leaves the two unscaled
    gradient sums; backward scales and adds two [K,D] tensors.  No double backward."""
    _host._require_tensors((codebook, "codebook", (torch.float32,)))
    _refuse_grad("codebook_loss is differentiable in the code book only (detach it)", image=image)
    return CodebookLoss.apply(codebook, image, ids, conf, assign, (float(weight_cls), float(weight_cluster)), float(conf_min),
                              int(ignore_id))


class NeighborConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, sample, scale, want_sample_loss):
        stats, row_lse, sample_loss, _ = _host.neighbor_kl(logits, sample, want_sample_loss=want_sample_loss)
        P = int(logits.shape[1])
        coef = scale / (sample.S * sample.k * P) if sample.S else 0.0
        ctx.save_for_backward(logits.detach(), row_lse)
        ctx.sample, ctx.scale = sample, scale
        out = sample_loss if sample_loss is not None else stats.new_zeros(0, dtype=torch.float32)
        ctx.mark_non_differentiable(out)
        return (coef * stats[0]).float(), out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _grad_sample_loss):
        logits, row_lse = ctx.saved_tensors
        grad = None
        if ctx.needs_input_grad[0]:
            grad = _host.neighbor_kl_gradient(logits, ctx.sample, row_lse, scale=ctx.scale,
                                              grad_loss=grad_loss.float().reshape(1).contiguous())
        return grad, None, None, None


def neighbor_consistency(logits, table, *, scale=2.0, sample=None, want_sample_loss=False):
    """The 3D neighbourhood regulariser (include/voxproj.h states the contract of vp_neighbor_kl; the reference's
    loss_cls_3d, utils/loss_utils.py:74-115): the mean KL divergence between a Gaussian's class distribution and those of its
    nearest neighbours in space, differentiable IN THE LOGITS ONLY (the positions are fixed: the table is built once).

      logits f32 [N,P] on the GPU       the parameter, 1 <= P <= 256
      table                             voxproj_host.NeighborTable(points, k); k counts the point itself (the reference's reg3d_k)
      scale                             the reference's lambda_val
      sample                            None: every Gaussian; an integer tensor [S] of rows (repeats allowed), or a
                                        voxproj_host.NeighborSample from table.select

    loss = scale / (S k P) sum_s sum_j sum_c p_sc (log(p_sc + 1e-10) - log(p_jc + 1e-10)), 0 for an empty sample.
    Returns the loss (f32 0-dim), or (loss, sample_loss f32 [S], unscaled and detached) with ``want_sample_loss``.  Forward:
    vp_neighbor_kl; backward: vp_neighbor_kl_gradient, one launch, no float atomics.  No double backward."""
    _host._require_tensors((logits, "logits", (torch.float32,)))
    if sample is None:
        sample = table.all
    elif isinstance(sample, torch.Tensor):
        sample = table.select(sample)
    loss, sample_loss = NeighborConsistency.apply(logits, sample, float(scale), bool(want_sample_loss))
    return (loss, sample_loss) if want_sample_loss else loss
