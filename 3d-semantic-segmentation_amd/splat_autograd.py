"""Differentiable Gaussian splatting: the splatting forward (vp_splat_project + vp_splat_rasterize) as a
``torch.autograd.Function``, with vp_splat_rasterize_backward as its backward.

Gradients flow from the logits [D,H,W] and alpha [H,W] to the per-Gaussian features [N,D] and the activated opacities [N],
through the branch the forward took (include/voxproj.h states the contract).  Labels and confidence are returned but not
differentiable.  Geometry gradients (means, quats, scales) are not implemented: a call whose geometry requires grad raises
instead of dropping them.  No double backward.

Each call keeps its own SplatWorkspace until its backward has run (the backward reads the forward's sorted intersections),
so calls from several threads or views share no state.  The workspace is freed after the backward, or with the graph.
"""
import torch
from torch.autograd.function import once_differentiable

import voxproj_host as _host

__all__ = ["splat_features", "SplatFeatures"]


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
        ws, ctx.ws = ctx.ws, None
        W, H, cap = ctx.shape
        want_f, want_o = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gf = go = None
        if want_f or want_o:
            gf, go = _host.splat_rasterize_backward(f, int(f.shape[0]), W, H, cap, ws,
                                                    grad_logits=grad_logits.float() if grad_logits is not None else None,
                                                    grad_alpha=grad_alpha.float() if grad_alpha is not None else None,
                                                    want_features=want_f, want_opacities=want_o)
        return gf, go, None, None, None, None, None, None, None, None, None, None, None


def splat_features(means, quats, scales, opacities, features, viewmat, K, W, H, *, near=0.01, far=1e10, eps2d=0.3,
                   check=True):
    """Differentiable splatting of D-channel per-Gaussian features into one W x H view.

      means f32 [N,3], quats f32 [N,4], scales f32 [N,3]   the geometry, on the GPU; must not require grad
      opacities f32 [N] (activated), features f32 [N,D]   D <= 64, on the same GPU; either may require grad
      viewmat [4,4] world-to-camera, K [3,3]               any device, read on the host

    Returns (logits f32 [D,H,W], alpha f32 [H,W], labels int32 [H,W], confidence f32 [H,W]); only logits and alpha are
    differentiable.  The images are bit-identical to voxproj_host.splat_features(..., want_logits=True, want_alpha=True).
    ``check``: raise when a Gaussian has a non-finite parameter (it is culled either way)."""
    for t, name in ((means, "means"), (quats, "quats"), (scales, "scales")):
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise ValueError(f"{name} requires grad, but geometry gradients are not implemented: only the features and "
                             "the opacities are differentiable (detach the geometry)")
    _host._require_tensors(*((t, name, (torch.float32,)) for t, name in
                             ((means, "means"), (quats, "quats"), (scales, "scales"), (opacities, "opacities"),
                              (features, "features"))))
    return SplatFeatures.apply(features, opacities, means, quats, scales, viewmat, K, int(W), int(H), float(near), float(far),
                               float(eps2d), bool(check))
