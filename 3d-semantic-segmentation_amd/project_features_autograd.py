"""Differentiable projection: the forward projector as a ``torch.autograd.Function``.

The projector is linear in the feature maps:  out[id, :] = sum of feats[p, :] over the pixels p whose ray hits voxel ``id``
first.  Its transpose copies, for every pixel, the row of that voxel (vp_render_features), so the gradient of a loss on
``out`` with respect to ``feats`` is the upstream gradient rendered through the forward call's own first-hit assignment:

    grad_feats[p, :] = grad_out[hit[p], :]        (zeros where the ray hits nothing)

The forward keeps that assignment -- one int32 per pixel, copied out of the workspace right behind the call -- and the backward
is one render launch.  Gradients flow to the feature maps only: the assignment is piecewise constant in the poses and the
occupancy.  No double backward.

The in-place drop-in (project_features_cuda, both fronts) is not differentiable and stays so: it keeps the reference's
signature.  This module is the differentiable entry point.
"""
import threading

import torch
from torch.autograd.function import once_differentiable

import voxproj_host as _host

__all__ = ["project_features", "ProjectFeatures"]

_workspaces = {}
_lock = threading.Lock()     # the forward call and the copy of its hit image must not be separated by another call


def _workspace(device):
    key = (device.type, device.index)
    ws = _workspaces.get(key)
    if ws is None:
        ws = _workspaces[key] = _host.Workspace()
    return ws


class ProjectFeatures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, occ, vmi, intr, opts5, grid_origin3, voxel_size, n_rows, reduce):
        dev = feats.device
        B, V, H, W, C = (int(v) for v in feats.shape)
        n_rows = int(n_rows)
        out = torch.zeros((n_rows, C), dtype=torch.float32, device=dev)
        count = torch.zeros((n_rows,), dtype=torch.int32, device=dev)
        ids = torch.empty((B, V, H, W), dtype=torch.int32, device=dev)
        f = feats.detach().contiguous()
        with _lock:
            ws = _host.project_features_raw(f, occ, vmi.reshape(-1), intr, opts5, count, out, grid_origin3, voxel_size,
                                            workspace=_workspace(dev), sync=True)
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev)
                _host.check(_host.lib().vp_copy_hit_image(ws.ptr(), ids.data_ptr(), B, V, H, W, C, *occ.shape[1:], n_rows,
                                                          stream.cuda_stream))
                # the copy reads the workspace's hit image: it must have run before another forward (another thread, another
                # stream) can march into the same workspace.  The forward call blocked already; this waits for one copy.
                stream.synchronize()
        if reduce == "mean":
            out = out / count.clamp(min=1)[:, None].to(torch.float32)
        ctx.save_for_backward(ids, count)
        ctx.mark_non_differentiable(count)
        ctx.reduce = reduce
        ctx.feats_dtype = feats.dtype
        ctx.feats_shape = feats.shape
        return out, count

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, grad_count):
        ids, count = ctx.saved_tensors
        g = grad_out.to(torch.float32)
        if ctx.reduce == "mean":
            g = g / count.clamp(min=1)[:, None].to(torch.float32)
        grad = _host.render_features(ids, g.contiguous(), dtype=ctx.feats_dtype, check=False)
        return grad.reshape(ctx.feats_shape), None, None, None, None, None, None, None, None


def project_features(feats, occ, vmi, intr, opts5, grid_origin3, voxel_size, n_rows, reduce="sum"):
    """Differentiable projection of feature maps into voxel rows.

      feats        float32 or float16 [B,V,H,W,C] CUDA (float16: C % 8 == 0), may require grad
      occ          int64 [B,Z,Y,X] CUDA, 0 = empty, else voxel ID in [1, n_rows)
      vmi          float32 [B*V*16] (or [B,V,4,4]) camera->world, intr float32 [B,4] = fx, fy, cx, cy, both CUDA
      opts5        [W, H, depth_min, depth_max, ray_increment];  grid_origin3, voxel_size: the occupancy grid
      reduce       "sum": out = per-voxel sum of the pixels' rows; "mean": that sum / max(count, 1)

    Returns fresh tensors (out float32 [n_rows, C], count int32 [n_rows]); ``count`` is not differentiable.  The gradient
    with respect to ``feats`` has ``feats``' dtype."""
    if reduce not in ("sum", "mean"):
        raise ValueError(f"reduce must be 'sum' or 'mean', not {reduce!r}")
    if not isinstance(feats, torch.Tensor) or feats.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"feats must be a float32 or float16 tensor, not {getattr(feats, 'dtype', type(feats))}")
    if feats.dim() != 5:
        raise ValueError("feats must be [B,V,H,W,C]")
    for t, name, dt in ((occ, "occ", torch.int64), (vmi, "vmi", torch.float32), (intr, "intr", torch.float32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise ValueError(f"{name} must be a {dt} tensor")
    # shapes: the library takes B, V, H, W and C from feats and only the grid's dims from occ -- a mismatch would read past
    # occ, vmi or intr on the device
    B, V, H, W, C = (int(v) for v in feats.shape)
    if min(B, V, H, W, C) <= 0:
        raise ValueError("feats must be [B,V,H,W,C] with every dimension >= 1")
    if occ.dim() != 4 or int(occ.shape[0]) != B or min(int(v) for v in occ.shape) <= 0:
        raise ValueError(f"occ must be [B,Z,Y,X] with B = {B} (feats' batch), not {tuple(occ.shape)}")
    if vmi.numel() != B * V * 16:
        raise ValueError(f"vmi must hold B*V*16 = {B * V * 16} floats (one camera->world matrix per view), not {vmi.numel()}")
    if intr.numel() != B * 4 or (intr.dim() == 2 and int(intr.shape[1]) != 4):
        raise ValueError(f"intr must be [B,4] with B = {B}, not {tuple(intr.shape)}")
    if len(opts5) != 5:
        raise ValueError("opts5 must hold 5 values: W, H, depth_min, depth_max, ray_increment")
    if int(float(opts5[0]) + 0.5) != W or int(float(opts5[1]) + 0.5) != H:
        raise ValueError(f"opts5 width/height ({opts5[0]}, {opts5[1]}) must equal feats' ({W}, {H})")
    if len(grid_origin3) != 3:
        raise ValueError("grid_origin3 must hold 3 values")
    if int(n_rows) < 1:
        raise ValueError("n_rows must be >= 1")
    if not feats.is_cuda:
        raise ValueError("feats must be a CUDA tensor: there is no CPU path")
    for t, name in ((occ, "occ"), (vmi, "vmi"), (intr, "intr")):
        if not (t.is_cuda and t.device == feats.device):
            raise ValueError(f"{name} must be a CUDA tensor on feats' device")
    return ProjectFeatures.apply(feats, occ.contiguous(), vmi.contiguous().reshape(-1), intr.contiguous().reshape(B, 4),
                                 [float(v) for v in opts5],
                                 [float(v) for v in grid_origin3], float(voxel_size), int(n_rows), reduce)
