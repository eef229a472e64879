"""The prototype-contrastive loss and its gradient image on one rendered identity image (no Gaussians: the loss is what is
measured): vp_proto_contrast plus vp_proto_contrast_gradient against a VECTORISED torch autograd composite of the same loss
in float32 on the GPU -- one-hot matmuls for the per-id sums and the softmax, no loop over ids, no host synchronisation.
The image is WxH with D channels: --ids rectangles of a grid, each with its own direction plus noise.  Two arms:

  all      every pixel once (count = NULL); the composite works on all W H rows
  sampled  --samples pixels drawn with replacement; the fused call gets the multiplicity map (torch.bincount of the draw), the
           composite gathers the drawn rows (duplicates and all), which is the cheapest honest way to write it in torch

One JSON line per arm:
  forward_ms / gradient_ms / fused_ms   HIP events around --steps calls after --warmup; fused = forward + gradient
  torch_ms                              the composite's forward plus backward to the image's gradient
  forward_bytes / gradient_bytes        what the calls must move at least: the image three times (sampled: once; the second
                                        and third read touch the drawn rows only) plus the mask and the count map per read;
                                        the image once and the gradient image once; with the rate against --hbm_gbs
  loss_rel_diff / grad_max_diff_over_max   the two arms' results compared before anything is timed

python tools/bench_contrast.py [--steps K] [--warmup W] [--size 1600x1067] [--d 16] [--ids 40] [--samples 32768]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402
import voxproj_host  # noqa: E402
from bench_splat import timed  # noqa: E402

PHI_SCALE, PHI_MIN, PHI_MAX, MIN_COUNT = 10.0, 0.5, 1.0, 20


def composite(image, ids, draw, n_cols):
    """The loss in torch float32, differentiable in ``image`` [D,H,W]; ``draw``: int64 pixel indices (duplicates kept) or
    None for every pixel once.  Returns the scalar  (sum l) / K + mean (r - 1)^2."""
    D = image.shape[0]
    f = image.reshape(D, -1).T
    r_all = f.norm(dim=-1)
    reg = ((r_all - 1.0) ** 2).mean()
    lab = ids.reshape(-1).long()
    if draw is not None:
        f, lab, r = f[draw], lab[draw], r_all[draw]
    else:
        r = r_all
    s = f / (r + 1e-6).detach()[:, None]
    onehot = torch.nn.functional.one_hot(lab.clamp(0, n_cols - 1), n_cols).float()
    n_k = onehot.sum(0)
    active = n_k > MIN_COUNT
    K = active.sum()
    nk = n_k.clamp(min=1.0)
    u = (onehot.T @ s) / nk[:, None]
    dist = (s - onehot @ u).norm(dim=1)
    phi = (PHI_SCALE * (onehot.T @ dist) / (nk * torch.log(nk + 10.0))).clamp(PHI_MIN, PHI_MAX).detach()
    z = (s @ u.T) / phi[None, :]
    e = torch.where(active[None, :], torch.exp(z), torch.zeros_like(z))
    valid = (onehot * active[None, :].float()).sum(1)
    l = torch.log(e.sum(1) + 1e-6) - (z * onehot).sum(1)
    total = (valid * l).sum()
    return torch.where(K > 0, total / K.clamp(min=1).float(), torch.zeros_like(total)) + reg


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", default="1600x1067")
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--ids", type=int, default=40)
    ap.add_argument("--samples", type=int, default=32768)
    ap.add_argument("--hbm_gbs", type=float, default=6300.0, help="the streaming rate the calls are compared with")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    W, H = (int(v) for v in args.size.split("x"))
    D, n = args.d, W * H
    gen = torch.Generator(dev).manual_seed(0)
    cols = 8
    rows = (args.ids + cols - 1) // cols
    yy = torch.arange(H, device=dev)[:, None] * rows // H
    xx = torch.arange(W, device=dev)[None, :] * cols // W
    ids = (yy * cols + xx).clamp(max=args.ids - 1).to(torch.int32).contiguous()
    dirs = torch.randn((args.ids, D), device=dev, generator=gen)
    image = (dirs[ids.long()] + 0.5 * torch.randn((H, W, D), device=dev, generator=gen)).permute(2, 0, 1).contiguous()
    draw = torch.randint(0, n, (args.samples,), generator=torch.Generator().manual_seed(1)).to(dev)
    count = torch.bincount(draw, minlength=n).reshape(H, W).to(torch.int32)
    grad = torch.empty_like(image)
    ws = voxproj_host.SplatWorkspace()
    kw = dict(min_count=MIN_COUNT, phi_scale=PHI_SCALE, phi_min=PHI_MIN, phi_max=PHI_MAX)

    for arm, cnt, drw in (("all", None, None), ("sampled", count, draw)):
        def forward(i=0):
            return voxproj_host.proto_contrast(image, ids, cnt, workspace=ws, **kw)[0]

        def gradient(i=0):
            return voxproj_host.proto_contrast_gradient(image, ids, cnt, ws, out=grad)

        def fused(i=0):
            forward()
            gradient()

        def torch_step(i=0):
            x = image.detach().requires_grad_()
            loss = composite(x, ids, drw, args.ids)
            loss.backward()
            return loss.detach(), x.grad

        stats = forward()
        gradient()
        lt, gt = torch_step()
        lf = float(stats[0] / stats[1] + stats[2] / n)
        loss_diff = abs(lf - float(lt)) / abs(float(lt))
        gdiff = float((grad - gt).abs().max() / gt.abs().max())
        assert int(stats[1]) == args.ids, f"{int(stats[1])} active ids, expected {args.ids}"
        assert loss_diff <= 1e-4 and gdiff <= 1e-3, f"the two arms differ: loss {loss_diff:.3e}, gradient {gdiff:.3e}: nothing is timed"
        del gt
        ms = dict(forward=[], gradient=[], fused=[], torch=[])
        for _ in range(2):                                      # the arms alternated twice; the best of each
            ms["forward"].append(timed(forward, args.steps, args.warmup))
            ms["gradient"].append(timed(gradient, args.steps, args.warmup))
            ms["fused"].append(timed(fused, args.steps, args.warmup))
            ms["torch"].append(timed(torch_step, args.steps, args.warmup))
        best = {k: min(v) for k, v in ms.items()}
        maps = 4 * n * (1 if cnt is None else 2)
        fwd_bytes = (3 if cnt is None else 1) * 4 * D * n + 3 * maps
        grad_bytes = 2 * 4 * D * n + maps
        res = dict(metric="proto_contrast_ms", arm=arm, W=W, H=H, D=D, ids=args.ids, samples=None if cnt is None else args.samples,
                   forward_ms=round(best["forward"], 3), gradient_ms=round(best["gradient"], 3), fused_ms=round(best["fused"], 3),
                   torch_ms=round(best["torch"], 3), fused_over_torch=round(best["fused"] / best["torch"], 4),
                   runs={k: [round(x, 3) for x in v] for k, v in ms.items()},
                   forward_bytes=fwd_bytes, forward_gbs=round(fwd_bytes / best["forward"] / 1e6, 1),
                   forward_of_stream_rate=round(fwd_bytes / best["forward"] / 1e6 / args.hbm_gbs, 3),
                   gradient_bytes=grad_bytes, gradient_gbs=round(grad_bytes / best["gradient"] / 1e6, 1),
                   gradient_of_stream_rate=round(grad_bytes / best["gradient"] / 1e6 / args.hbm_gbs, 3), hbm_gbs=args.hbm_gbs,
                   loss=lf, loss_rel_diff=loss_diff, grad_max_diff_over_max=gdiff, steps=args.steps, warmup=args.warmup)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
