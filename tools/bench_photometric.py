"""The photometric loss (L1 + D-SSIM) and its gradient image on one rendered image (no Gaussians: the loss is what is
measured): vp_photo_loss plus vp_photo_loss_gradient against a torch autograd composite of the same formula in float32 on the
GPU -- five depthwise conv2d with the 11 x 11 window, the element-wise passes of utils/loss_utils.py's _ssim, torch.abs for
the L1 part, forward plus backward to the image.  The image is WxH with C channels: sinusoids plus noise against the same
sinusoids plus other noise.

One JSON line:
  forward_ms / gradient_ms / fused_ms   HIP events around --steps calls after --warmup; fused = forward + gradient
  evaluate_ms                           the forward without a workspace: one workgroup walks the tiles (evaluation only)
  torch_ms                              the composite's forward plus backward to the image's gradient
  forward_bytes / gradient_bytes        what the calls must move at least: 2 n reads + 3 n writes, 5 n reads + n writes of four
                                        bytes, with the rate against --hbm_gbs
  loss_rel_diff / grad_max_diff_over_max   the two arms' results compared before anything is timed

python tools/bench_photometric.py [--steps K] [--warmup W] [--size 1600x1067] [--c 3] [--lambda_dssim 0.2]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import voxproj_host  # noqa: E402
from bench_splat import timed  # noqa: E402

ROW = [float.fromhex(h) for h in ("0x1.0d956cp-10", "0x1.f1fe02p-8", "0x1.26eb18p-5", "0x1.bff0fep-4", "0x1.b43c3ep-3",
                                  "0x1.10656p-2", "0x1.b43c3ep-3", "0x1.bff0fep-4", "0x1.26eb18p-5", "0x1.f1fe02p-8",
                                  "0x1.0d956cp-10")]


def composite(x, y, window, lam):
    """(1 - lam) mean |x - y| + lam (1 - mean SSIM) in torch float32, differentiable in ``x`` [C,H,W]."""
    C = x.shape[0]

    def ws(a):
        return F.conv2d(a[None], window, padding=5, groups=C)[0]

    mu1, mu2 = ws(x), ws(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = ws(x * x) - mu1_sq, ws(y * y) - mu2_sq, ws(x * y) - mu1_mu2
    m = ((2 * mu1_mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1_sq + mu2_sq + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    return (1.0 - lam) * (x - y).abs().mean() + lam * (1.0 - m.mean())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", default="1600x1067")
    ap.add_argument("--c", type=int, default=3)
    ap.add_argument("--lambda_dssim", type=float, default=0.2)
    ap.add_argument("--hbm_gbs", type=float, default=6300.0, help="the streaming rate the calls are compared with")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    W, H = (int(v) for v in args.size.split("x"))
    C, lam = args.c, args.lambda_dssim
    n = C * W * H
    gen = torch.Generator(dev).manual_seed(0)
    yy = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
    xx = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
    ch = torch.arange(C, device=dev, dtype=torch.float32)[:, None, None]
    base = 0.5 + 0.3 * torch.sin(0.021 * xx + 0.7 * ch) * torch.cos(0.017 * yy - 0.3 * ch)
    image = (base + 0.1 * torch.randn((C, H, W), device=dev, generator=gen)).clamp(0, 1).contiguous()
    target = (base + 0.1 * torch.randn((C, H, W), device=dev, generator=gen)).clamp(0, 1).contiguous()
    row = torch.tensor(ROW, dtype=torch.float32, device=dev)
    window = (row[:, None] * row[None, :]).expand(C, 1, 11, 11).contiguous()
    grad = torch.empty_like(image)
    ws = voxproj_host.SplatWorkspace()

    def forward(i=0):
        return voxproj_host.photo_loss(image, target, workspace=ws)[0]

    def gradient(i=0):
        return voxproj_host.photo_loss_gradient(image, target, ws, lambda_dssim=lam, out=grad)

    def fused(i=0):
        forward()
        gradient()

    def evaluate(i=0):
        return voxproj_host.photo_loss(image, target, evaluate_only=True)[0]

    def torch_step(i=0):
        x = image.detach().requires_grad_()
        loss = composite(x, target, window, lam)
        loss.backward()
        return loss.detach(), x.grad

    stats = forward()
    gradient()
    assert torch.equal(evaluate(), stats), "the evaluation path's statistics are not the workspace path's bits"
    lt, gt = torch_step()
    lf = float((1.0 - lam) * stats[0] / n + lam * (1.0 - stats[2] / n))
    loss_diff = abs(lf - float(lt)) / abs(float(lt))
    gdiff = float((grad - gt).abs().max() / gt.abs().max())
    assert loss_diff <= 1e-4 and gdiff <= 1e-2, f"the two arms differ: loss {loss_diff:.3e}, gradient {gdiff:.3e}: nothing is timed"
    del gt
    ms = dict(forward=[], gradient=[], fused=[], evaluate=[], torch=[])
    for _ in range(2):                                      # the arms alternated twice; the best of each
        ms["forward"].append(timed(forward, args.steps, args.warmup))
        ms["gradient"].append(timed(gradient, args.steps, args.warmup))
        ms["fused"].append(timed(fused, args.steps, args.warmup))
        ms["evaluate"].append(timed(evaluate, max(args.steps // 4, 2), 1))
        ms["torch"].append(timed(torch_step, args.steps, args.warmup))
    best = {k: min(v) for k, v in ms.items()}
    fwd_bytes, grad_bytes = 5 * 4 * n, 6 * 4 * n
    met = voxproj_host.image_metrics(stats, n)
    res = dict(metric="photo_loss_ms", W=W, H=H, C=C, lambda_dssim=lam, forward_ms=round(best["forward"], 3),
               gradient_ms=round(best["gradient"], 3), fused_ms=round(best["fused"], 3), evaluate_ms=round(best["evaluate"], 3),
               torch_ms=round(best["torch"], 3), fused_over_torch=round(best["fused"] / best["torch"], 4),
               runs={k: [round(x, 3) for x in v] for k, v in ms.items()},
               forward_bytes=fwd_bytes, forward_gbs=round(fwd_bytes / best["forward"] / 1e6, 1),
               forward_of_stream_rate=round(fwd_bytes / best["forward"] / 1e6 / args.hbm_gbs, 3),
               gradient_bytes=grad_bytes, gradient_gbs=round(grad_bytes / best["gradient"] / 1e6, 1),
               gradient_of_stream_rate=round(grad_bytes / best["gradient"] / 1e6 / args.hbm_gbs, 3), hbm_gbs=args.hbm_gbs,
               loss=lf, psnr=round(met["psnr"], 3), ssim=round(met["ssim"], 5), loss_rel_diff=loss_diff,
               grad_max_diff_over_max=gdiff, steps=args.steps, warmup=args.warmup)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
