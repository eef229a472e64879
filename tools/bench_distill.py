"""One training step of per-Gaussian feature rows against a 2D feature map (forward plus backward to the rows' gradient):
the fused call, splat_autograd.splat_feature_loss, against the same step on the interface the library had before it,
splat_wide_features(dtype=float32) plus a torch loss with the same validity mask and autograd.  The scene of
tools/bench_lift.py: --g Gaussians of synthetic_gaussians.make_gaussians, view 0 of the trajectory at WxH, C channels; the map
is seeded fp16 noise, the rows seeded fp32 noise.  One JSON line:

  fused_ms / torch_ms      HIP events around --steps steps after --warmup, the two arms alternated twice; the best of each
  fused_peak_bytes / torch_peak_bytes   torch.cuda.max_memory_allocated over one step of the arm, above what was allocated
                           before it
  grad_max_diff_over_tol   largest |fused gradient - torch gradient| over the tolerance below; above 1 nothing is timed
  loss_ms / gradient_ms    vp_feature_loss and vp_feature_loss_gradient alone on the rendered fp16 image, with the bytes they
                           must move (both maps read once; the gradient call also writes one) and the rate against --hbm_gbs

The tolerance of the gradient comparison is the one of tests/test_gpu_splat_distill.py::test_agreement_with_the_torch_path,
in a form that needs no float64 lift of a 1600 x 1067 x 512 map: both gradients are lifts of maps that differ, per element,
by at most twice 2^-11 of the map's largest element (the quantisation to binary16 with one exponent; the fp32 error of
either path is far below it), so they differ by at most  2 * 2^-11 * max|G| * sum_p w_g(p)  per Gaussian, plus twice the
lift's own 1e-4 of the magnitude; sum_p w_g(p) is lifted from a map of ones.

python tools/bench_distill.py [--steps K] [--warmup W] [--g 200000] [--size 1600x1067] [--c 512] [--kind cosine|l2]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402
import splat_autograd  # noqa: E402
import synthetic_gaussians as sg  # noqa: E402
import voxproj_host  # noqa: E402
from bench_splat import timed  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--g", type=int, default=200000)
    ap.add_argument("--size", default="1600x1067")
    ap.add_argument("--c", type=int, default=512)
    ap.add_argument("--kind", choices=("cosine", "l2"), default="cosine")
    ap.add_argument("--min_alpha", type=float, default=0.5)
    ap.add_argument("--hbm_gbs", type=float, default=6300.0, help="the streaming rate the two kernels are compared with")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    G, C, kind, min_alpha = args.g, args.c, args.kind, args.min_alpha
    W, H = (int(v) for v in args.size.split("x"))
    g = sg.make_gaussians(G, seed=0)
    t = {k: torch.from_numpy(g[k]).to(dev) for k in ("means", "quats", "scales", "opacities")}
    w2c, K = sg.make_views(8 * 12, g["room"], W, seed=0)       # view 0 of bench_splat.py
    vm = w2c[0]
    gen = torch.Generator(dev).manual_seed(0)
    target = torch.randn((H, W, C), device=dev, generator=gen, dtype=torch.float32).to(torch.float16)
    rows = torch.randn((G, C), device=dev, generator=gen, dtype=torch.float32)
    geo = (t["means"], t["quats"], t["scales"], t["opacities"])

    def fused_step(i=0):
        x = rows.detach().requires_grad_()
        loss, _ = splat_autograd.splat_feature_loss(*geo, x, vm, K, W, H, target, kind=kind, min_alpha=min_alpha,
                                                    dtype=torch.float32 if i < 0 else torch.float16, check=False)
        loss.backward()
        return loss.detach(), x.grad

    def torch_step(i=0):
        x = rows.detach().requires_grad_()
        out, alpha = splat_autograd.splat_wide_features(*geo, x, vm, K, W, H, dtype=torch.float32, check=False)
        tt = target.float()
        valid = alpha >= min_alpha
        if kind == "cosine":
            valid = valid & ((out.detach() ** 2).sum(-1) > 0) & ((tt ** 2).sum(-1) > 0)
            o = torch.where(valid[..., None], out, torch.ones_like(out))
            per = 1.0 - torch.nn.functional.cosine_similarity(o, torch.where(valid[..., None], tt, torch.ones_like(tt)), dim=-1)
        else:
            per = ((out - tt) ** 2).mean(-1)
        m = valid.float()
        loss = (m * per).sum() / m.sum()
        loss.backward()
        return loss.detach(), x.grad

    # the comparison first, both arms on the fp32 image: the tolerance of the docstring
    la, ga = fused_step(-1)
    lb, gb = torch_step()
    ws, lw = voxproj_host.SplatWorkspace(), voxproj_host.SplatWorkspace()
    image, alpha, cap, _ = voxproj_host.splat_render_view(*geo, rows, vm, K, W, H, dtype=torch.float16, want_alpha=True,
                                                          workspace=ws, check=False)
    stats, _, fws = voxproj_host.feature_loss(image, target, None, alpha, kind=kind, min_alpha=min_alpha)
    Gq, k = voxproj_host.feature_loss_gradient(image, target, stats, fws, reduction="mean")
    gmax = float(Gq.float().abs().max()) * 2.0 ** -int(k)
    mag = torch.zeros((G, 1), device=dev)
    voxproj_host.splat_lift(torch.ones((H, W, 1), device=dev, dtype=torch.float16), G, W, H, cap, ws, mag, None, sorted=True,
                            lift_workspace=lw)
    tol = (2 * 2.0 ** -11 + 2e-4) * gmax * mag + 1e-30
    ratio = float(((ga - gb).abs() / tol).max())
    assert ratio <= 1.0, f"the two gradients differ by {ratio:.3f} of the tolerance: nothing is timed"
    assert abs(float(la) - float(lb)) <= 1e-4 * max(abs(float(lb)), 1e-6), (float(la), float(lb))
    del ga, gb, mag, tol
    torch.cuda.synchronize()

    def peak(step):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        step()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated(dev) - base)

    peaks = (peak(fused_step), peak(torch_step))
    ms = [timed(fn, args.steps, args.warmup) for fn in (fused_step, torch_step, fused_step, torch_step)]
    out16 = torch.empty_like(Gq)
    loss_ms = timed(lambda i: voxproj_host.feature_loss(image, target, None, alpha, kind=kind, min_alpha=min_alpha, workspace=fws),
                    args.steps, args.warmup)
    grad_ms = timed(lambda i: voxproj_host.feature_loss_gradient(image, target, stats, fws, reduction="mean", out=out16),
                    args.steps, args.warmup)
    best_f, best_t = min(ms[0], ms[2]), min(ms[1], ms[3])
    maps = 2 * W * H * C * 2
    res = dict(metric="distill_step_ms", G=G, C=C, W=W, H=H, kind=kind, min_alpha=min_alpha, n_isect=cap,
               fused_ms=round(best_f, 3), torch_ms=round(best_t, 3), fused_over_torch=round(best_f / best_t, 4),
               fused_ms_runs=[round(ms[0], 3), round(ms[2], 3)], torch_ms_runs=[round(ms[1], 3), round(ms[3], 3)],
               fused_peak_bytes=peaks[0], torch_peak_bytes=peaks[1], grad_max_diff_over_tol=round(ratio, 4),
               loss=float(la), loss_torch=float(lb), grad_exponent=int(k),
               loss_ms=round(loss_ms, 3), loss_bytes=maps, loss_gbs=round(maps / loss_ms / 1e6, 1),
               gradient_ms=round(grad_ms, 3), gradient_bytes=maps + W * H * C * 2,
               gradient_gbs=round((maps + W * H * C * 2) / grad_ms / 1e6, 1), hbm_gbs=args.hbm_gbs,
               loss_of_stream_rate=round(maps / loss_ms / 1e6 / args.hbm_gbs, 3),
               gradient_of_stream_rate=round((maps + W * H * C * 2) / grad_ms / 1e6 / args.hbm_gbs, 3),
               steps=args.steps, warmup=args.warmup)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
