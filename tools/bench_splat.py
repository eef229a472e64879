"""Gaussian splatting of logits (vp_splat_project + vp_splat_rasterize) at the shapes of stage 5.2, one JSON line per leg:
G in {200k (the reference's 195 120-Gaussian scene), 1M} Gaussians of synthetic_gaussians.make_gaussians, D in {13, 32}
channels, 876x584 and 1600x1067 views from the synthetic trajectory, labels + confidence only or with the [D,H,W] logits.

  ms_per_view     HIP events around --steps views (cycled over --views cameras) after --warmup: splat_features as the CLI
                  calls it, the 8-byte count read included
  project_ms      vp_splat_project alone (projection + rocprim scan of the tile counts), same event timing
  raster_ms       vp_splat_rasterize alone (emit, rocprim radix sort, ranges, blend), same event timing
  n_isect         mean (tile, Gaussian) intersections per view = keys sorted
  isect_px_per_s  n_isect * 256 / raster_ms: the (Gaussian, pixel) pairs the blend may visit (an upper bound: pixels stop
                  at T <= 1e-4), per second of the whole rasterize call
  logits_GBs      D*H*W*4 bytes / raster_ms, when logits are written
The per-kernel split (project / scan / emit / sort / ranges / blend) is in the rocprofv3 --kernel-trace --stats run of one
leg committed under profiles/ (r08_splat_*).

With --backward, every logits-on leg adds a splat_backward_ms_per_view line: vp_splat_rasterize (logits and alpha) and
vp_splat_rasterize_backward (random gradients on both) on view 0, and their ratio (profiles/r09_splat_backward*).
With --geometry as well, one more splat_geometry_backward_ms_per_view line per leg: the fused
vp_splat_rasterize_backward_geometry asking for every gradient (means, quats, scales, features, opacities) beside the
existing backward on the same view and gradients, timed in alternation, and their ratio (profiles/r10_splat_geometry*).

With --loss, one splat_loss_step_ms line per (G, D, size) instead of the legs above: one refinement step on view 0
(forward + backward in the features, the intersection count read included) for three arms timed in alternation in one
process: the fused loss with the replay backward, the fused loss with the saved logits, and the composite
(splat_autograd.splat_features + F.cross_entropy + backward); torch.cuda.max_memory_allocated of each arm beside it.

python tools/bench_splat.py [--steps K] [--warmup W] [--g 200000 1000000] [--d 13 32] [--size 876x584 1600x1067]
[--logits off on] [--views V] [--backward [--geometry]] [--loss]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import synthetic_gaussians as sg  # noqa: E402
import voxproj_host  # noqa: E402


def timed(fn, steps, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--g", type=int, nargs="+", default=[200000, 1000000])
    ap.add_argument("--d", type=int, nargs="+", default=[13, 32])
    ap.add_argument("--size", nargs="+", default=["876x584", "1600x1067"])
    ap.add_argument("--logits", nargs="+", default=["off", "on"])
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--backward", action="store_true",
                    help="after each logits-on leg, one splat_backward_ms_per_view line: rasterize forward vs backward")
    ap.add_argument("--geometry", action="store_true",
                    help="with --backward: one splat_geometry_backward_ms_per_view line: the fused geometry backward vs the backward")
    ap.add_argument("--loss", action="store_true",
                    help="one splat_loss_step_ms line per configuration: a refinement step, fused (replay, saved) vs composite")
    args = ap.parse_args(argv)
    if args.geometry and not args.backward:
        ap.error("--geometry needs --backward")
    dev = torch.device("cuda:0")
    for G in args.g:
        g = sg.make_gaussians(G, seed=0)
        t = {k: torch.from_numpy(g[k]).to(dev) for k in ("means", "quats", "scales", "opacities")}
        lg32 = torch.from_numpy(sg.make_logits(g["classes"], 32, seed=0)).to(dev)
        for size in args.size:
            W, H = (int(v) for v in size.split("x"))
            # the trajectory's later frames (the first ones are a close-up of one wall)
            w2c, K = sg.make_views(args.views * 12, g["room"], W, seed=0)
            w2c = w2c[::12]
            for D in args.d:
                feats = lg32[:, :D].contiguous() if D <= 32 else lg32
                if args.loss:
                    loss_leg(t, feats, G, W, H, w2c[0], K, args)
                    continue
                ws = voxproj_host.SplatWorkspace()
                for lo in args.logits:
                    want = lo == "on"
                    counts = []

                    def full(i):
                        r = voxproj_host.splat_features(t["means"], t["quats"], t["scales"], t["opacities"], feats,
                                                        w2c[i % len(w2c)], K, W, H, want_logits=want, workspace=ws,
                                                        check=False)
                        counts.append(r.n_isect)
                    ms = timed(full, args.steps, args.warmup)
                    caps = {}

                    def proj(i):
                        n = voxproj_host.splat_project(t["means"], t["quats"], t["scales"], t["opacities"],
                                                       w2c[i % len(w2c)], K, W, H, workspace=ws)
                        if i % len(w2c) not in caps:
                            caps[i % len(w2c)] = int(n.item())
                    proj_ms = timed(proj, len(w2c), 0)          # fills caps (one count read per camera, not timed below)
                    proj_ms = timed(lambda i: voxproj_host.splat_project(t["means"], t["quats"], t["scales"], t["opacities"],
                                                                          w2c[0], K, W, H, workspace=ws), args.steps, args.warmup)
                    voxproj_host.splat_project(t["means"], t["quats"], t["scales"], t["opacities"], w2c[0], K, W, H, workspace=ws)
                    raster_ms = timed(lambda i: voxproj_host.splat_rasterize(feats, G, W, H, caps[0], ws, want_logits=want),
                                      args.steps, args.warmup)
                    n_isect = float(np.mean(counts))
                    res = dict(metric="splat_ms_per_view", G=G, D=D, W=W, H=H, logits=want, ms_per_view=round(ms, 4),
                               project_ms=round(proj_ms, 4), raster_ms=round(raster_ms, 4),
                               raster_view0_isect=caps[0], n_isect=int(n_isect),
                               isect_px_per_s=round(caps[0] * 256 / (raster_ms * 1e-3), 1),
                               logits_GBs=round(D * H * W * 4 / (raster_ms * 1e-3) / 1e9, 2) if want else None,
                               views=len(w2c), steps=args.steps, warmup=args.warmup)
                    print(json.dumps(res), flush=True)
                    if args.backward and want:
                        backward_leg(t, feats, G, W, H, w2c[0], K, ws, caps[0], args)


def backward_leg(t, feats, G, W, H, vm, K, ws, cap, args):
    """--backward: vp_splat_rasterize on view 0 (logits and alpha written) against vp_splat_rasterize_backward with a
    random upstream gradient on both outputs, same event timing."""
    D = int(feats.shape[1])
    gen = torch.Generator(feats.device).manual_seed(0)
    g_logits = torch.randn((D, H, W), device=feats.device, generator=gen)
    g_alpha = torch.randn((H, W), device=feats.device, generator=gen)
    bws = voxproj_host.SplatWorkspace()
    voxproj_host.splat_project(t["means"], t["quats"], t["scales"], t["opacities"], vm, K, W, H, workspace=ws)
    fwd_ms = timed(lambda i: voxproj_host.splat_rasterize(feats, G, W, H, cap, ws, want_logits=True, want_alpha=True),
                   args.steps, args.warmup)
    bwd_ms = timed(lambda i: voxproj_host.splat_rasterize_backward(feats, G, W, H, cap, ws, g_logits, g_alpha,
                                                                   bwd_workspace=bws), args.steps, args.warmup)
    res = dict(metric="splat_backward_ms_per_view", G=G, D=D, W=W, H=H, raster_fwd_ms=round(fwd_ms, 4),
               raster_bwd_ms=round(bwd_ms, 4), bwd_over_fwd=round(bwd_ms / fwd_ms, 2), n_isect=cap,
               bwd_scratch_MB=round(bws.capacity() / 2 ** 20, 1), steps=args.steps, warmup=args.warmup)
    print(json.dumps(res), flush=True)
    if args.geometry:
        gws = voxproj_host.SplatWorkspace()
        old = lambda i: voxproj_host.splat_rasterize_backward(feats, G, W, H, cap, ws, g_logits, g_alpha,  # noqa: E731
                                                              bwd_workspace=bws)
        new = lambda i: voxproj_host.splat_rasterize_backward_geometry(  # noqa: E731
            t["means"], t["quats"], t["scales"], feats, vm, K, W, H, cap, ws, g_logits, g_alpha, bwd_workspace=gws)
        # alternated twice: the two readings of each show the run-to-run spread next to the ratio
        ms = [timed(fn, args.steps, args.warmup) for fn in (old, new, old, new)]
        bwd, geo = min(ms[0], ms[2]), min(ms[1], ms[3])
        res = dict(metric="splat_geometry_backward_ms_per_view", G=G, D=D, W=W, H=H, raster_bwd_ms=round(bwd, 4),
                   geometry_bwd_ms=round(geo, 4), geometry_over_bwd=round(geo / bwd, 3),
                   raster_bwd_ms_runs=[round(ms[0], 4), round(ms[2], 4)], geometry_bwd_ms_runs=[round(ms[1], 4), round(ms[3], 4)],
                   n_isect=cap, geometry_scratch_MB=round(gws.capacity() / 2 ** 20, 1), steps=args.steps, warmup=args.warmup)
        print(json.dumps(res), flush=True)


def loss_leg(t, feats, G, W, H, vm, K, args):
    """--loss: one refinement step (loss forward + backward in the per-Gaussian logits) on one view, three arms."""
    import splat_autograd
    D = int(feats.shape[1])
    dev = feats.device
    ref = voxproj_host.splat_features(t["means"], t["quats"], t["scales"], t["opacities"], feats, vm, K, W, H, want_alpha=True,
                                      check=False)
    target = torch.where(ref.alpha > 0.5, ref.labels, torch.full_like(ref.labels, -1))
    weight = ref.confidence.clone()
    mask = (target >= 0).reshape(-1)
    tl, wl = target.reshape(-1)[mask].long(), weight.reshape(-1)[mask]
    n_isect = ref.n_isect
    del ref
    param = feats.clone().requires_grad_()

    def fused(keep):
        def fn(i):
            param.grad = None
            loss = splat_autograd.splat_cross_entropy(t["means"], t["quats"], t["scales"], t["opacities"], param, vm, K, W, H,
                                                      target, weight, keep_logits=keep, check=False)[0]
            loss.backward()
        return fn

    def composite(i):
        param.grad = None
        lg = splat_autograd.splat_features(t["means"], t["quats"], t["scales"], t["opacities"], param, vm, K, W, H,
                                           check=False)[0]
        ce = torch.nn.functional.cross_entropy(lg.reshape(D, -1).T[mask], tl, reduction="none")
        ((ce * wl).sum() / wl.sum()).backward()

    arms = (("replay", fused(False)), ("saved", fused(True)), ("composite", composite))
    ms = {k: [] for k, _ in arms}
    peak = {}
    for rnd in range(2):                               # alternated twice: the two readings show the run-to-run spread
        for k, fn in arms:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            ms[k].append(timed(fn, args.steps, args.warmup))
            peak[k] = torch.cuda.max_memory_allocated() - base
    best = {k: min(v) for k, v in ms.items()}
    res = dict(metric="splat_loss_step_ms", G=G, D=D, W=W, H=H, n_isect=n_isect,
               replay_ms=round(best["replay"], 4), saved_ms=round(best["saved"], 4), composite_ms=round(best["composite"], 4),
               replay_ms_runs=[round(v, 4) for v in ms["replay"]], saved_ms_runs=[round(v, 4) for v in ms["saved"]],
               composite_ms_runs=[round(v, 4) for v in ms["composite"]],
               best_fused_over_composite=round(min(best["replay"], best["saved"]) / best["composite"], 3),
               replay_peak_MB=round(peak["replay"] / 2 ** 20, 1), saved_peak_MB=round(peak["saved"] / 2 ** 20, 1),
               composite_peak_MB=round(peak["composite"] / 2 ** 20, 1), two_images_MB=round(2 * D * H * W * 4 / 2 ** 20, 1),
               valid_pixels=int(mask.sum()), steps=args.steps, warmup=args.warmup)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
