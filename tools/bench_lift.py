"""Lifting one fp16 feature map onto the Gaussians (vp_splat_lift) against what the library could do before it: the map
converted to planar fp32 and vp_splat_rasterize_backward (grad_features only) once per 64 channels, conversion included.
The scene of tools/bench_splat.py: --g Gaussians of synthetic_gaussians.make_gaussians, one WxH view of the trajectory,
C fp16 channels of seeded noise.  One JSON line:

  lift_ms            vp_splat_lift(sorted = 1) on the workspace a vp_splat_rasterize call sorted: what the comparator also
                     starts from; HIP events around --steps calls after --warmup, the two arms alternated twice
  lift_sort_ms       vp_splat_lift(sorted = 0) directly after vp_splat_project (the sort included), timed once
  backward8_ms       per 64 channels: feats[:, :, c:c+64] -> planar fp32 [64,H,W], then vp_splat_rasterize_backward
  convert_ms         the conversions alone
  max_rel_diff       largest |lift - comparator| over the per-Gaussian magnitude (both from zero); asserted <= 1e-5 before
                     anything is timed
  map_read_ms_at     W*H*C*2 bytes at --hbm_gbs (reading the map once)
  partial_bytes      n_isect * C * 4: the partial rows written by the sweeps and read by the reduces, over all passes
  scratch_bytes      vp_splat_lift_workspace_bytes(n_isect, C)

python tools/bench_lift.py [--steps K] [--warmup W] [--g 200000] [--size 1600x1067] [--c 512] [--hbm_gbs 4000]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402
import synthetic_gaussians as sg  # noqa: E402
import voxproj_host  # noqa: E402
from bench_splat import timed  # noqa: E402

MAX_REL_DIFF = 1e-5


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--g", type=int, default=200000)
    ap.add_argument("--size", default="1600x1067")
    ap.add_argument("--c", type=int, default=512)
    ap.add_argument("--hbm_gbs", type=float, default=4000.0, help="the streaming rate the map's read is compared with")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    G, C = args.g, args.c
    W, H = (int(v) for v in args.size.split("x"))
    g = sg.make_gaussians(G, seed=0)
    t = {k: torch.from_numpy(g[k]).to(dev) for k in ("means", "quats", "scales", "opacities")}
    w2c, K = sg.make_views(8 * 12, g["room"], W, seed=0)       # view 0 of bench_splat.py
    vm = w2c[0]
    gen = torch.Generator(dev).manual_seed(0)
    feats = torch.randn((H, W, C), device=dev, generator=gen, dtype=torch.float32).to(torch.float16)
    zeros64 = torch.zeros((G, 64), device=dev)
    ws, lw, bws = voxproj_host.SplatWorkspace(), voxproj_host.SplatWorkspace(), voxproj_host.SplatWorkspace()
    cap = int(voxproj_host.splat_project(t["means"], t["quats"], t["scales"], t["opacities"], vm, K, W, H, workspace=ws).item())
    voxproj_host.splat_rasterize(zeros64, G, W, H, cap, ws)            # the sort both arms start from
    sums, wsum = torch.zeros((G, C), device=dev), torch.zeros(G, device=dev)
    old = torch.zeros((G, C), device=dev)

    def lift(i):
        voxproj_host.splat_lift(feats, G, W, H, cap, ws, sums, wsum, sorted=True, lift_workspace=lw)

    def convert(c0):
        return feats[:, :, c0:c0 + 64].permute(2, 0, 1).float().contiguous()

    def backward8(i, keep=False):
        for c0 in range(0, C, 64):
            gl = convert(c0)
            gf, _ = voxproj_host.splat_rasterize_backward(zeros64[:, :gl.shape[0]], G, W, H, cap, ws, gl, None, bwd_workspace=bws,
                                                          want_opacities=False)
            if keep:                        # the comparison below; the timed calls leave the result where the call wrote it
                old[:, c0:c0 + 64] = gf

    lift(0)
    backward8(0, keep=True)
    torch.cuda.synchronize()
    ones = torch.ones((H, W, 1), device=dev, dtype=torch.float16)
    mag = torch.zeros((G, 1), device=dev)
    voxproj_host.splat_lift(ones, G, W, H, cap, ws, mag, None, sorted=True, lift_workspace=lw)
    rel = float(((sums - old).abs().max(dim=1).values / (mag[:, 0] * float(feats.abs().max()) + 1e-30)).max())
    # both arms hold every entry to 1e-4 of its magnitude (their tests' bound); two results further apart than a tenth of
    # that mean one of them is wrong, and then no timing line is printed
    assert rel <= MAX_REL_DIFF, f"lift and comparator differ by {rel:.3e} of the magnitude (limit {MAX_REL_DIFF:.0e})"
    ms = [timed(fn, args.steps, args.warmup) for fn in (lift, backward8, lift, backward8)]
    conv_ms = timed(lambda i: [convert(c0) for c0 in range(0, C, 64)], args.steps, args.warmup)

    def lift_sort(i):
        voxproj_host.splat_project(t["means"], t["quats"], t["scales"], t["opacities"], vm, K, W, H, workspace=ws)
        voxproj_host.splat_lift(feats, G, W, H, cap, ws, sums, wsum, sorted=False, lift_workspace=lw)
    sort_ms = timed(lift_sort, args.steps, args.warmup)
    proj_ms = timed(lambda i: voxproj_host.splat_project(t["means"], t["quats"], t["scales"], t["opacities"], vm, K, W, H,
                                                         workspace=ws), args.steps, args.warmup)
    best_l, best_b = min(ms[0], ms[2]), min(ms[1], ms[3])
    res = dict(metric="splat_lift_ms_per_view", G=G, C=C, W=W, H=H, n_isect=cap, lift_ms=round(best_l, 3),
               backward8_ms=round(best_b, 3), lift_over_backward8=round(best_l / best_b, 4),
               lift_ms_runs=[round(ms[0], 3), round(ms[2], 3)], backward8_ms_runs=[round(ms[1], 3), round(ms[3], 3)],
               convert_ms=round(conv_ms, 3), lift_sort_ms=round(sort_ms - proj_ms, 3), project_ms=round(proj_ms, 3),
               max_rel_diff=rel, map_bytes=W * H * C * 2, map_read_ms_at=round(W * H * C * 2 / (args.hbm_gbs * 1e9) * 1e3, 3),
               hbm_gbs=args.hbm_gbs, partial_bytes=cap * C * 4,
               partial_write_read_ms_at=round(2 * cap * C * 4 / (args.hbm_gbs * 1e9) * 1e3, 3),
               scratch_bytes=voxproj_host.splat_lift_workspace_bytes(cap, C), passes=(C + 63) // 64 if C > 16 else 1,
               steps=args.steps, warmup=args.warmup)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
