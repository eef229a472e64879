"""Rendering wide per-Gaussian rows into one view (vp_splat_render) against what the library could do before it:
vp_splat_rasterize once per 64 channels (fp32 rows, planar fp32 logits), plus the conversion of every [64,H,W] fp32 block
into the channels-last fp16 image.  The scene of tools/bench_lift.py: --g Gaussians of synthetic_gaussians.make_gaussians,
one WxH view of the trajectory, C channels of seeded noise as fp16 and as fp32 rows.  One JSON line:

  wide_f16_ms        vp_splat_render(sorted = 1), fp16 rows -> fp16 [H,W,C], on a workspace that is already sorted; HIP
                     events around --steps calls after --warmup, the arms alternated twice, the best of each kept
  wide_f32_ms        the same with fp32 rows
  wide_f32out_ms     fp16 rows -> fp32 [H,W,C]
  wide_sort_ms       vp_splat_render(sorted = 0) directly after vp_splat_project, the projection's time subtracted: the
                     render with its one sort, what the baseline's first call also pays
  baseline_ms        per 64 channels: vp_splat_rasterize(want_logits) on fp32 rows[:, c:c+64], then
                     out[:, :, c:c+64] = logits.permute(1, 2, 0).half().  Every vp_splat_rasterize call sorts (the entry point
                     has no sorted flag), so sort_ms is reported beside it and baseline_less_sorts_ms = baseline - (C/64 - 1)
                     sorts is the comparator had it sorted once
  convert_ms         the baseline's conversions alone
  max_diff_over_max  largest |wide fp32 - baseline fp32| over max |rows|; asserted <= 1e-5 before anything is timed
  out_write_ms_at    W*H*C*2 bytes at --hbm_gbs (writing the fp16 image once)

python tools/bench_render_wide.py [--steps K] [--warmup W] [--g 200000] [--size 1600x1067] [--c 512] [--hbm_gbs 4000]"""
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

MAX_DIFF = 1e-5


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--g", type=int, default=200000)
    ap.add_argument("--size", default="1600x1067")
    ap.add_argument("--c", type=int, default=512)
    ap.add_argument("--hbm_gbs", type=float, default=4000.0, help="the streaming rate the image's write is compared with")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    G, C = args.g, args.c
    W, H = (int(v) for v in args.size.split("x"))
    g = sg.make_gaussians(G, seed=0)
    t = {k: torch.from_numpy(g[k]).to(dev) for k in ("means", "quats", "scales", "opacities")}
    w2c, K = sg.make_views(8 * 12, g["room"], W, seed=0)       # view 0 of bench_splat.py
    vm = w2c[0]
    gen = torch.Generator(dev).manual_seed(0)
    rows16 = torch.randn((G, C), device=dev, generator=gen, dtype=torch.float32).to(torch.float16)
    rows32 = rows16.float()                                     # the same values: the arms render the same image
    ws = voxproj_host.SplatWorkspace()

    def project(i=0):
        return voxproj_host.splat_project(t["means"], t["quats"], t["scales"], t["opacities"], vm, K, W, H, workspace=ws)

    cap = int(project().item())
    out16 = torch.empty((H, W, C), device=dev, dtype=torch.float16)
    out32 = torch.empty((H, W, C), device=dev, dtype=torch.float32)
    base16 = torch.empty((H, W, C), device=dev, dtype=torch.float16)
    voxproj_host.splat_rasterize(rows32[:, :1], G, W, H, cap, ws, want_confidence=False)     # the sort the sorted arms start from

    def wide(rows, out, srt=True):
        return lambda i: voxproj_host.splat_render(rows, G, W, H, cap, ws, out=out, sorted=srt, check=False)

    def convert(logits, c0):
        base16[:, :, c0:c0 + logits.shape[0]] = logits.permute(1, 2, 0).half()

    def baseline(i, keep=None):
        for c0 in range(0, C, 64):
            logits = voxproj_host.splat_rasterize(rows32[:, c0:c0 + 64], G, W, H, cap, ws, want_logits=True,
                                                  want_confidence=False)[3]
            convert(logits, c0)
            if keep is not None:
                keep[:, :, c0:c0 + 64] = logits.permute(1, 2, 0)

    old32 = torch.empty((H, W, C), device=dev, dtype=torch.float32)
    wide(rows16, out32)(0)
    baseline(0, keep=old32)
    torch.cuda.synchronize()
    diff = float((out32 - old32).abs().max()) / float(rows32.abs().max())
    # both arms hold every element to 1e-4 of the channel's largest row value (their tests' bound); two results further
    # apart than a tenth of that mean one of them is wrong, and then no timing line is printed
    assert diff <= MAX_DIFF, f"wide render and comparator differ by {diff:.3e} of max |rows| (limit {MAX_DIFF:.0e})"
    del old32
    arms = (wide(rows16, out16), wide(rows32, out16), baseline)
    ms = [timed(fn, args.steps, args.warmup) for fn in arms + arms]
    best = [min(ms[k], ms[k + len(arms)]) for k in range(len(arms))]
    f32out_ms = timed(wide(rows16, out32), args.steps, args.warmup)
    blk = torch.empty((min(64, C), H, W), device=dev)
    conv_ms = timed(lambda i: [convert(blk, c0) for c0 in range(0, C, 64)], args.steps, args.warmup)
    one_ms = timed(lambda i: voxproj_host.splat_rasterize(rows32[:, :1], G, W, H, cap, ws, want_confidence=False), args.steps,
                   args.warmup)

    def wide_sort(i):
        project()
        wide(rows16, out16, srt=False)(i)
    sort_ms = timed(wide_sort, args.steps, args.warmup)
    proj_ms = timed(project, args.steps, args.warmup)
    sort_only = max(sort_ms - proj_ms - best[0], 0.0)
    n_calls = (C + 63) // 64
    res = dict(metric="splat_render_wide_ms_per_view", G=G, C=C, W=W, H=H, n_isect=cap, wide_f16_ms=round(best[0], 3),
               wide_f32_ms=round(best[1], 3), baseline_ms=round(best[2], 3),
               baseline_over_wide_f16=round(best[2] / best[0], 3), baseline_over_wide_f32=round(best[2] / best[1], 3),
               wide_f32out_ms=round(f32out_ms, 3), wide_sort_ms=round(sort_ms - proj_ms, 3), project_ms=round(proj_ms, 3),
               sort_ms=round(sort_only, 3), baseline_less_sorts_ms=round(best[2] - (n_calls - 1) * sort_only, 3),
               rasterize_1ch_ms=round(one_ms, 3), convert_ms=round(conv_ms, 3),
               runs_ms=[round(v, 3) for v in ms], max_diff_over_max=diff, out_bytes=W * H * C * 2,
               out_write_ms_at=round(W * H * C * 2 / (args.hbm_gbs * 1e9) * 1e3, 3), hbm_gbs=args.hbm_gbs,
               passes=(C + 63) // 64 if C > 16 else 1, steps=args.steps, warmup=args.warmup)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
