"""Fit the appearance (and, on request, the opacities and geometry) of a 3DGS point cloud to its photographs with the
photometric loss of the reference's training loop, (1 - lambda) L1 + lambda (1 - SSIM) (train_unified_lift.py:401-416,
utils/loss_utils.py:15-71), every view one fused call (splat_autograd.splat_photometric: no torch pass over an image).

  fit_gaussian_appearance.py --gaussians_ply point_cloud.ply --cam_params camera_params.json --images_dir DIR --out REFINED.ply
      [--views NAME ...] [--max_images N] [--downsample_factor F] [--principal_point center|camera]
      [--train colors,opacities,scales,quats,means] [--steps 200] [--views_per_step 4] [--lambda_dssim 0.2]
      [--lr_colors 0.01] [--lr_opacities 0.05] [--lr_scales 0.005] [--lr_quats 0.001] [--lr_means 0.00016] [--seed 0]
      [--densify_interval 0] [--densify_from 500] [--densify_until 15000] [--densify_grad_threshold 0.0002]
      [--percent_dense 0.01] [--min_opacity 0.005] [--opacity_reset_interval 0] [--max_screen_size 0] [--scene_extent E]
      [--sh_degree 0] [--sh_degree_interval 1000] [--lr_sh_rest LR] [--report REPORT.json]

With --sh_degree 0 (the default) appearance is one view-independent colour row per Gaussian: it starts at
max(0, 0.5 + 0.28209479 f_dc), the reference's degree-0 colour, is trained as a row, and is written back as
f_dc = (c - 0.5) / 0.28209479; f_rest_* fields are then neither read nor written.  With --sh_degree D in 1 .. 3 appearance is
the reference's view-dependent colour, spherical harmonics up to degree D evaluated per Gaussian and view
(splat_autograd.sh_colors in front of splat_photometric): ``colors`` in --train then means the raw coefficients f_dc [N,3] and
f_rest [N,Kr,3].  f_rest is read from the ply (its degree must be >= D; the whole width is kept) or starts at zeros of
degree D when the ply has none.  f_dc trains at --lr_colors / 0.28209479, the same step in colour units as the colour row,
f_rest at --lr_sh_rest (default: a twentieth of that, the reference's feature_lr / 20).  The active degree is
active_sh_degree(step): min(D, step // --sh_degree_interval), the reference's oneupSHdegree every 1000 iterations; a ply that
brought its own f_rest starts at D, as the reference's load_ply does.  The numbers before and after are rendered at the degree
reached, the output ply carries f_rest_*, and densification moves f_rest and its Adam moments with the other arrays.
There is no background colour.  --train picks the parameters (default: colors).  Opacities and
scales are trained through the ply's raw parametrisation (sigmoid, exp) in torch, quaternions raw (the splatter normalises
them), means as they are.  Without densification a field that is not trained is written back bit for bit.

Adaptive density control (the reference's train_unified_lift.py:463-473, scene/gaussian_model.py:399-608) is off by default.
--densify_interval K turns it on: every view's backward adds its screen-space gradient norms to the statistics
(vp_densify_accumulate behind splat_photometric), and every K steps after --densify_from and up to --densify_until one plan
(vp_densify_plan) clones the small Gaussians whose mean gradient reaches --densify_grad_threshold, splits the large ones
(larger than --percent_dense x extent) into two children and prunes those below --min_opacity; with --max_screen_size S > 0
and once the step is past --opacity_reset_interval it also prunes Gaussians wider than S pixels in some view or larger than
0.1 x extent.  The extent is --scene_extent, by default 1.1 x the largest distance of a training camera from their mean.
All five arrays are then resampled in their raw parametrisation (vp_densify_rows, vp_densify_split with the seed
(--seed, step)), trained or not; Adam's moments follow (kept rows bit for bit, new rows zero) and the statistics start over.
--opacity_reset_interval R sets raw opacity = min(raw, logit(0.01)) every R steps and zeroes that parameter's moments.

Images are paired with the cameras by name, the camera's file extension dropped: DIR/<name>.png / .jpg / .jpeg through PIL
(8-bit RGB, / 255; resized to the render size when it differs), or DIR/<name>.npy, f32 [3,H,W] at the render size.

Optimisation: torch Adam with one learning rate per parameter; each step draws --views_per_step views with a seeded
generator and takes the mean of their losses.  Before and after, the mean loss, PSNR, SSIM and L1 over all views are
printed, computed with voxproj_host.photo_loss(evaluate_only=True); --report writes them per view as JSON.  Every kernel on
the path is deterministic, so two runs with the same arguments write byte-identical files.
Runs on the GPU only; there is no CPU path.
"""
import argparse
import json
import os

import numpy as np
import torch

import gaussian_views

SH_C0 = 0.28209479177387814
PARAMS = ("colors", "opacities", "scales", "quats", "means")
IMAGE_EXTS = (".png", ".jpg", ".jpeg", ".PNG", ".JPG", ".JPEG")


def colors_from_dc(f_dc):
    """max(0, 0.5 + C0 f_dc): the reference's colour of a degree-0 Gaussian."""
    return np.maximum(0.5 + SH_C0 * np.asarray(f_dc, np.float64), 0.0).astype(np.float32)


def dc_from_colors(colors):
    return ((np.asarray(colors, np.float64) - 0.5) / SH_C0).astype(np.float32)


def active_sh_degree(step, max_degree, interval, start=0):
    """The SH degree in use at training step ``step`` (1-based; 0 = before the first): one degree more every ``interval``
    steps from ``start``, ``max_degree`` at the most (the reference's oneupSHdegree at iteration % 1000 == 0)."""
    if step < 0 or max_degree < 0 or interval < 1 or not 0 <= start <= max_degree:
        raise ValueError(f"active_sh_degree: step {step}, max_degree {max_degree}, interval {interval}, start {start}")
    return min(int(max_degree), int(start) + int(step) // int(interval))


def load_image(images_dir, name, W, H):
    """f32 [3,H,W] in [0, 1] of the view ``name`` (a camera name; its extension is dropped)."""
    stem = os.path.splitext(name)[0]
    npy = os.path.join(images_dir, stem + ".npy")
    if os.path.exists(npy):
        a = np.load(npy)
        if a.shape != (3, H, W):
            raise ValueError(f"{npy}: shape {a.shape}, but the view renders at [3, {H}, {W}]")
        return np.ascontiguousarray(a, dtype=np.float32)
    for ext in IMAGE_EXTS:
        p = os.path.join(images_dir, stem + ext)
        if os.path.exists(p):
            from PIL import Image
            with Image.open(p) as im:
                im = im.convert("RGB")
                if im.size != (W, H):
                    im = im.resize((W, H), Image.BICUBIC)
                a = np.asarray(im, dtype=np.uint8)
            return np.ascontiguousarray(a.transpose(2, 0, 1).astype(np.float32) / 255.0)
    raise FileNotFoundError(f"no image for view {name} in {images_dir} ({stem}.npy or {stem}{{.png,.jpg,.jpeg}})")


def build_parser():
    ap = argparse.ArgumentParser(description="Fit Gaussian colours / opacities / geometry to photographs (fused L1 + D-SSIM)")
    gaussian_views.add_view_arguments(ap, images_help="<name>.png / .jpg / .npy per view: the photographs")
    ap.add_argument("--out", required=True, help="the refined .ply")
    ap.add_argument("--train", default="colors", help="comma-separated subset of " + ",".join(PARAMS))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--views_per_step", type=int, default=4)
    ap.add_argument("--lambda_dssim", type=float, default=0.2)
    ap.add_argument("--lr_colors", type=float, default=0.01)
    ap.add_argument("--lr_opacities", type=float, default=0.05)
    ap.add_argument("--lr_scales", type=float, default=0.005)
    ap.add_argument("--lr_quats", type=float, default=0.001)
    ap.add_argument("--lr_means", type=float, default=0.00016)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--densify_interval", type=int, default=0, help="densify every K steps (0: off)")
    ap.add_argument("--densify_from", type=int, default=500, help="first densification after this step")
    ap.add_argument("--densify_until", type=int, default=15000, help="no statistics or densification from this step on")
    ap.add_argument("--densify_grad_threshold", type=float, default=0.0002)
    ap.add_argument("--percent_dense", type=float, default=0.01)
    ap.add_argument("--min_opacity", type=float, default=0.005)
    ap.add_argument("--opacity_reset_interval", type=int, default=0, help="reset opacities every R steps (0: never)")
    ap.add_argument("--max_screen_size", type=float, default=0.0, help="prune Gaussians wider than this in pixels (0: off)")
    ap.add_argument("--scene_extent", type=float, default=None, help="default: the extent of the training cameras")
    ap.add_argument("--report", default="", help="write the per-view numbers before and after as JSON")
    return ap


def add_sh_arguments(ap):
    """The view-dependent colour's options.  build_parser() stays the option set that tests/golden/cli_parsers.json records
    for this tool; the command line is build_cli(): that set and these."""
    ap.add_argument("--sh_degree", type=int, default=0, help="spherical-harmonics degree of the colour, 0 .. 3 (0: one colour row)")
    ap.add_argument("--sh_degree_interval", type=int, default=1000, help="one SH degree more every this many steps")
    ap.add_argument("--lr_sh_rest", type=float, default=None, help="default: (--lr_colors / 0.28209479) / 20")
    return ap


def build_cli():
    return add_sh_arguments(build_parser())


def check_densify_args(ap, args):
    """Refuse bad values of the densification options (ap.error: exit status 2)."""
    if args.densify_interval < 0 or args.opacity_reset_interval < 0:
        ap.error("--densify_interval and --opacity_reset_interval must be >= 0")
    if args.densify_from < 0 or args.densify_from >= args.densify_until:
        ap.error("need 0 <= --densify_from < --densify_until")
    if not args.densify_grad_threshold > 0.0 or not args.percent_dense > 0.0 or not args.min_opacity > 0.0:
        ap.error("--densify_grad_threshold, --percent_dense and --min_opacity must be > 0")
    if not args.max_screen_size >= 0.0 or (args.scene_extent is not None and not args.scene_extent > 0.0):
        ap.error("--max_screen_size must be >= 0 and --scene_extent > 0")


def main(argv=None):
    import gaussian_ply
    import splat_autograd
    import voxproj_host
    ap = build_cli()
    args = ap.parse_args(argv)
    train = tuple(t for t in (s.strip() for s in args.train.split(",")) if t)
    if not train or any(t not in PARAMS for t in train):
        ap.error(f"--train takes a comma-separated subset of {','.join(PARAMS)}")
    if args.steps < 0 or args.views_per_step < 1 or not 0.0 <= args.lambda_dssim <= 1.0:
        ap.error("--steps must be >= 0, --views_per_step >= 1 and --lambda_dssim in [0, 1]")
    check_densify_args(ap, args)
    if not 0 <= args.sh_degree <= gaussian_ply.SH_MAX_DEGREE or args.sh_degree_interval < 1:
        ap.error(f"--sh_degree must be in 0 .. {gaussian_ply.SH_MAX_DEGREE} and --sh_degree_interval >= 1")
    if args.lr_sh_rest is not None and not args.lr_sh_rest >= 0.0:
        ap.error("--lr_sh_rest must be >= 0")
    densify_on = args.densify_interval > 0
    sh_on = args.sh_degree > 0
    dev = gaussian_views.require_gpu("fit_gaussian_appearance")
    ply = gaussian_ply.read_gaussian_ply(args.gaussians_ply, want_dc=True, want_raw=True, want_sh=sh_on)
    N = int(ply["means"].shape[0])
    sh_start = 0
    if sh_on:
        kr = int(ply["f_rest"].shape[1])
        if kr == 0:
            ply["f_rest"] = np.zeros((N, (args.sh_degree + 1) ** 2 - 1, 3), np.float32)
        elif gaussian_ply.sh_degree_of_width(kr) < args.sh_degree:
            raise ValueError(f"{args.gaussians_ply} carries SH degree {gaussian_ply.sh_degree_of_width(kr)}, below --sh_degree "
                             f"{args.sh_degree}")
        else:
            sh_start = args.sh_degree

    def degree_at(step):
        return active_sh_degree(step, args.sh_degree, args.sh_degree_interval, sh_start)
    names, view = gaussian_views.open_views(args, images_dir="")      # the size is the camera's, not the photograph's
    if not names:
        raise ValueError("no views to train on")
    views = []
    for name in names:
        vm, K, W, H = view(name)
        views.append((vm, K, W, H, torch.from_numpy(load_image(args.images_dir, name, W, H)).to(dev)))

    # the parameters in the ply's own parametrisation; what is not trained stays a constant
    raw = dict(colors=colors_from_dc(ply["f_dc"]), opacities=ply["opacity_logits"], scales=ply["log_scales"], quats=ply["rots"],
               means=ply["means"])
    if sh_on:                             # the colour row gives way to the raw coefficients
        del raw["colors"]
        raw.update(f_dc=ply["f_dc"], f_rest=ply["f_rest"])
        lr_dc = args.lr_colors / SH_C0
        args.lr_f_dc, args.lr_f_rest = lr_dc, args.lr_sh_rest if args.lr_sh_rest is not None else lr_dc / 20.0
        trained = tuple(n for k in train for n in (("f_dc", "f_rest") if k == "colors" else (k,)))
    else:
        trained = train
    p = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in raw.items()}
    for k in trained:
        p[k] = torch.nn.Parameter(p[k])
    fixed = {k: torch.from_numpy(ply[k]).to(dev) for k in ("opacities", "scales", "quats")}

    def activated():
        op = torch.sigmoid(p["opacities"]) if "opacities" in train else fixed["opacities"]
        sc = torch.exp(p["scales"]) if "scales" in train else fixed["scales"]
        qt = p["quats"] if "quats" in train else fixed["quats"]
        return p["means"], qt, sc, op, None if sh_on else p["colors"]

    def colors_of(tensors, vm, degree):
        """The colour rows of one view: the row itself, or the SH expansion seen from the view's camera."""
        if not sh_on:
            return tensors
        return tensors[:4] + (splat_autograd.sh_colors(p["f_dc"], p["f_rest"], tensors[0], vm, degree),)

    def view_loss(v, tensors, stats=None, stats_scale=1.0, degree=0):
        vm, K, W, H, target = v
        return splat_autograd.splat_photometric(*colors_of(tensors, vm, degree), vm, K, W, H, target,
                                                lambda_dssim=args.lambda_dssim, check=False, densify_stats=stats,
                                                stats_scale=stats_scale)

    def densify(step, opt, stats):
        """One plan, every array and Adam moment resampled by it: the [FIT] record of the densification."""
        with torch.no_grad():
            screen = args.max_screen_size if step > args.opacity_reset_interval else 0.0
            plan = voxproj_host.densify_plan(stats, torch.exp(p["scales"]), torch.sigmoid(p["opacities"]),
                                             grad_threshold=args.densify_grad_threshold,
                                             size_threshold=float(np.float32(args.percent_dense * extent)),
                                             min_opacity=args.min_opacity, max_screen_size=screen,
                                             max_world_size=float(np.float32(0.1 * extent)))
            new = plan.resample({k: (p[k], "copy") for k in raw if k not in ("means", "scales")})
            new["means"], new["scales"] = plan.split_geometry(p["means"], p["quats"], p["scales"], (args.seed, step))
            old = {k: p[k] for k in trained}
            for k in raw:
                p[k] = torch.nn.Parameter(new[k]) if k in trained else new[k]
            voxproj_host.resample_adam(opt, old, {k: p[k] for k in trained}, plan)
            fixed.update(opacities=torch.sigmoid(p["opacities"]).detach(), scales=torch.exp(p["scales"]).detach(),
                         quats=p["quats"].detach())
            stats.reset(plan.n_out)
        rec = dict(step=step, n_before=plan.n, n_after=plan.n_out, kept=plan.kept, clones=plan.clones, split=plan.split,
                   pruned=plan.n - plan.kept - plan.split)
        print(f"[FIT] densify at step {step}: {rec['n_before']} -> {rec['n_after']} Gaussians (kept {rec['kept']}, clones "
              f"{rec['clones']}, split sources {rec['split']}, pruned {rec['pruned']})")
        return rec

    def reset_opacity(opt):
        """raw opacity = min(raw, logit(0.01)); that parameter's moments start over."""
        with torch.no_grad():
            p["opacities"].clamp_(max=float(np.log(0.01 / 0.99)))
            st = opt.state.get(p["opacities"]) if "opacities" in trained else None
            for key in ("exp_avg", "exp_avg_sq"):
                if st and key in st:
                    st[key].zero_()
            fixed["opacities"] = torch.sigmoid(p["opacities"]).detach()

    def evaluate(degree=0):
        rows = []
        with torch.no_grad():
            tensors = activated()
            for name, (vm, K, W, H, target) in zip(names, views):
                m, q, s, o, c = colors_of(tensors, vm, degree)
                r = voxproj_host.splat_features(m, q, s, o, c, vm, K, W, H, want_logits=True, want_alpha=False,
                                                want_confidence=False, check=False)
                stats, _, _ = voxproj_host.photo_loss(r.logits, target, evaluate_only=True)
                n = 3 * W * H
                row = voxproj_host.image_metrics(stats, n)
                row["loss"] = (1.0 - args.lambda_dssim) * row["l1"] + args.lambda_dssim * (1.0 - row["ssim"])
                row["view"] = name
                rows.append(row)
        mean = {k: float(np.mean([r[k] for r in rows])) for k in ("loss", "psnr", "ssim", "l1")}
        return mean, rows

    def line(tag, m):
        print(f"[FIT] {tag}: mean loss {m['loss']:.6f}, PSNR {m['psnr']:.3f} dB, SSIM {m['ssim']:.5f}, L1 {m['l1']:.6f}")

    before, rows_before = evaluate(degree_at(0))
    print(f"[FIT] {len(views)} view(s), {N} Gaussians, training {','.join(train)}, lambda_dssim {args.lambda_dssim}")
    if sh_on:
        print(f"[FIT] SH degree {args.sh_degree} (f_rest [{N}, {int(p['f_rest'].shape[1])}, 3]), degree {degree_at(0)} before the "
              f"first step, one more every {args.sh_degree_interval} step(s); lr f_dc {args.lr_f_dc:.6g}, f_rest {args.lr_f_rest:.6g}")
    line("before", before)
    opt = torch.optim.Adam([dict(params=[p[k]], lr=getattr(args, "lr_" + k)) for k in trained])
    gen = torch.Generator().manual_seed(args.seed)
    k = min(args.views_per_step, len(views))
    extent = args.scene_extent if args.scene_extent is not None else voxproj_host.camera_extent([v[0] for v in views])
    stats = voxproj_host.DensifyStats(N, dev, want_radius=args.max_screen_size > 0.0) if densify_on else None
    densifications = []
    for step in range(1, args.steps + 1):
        pick = gaussian_views.draw_indices(len(views), k, gen)
        opt.zero_grad(set_to_none=True)
        tensors = activated()
        loss = 0
        collect = stats if densify_on and step < args.densify_until else None
        for i in pick:
            loss = loss + view_loss(views[i], tensors, collect, float(k), degree_at(step))[0] / k
        loss.backward()
        opt.step()
        if collect is not None and step > args.densify_from and step % args.densify_interval == 0:
            opt.zero_grad(set_to_none=True)
            densifications.append(densify(step, opt, stats))
        if args.opacity_reset_interval > 0 and step % args.opacity_reset_interval == 0:
            reset_opacity(opt)
    after, rows_after = evaluate(degree_at(args.steps))
    line(f"after {args.steps} step(s)", after)
    n_after = int(p["means"].shape[0])
    if densify_on:
        print(f"[FIT] {N} -> {n_after} Gaussians in {len(densifications)} densification(s), extent {extent:.6g}")
    out = {k: p[k].detach().cpu().numpy() for k in raw}
    if sh_on:
        gaussian_ply.write_gaussian_ply(args.out, out["means"], out["opacities"], out["scales"], out["quats"], f_dc=out["f_dc"],
                                        f_rest=out["f_rest"])
    else:
        f_dc = dc_from_colors(out["colors"]) if "colors" in train or densifications else ply["f_dc"]
        gaussian_ply.write_gaussian_ply(args.out, out["means"], out["opacities"], out["scales"], out["quats"], f_dc=f_dc)
    print(f"[FIT] -> {args.out}")
    res = dict(loss_before=before["loss"], loss_after=after["loss"], n_before=N, n_after=n_after)
    for key in ("psnr", "ssim", "l1"):
        res[key + "_before"], res[key + "_after"] = before[key], after[key]
    if sh_on:
        res.update(sh_degree=args.sh_degree, sh_degree_reached=degree_at(args.steps))
    if args.report:
        with open(args.report, "w") as f:
            report = dict(summary=res, train=list(train), steps=args.steps, lambda_dssim=args.lambda_dssim,
                          before=rows_before, after=rows_after, densify=densifications)
            if sh_on:
                report.update(sh_degree=args.sh_degree, sh_degree_reached=degree_at(args.steps))
            json.dump(report, f, indent=1)
    return res


if __name__ == "__main__":
    main()
