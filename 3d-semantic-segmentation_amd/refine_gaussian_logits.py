"""Refine per-Gaussian logits against per-view label maps: the step between ``query_voxel_features.py`` (which writes both
the per-Gaussian logits and the per-view labels) and ``render_semantics_logits.py`` (which renders the logits).

  refine_gaussian_logits.py --gaussians_ply point_cloud.ply --logit_path X.npz --cam_params camera_params.json
      --targets_dir DIR [--views NAME ...] [--max_images N] [--downsample_factor F] [--principal_point center|camera]
      [--weight confidence|none] [--steps 200] [--views_per_step 4] [--lr 0.1] [--seed 0] [--report_miou] --out REFINED.npz
      [--reg3d_weight 0] [--reg3d_k 5] [--reg3d_interval 2] [--reg3d_sample_size 0]

Inputs: the 3DGS point cloud and the .npz of ``query_voxel_features.py gaussians`` ('logits' [N, P], 'prompts'), as
render_semantics_logits.py reads them, with its cameras and image sizes; the targets ``DIR/<name>_labels.npy`` (int16 [H,W],
-1 = no label; any value outside [0, P) is ignored) and, with --weight confidence, the per-pixel weights
``DIR/<name>_confidence.npy`` (f32 [H,W]), both as ``query_voxel_features.py views`` writes them.  A target whose size
differs from the view's render size is an error.

Training: the P real channels of 'logits' (no padding) are the parameters of torch Adam; each step draws --views_per_step
views with a seeded generator and takes the mean of their weighted cross-entropies, each one fused call
(splat_autograd.splat_cross_entropy: no logits image, no gradient image).  Before and after, the mean loss and the share of
labelled pixels whose rendered label agrees with the target are printed over all views; with --report_miou also the mIoU
and fwIoU of the rendered labels against the targets (one confusion over all views, voxproj_host.label_scores).  Every kernel on the path is
deterministic, so two runs with the same arguments write byte-identical logits.

--reg3d_weight W > 0 adds the 3D neighbourhood regulariser (splat_autograd.neighbor_consistency, the reference's loss_cls_3d):
a Gaussian no training view sees is tied to its --reg3d_k - 1 nearest neighbours in space (k counts the Gaussian itself, as
the reference's reg3d_k does).  The neighbour table is built once from the ply's means; on every --reg3d_interval-th step W
times the regulariser (scale 1) is added to the step's loss, over every Gaussian (--reg3d_sample_size 0) or over that many
drawn from the seeded generator.  The regulariser over all Gaussians joins the before / after lines.  With W = 0 no table is
built, no random number is drawn and the output is what it was without these flags.

Output: --out, an .npz with the input's schema: 'labels' int16 [N] (argmax of the refined logits), 'logits' f32 [N, P],
'prompts' (and 'colors' when the input has them), which render_semantics_logits.py --logit_path reads unchanged.
Runs on the GPU only; there is no CPU path.
"""
import argparse
import os

import numpy as np
import torch

import gaussian_views


def load_target(targets_dir, name, W, H, n_classes, weight="confidence"):
    """(target int32 [H,W] with every ignored pixel at -1, weight f32 [H,W] or None) of one view; raises ValueError when a
    file's size is not the render size H x W."""
    path = os.path.join(targets_dir, name + "_labels.npy")
    lab = np.load(path)
    if lab.shape != (H, W):
        raise ValueError(f"{path}: the target is {lab.shape[1] if lab.ndim == 2 else '?'}x{lab.shape[0]} "
                         f"(shape {lab.shape}) but the view renders at {W}x{H}")
    lab = lab.astype(np.int64)
    target = np.where((lab >= 0) & (lab < n_classes), lab, -1).astype(np.int32)
    w = None
    if weight == "confidence":
        wpath = os.path.join(targets_dir, name + "_confidence.npy")
        w = np.load(wpath)
        if w.shape != (H, W):
            raise ValueError(f"{wpath}: the weights have shape {w.shape} but the view renders at {W}x{H}")
        w = np.ascontiguousarray(w, dtype=np.float32)
    return target, w


def save_refined(path, logits, prompts=None, colors=None):
    """The schema of ``query_voxel_features.py gaussians``: labels int16 [N] = argmax, logits f32 [N,P], prompts."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    d = dict(labels=logits.argmax(1).astype(np.int16), logits=logits)
    if prompts is not None:
        d["prompts"] = np.asarray(prompts)
    if colors is not None:
        d["colors"] = np.asarray(colors, dtype=np.uint8)
    np.savez(path, **d)


def build_parser():
    ap = argparse.ArgumentParser(description="Refine per-Gaussian logits against per-view label maps (fused GPU loss)")
    gaussian_views.add_view_arguments(ap)
    ap.add_argument("--logit_path", required=True, help=".npz with 'logits' [N, P] (query_voxel_features.py gaussians)")
    ap.add_argument("--targets_dir", required=True, help="<name>_labels.npy / <name>_confidence.npy per view")
    ap.add_argument("--weight", choices=("confidence", "none"), default="confidence")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--views_per_step", type=int, default=4)
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--report_miou", action="store_true", help="add mIoU / fwIoU against the targets to the before / after lines")
    ap.add_argument("--reg3d_weight", type=float, default=0.0, help="weight of the 3D neighbourhood regulariser (0: off)")
    ap.add_argument("--reg3d_k", type=int, default=5, help="neighbourhood size, the Gaussian itself included (2..16)")
    ap.add_argument("--reg3d_interval", type=int, default=2, help="apply the regulariser on every N-th step")
    ap.add_argument("--reg3d_sample_size", type=int, default=0, help="Gaussians per application (0: every Gaussian)")
    ap.add_argument("--out", required=True, help="the refined .npz")
    return ap


def main(argv=None):
    import splat_autograd
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.steps < 0 or args.views_per_step < 1:
        ap.error("--steps must be >= 0 and --views_per_step >= 1")
    if args.reg3d_weight < 0 or not 2 <= args.reg3d_k <= 16 or args.reg3d_interval < 1 or args.reg3d_sample_size < 0:
        ap.error("--reg3d_weight must be >= 0, --reg3d_k in [2, 16], --reg3d_interval >= 1 and --reg3d_sample_size >= 0")
    dev = gaussian_views.require_gpu("refine_gaussian_logits")
    g = gaussian_views.load_gaussians(args.gaussians_ply, dev)
    d = np.load(args.logit_path)
    if "logits" not in d:
        raise KeyError(f"{args.logit_path}: no 'logits' array")
    raw = np.asarray(d["logits"], dtype=np.float32)
    if raw.ndim != 2 or raw.shape[0] != g["means"].shape[0]:
        raise ValueError(f"{args.logit_path}: logits {raw.shape} for {g['means'].shape[0]} Gaussians")
    P = int(raw.shape[1])
    if not 1 <= P <= 64:
        raise ValueError(f"{args.logit_path}: {P} classes outside [1, 64]")
    names, view = gaussian_views.open_views(args)
    if not names:
        raise ValueError("no views to train on")
    views = []
    for name in names:
        vm, K, W, H = view(name)
        target, w = load_target(args.targets_dir, name, W, H, P, args.weight)
        views.append((vm, K, W, H, torch.from_numpy(target).to(dev), torch.from_numpy(w).to(dev) if w is not None else None))
    param = torch.nn.Parameter(torch.from_numpy(raw).to(dev))
    opt = torch.optim.Adam([param], lr=args.lr)

    def view_loss(v):
        vm, K, W, H, target, w = v
        return splat_autograd.splat_cross_entropy(g["means"], g["quats"], g["scales"], g["opacities"], param, vm, K, W, H,
                                                  target, w, reduction="mean", check=False)

    scores = None
    if args.report_miou:
        import label_metrics
        import voxproj_host
        scores = voxproj_host.LabelScores(P, dev)

    def evaluate():
        with torch.no_grad():
            loss, agree, total = 0.0, 0, 0
            if scores is not None:
                scores.zero_()
            for v in views:
                ce, labels, _, _ = view_loss(v)
                valid = v[4] >= 0
                loss += float(ce)
                agree += int((labels[valid] == v[4][valid]).sum())
                total += int(valid.sum())
                if scores is not None:
                    voxproj_host.label_scores(labels, v[4], P, out=scores)
        m = label_metrics.metrics(scores.numpy()[0]) if scores is not None else None
        return loss / len(views), agree / max(total, 1), total, m

    def miou_text(m):
        if m is None:
            return ""
        fmt = lambda x: "null" if x is None else f"{x:.4f}"  # noqa: E731
        return f", mIoU {fmt(m['miou'])}, fwIoU {fmt(m['fwiou'])}"

    table = None
    if args.reg3d_weight > 0:
        import voxproj_host
        table = voxproj_host.NeighborTable(g["means"], args.reg3d_k)

    def reg3d(sample=None):
        return splat_autograd.neighbor_consistency(param, table, scale=1.0, sample=sample)

    def reg_text(r):
        return "" if r is None else f", reg3d {r:.6f}"

    l0, a0, total, m0 = evaluate()
    r0 = float(reg3d().detach()) if table is not None else None
    print(f"[REFINE] {len(views)} view(s), {total} labelled pixels, {P} classes, {raw.shape[0]} Gaussians")
    print(f"[REFINE] before: mean loss {l0:.6f}, pixel agreement {a0:.4f}{miou_text(m0)}{reg_text(r0)}")
    gen = torch.Generator().manual_seed(args.seed)
    k = min(args.views_per_step, len(views))
    for step in range(args.steps):
        pick = gaussian_views.draw_indices(len(views), k, gen)
        opt.zero_grad(set_to_none=True)
        loss = 0
        for i in pick:
            loss = loss + view_loss(views[i])[0] / k
        if table is not None and step % args.reg3d_interval == 0:
            sample = None
            if 0 < args.reg3d_sample_size < raw.shape[0]:
                sample = torch.randperm(raw.shape[0], generator=gen)[:args.reg3d_sample_size].to(dev)
            loss = loss + args.reg3d_weight * reg3d(sample)
        loss.backward()
        opt.step()
    l1, a1, _, m1 = evaluate()
    r1 = float(reg3d().detach()) if table is not None else None
    print(f"[REFINE] after {args.steps} step(s): mean loss {l1:.6f}, pixel agreement {a1:.4f}{miou_text(m1)}{reg_text(r1)}")
    prompts = d["prompts"] if "prompts" in d else None
    save_refined(args.out, param.detach().cpu().numpy(), prompts, d["colors"] if "colors" in d else None)
    print(f"[REFINE] -> {args.out}")
    res = dict(loss_before=l0, loss_after=l1, agreement_before=a0, agreement_after=a1)
    if scores is not None:
        res.update(miou_before=m0["miou"], miou_after=m1["miou"], fwiou_before=m0["fwiou"], fwiou_after=m1["fwiou"])
    if table is not None:
        res.update(reg3d_before=r0, reg3d_after=r1)
    return res


if __name__ == "__main__":
    main()
