"""Lift per-view 2D instance masks onto the Gaussians: train a --dim channel identity row per Gaussian so that the rows
RENDERED into a view fall into one cluster per mask id of that view.  The masks (DEVA, SAM) carry ids that mean nothing
in any other view, so no fixed class can be the target; the loss is the per-view prototype-contrastive loss
(splat_autograd.splat_contrastive: vp_splat_rasterize, vp_proto_contrast, vp_proto_contrast_gradient and the rasterizer's
backward, with the norm regulariser (|f| - 1)^2), and the rows of one object end up alike across views because they are
the same Gaussians.

  lift_instance_features.py --gaussians_ply point_cloud.ply --cam_params camera_params.json --masks_dir object_mask
      [--views NAME ...] [--max_images N] [--downsample_factor F] [--principal_point center|camera] [--images_dir DIR]
      [--dim 16] [--steps 200] [--views_per_step 1] [--samples 32768 | --all_pixels] [--min_count 20] [--ignore_id -1]
      [--weight_contrast 1.0] [--weight_norm 1.0] [--lr 0.01] [--seed 0] --out IDENTITY.pt

Inputs: cameras and sizes are lift_gaussian_features.py's.  --masks_dir holds one 8-bit .png per view (mode L or P),
paired with the cameras by view name the way evaluate_label_maps.py pairs files (<name>.png or <name>_labels.png, here or
in a labels/ subdirectory); a mask of another size is brought to the render size by nearest neighbour.  Value 255 is read
as "no mask" and takes no part, like --ignore_id.
--samples S draws S pixels of the view WITH replacement with a seeded generator and turns the draw into a multiplicity map
with torch.bincount (a pixel drawn twice counts twice); --all_pixels uses every pixel once.  An id takes part in a view when
more than --min_count of its pixels were drawn.

Training: the rows are an fp32 parameter of torch Adam, started from seeded normal values; the Gaussians' geometry stays
fixed.  Each step draws --views_per_step views and takes the mean of their losses.  The mean loss over all views (all
pixels) is printed before and after.  Every kernel on the path is deterministic, so two runs with the same arguments write
byte-identical tensors.

Output (--out): LIFTED.pt's schema -- xyz f32 [N,3], avg_feats f16 [N,dim] (the trained rows), weight f32 [N] (ones),
views -- which ``render_gaussian_features.py`` and ``query_voxel_features.py gaussians --gauss_feats`` read unchanged.
The second half of the method -- a code book of global labels, the linear assignment of every view's ids to it and the
clustering loss -- is ``associate_instances.py``, which trains the code book on the rows this tool wrote and gives one
instance id per Gaussian and id maps that mean the same thing in every view.  Runs on the GPU only; there is no CPU path.
"""
import argparse

import torch

import gaussian_views
import lift_gaussian_features as lgf


def build_parser():
    ap = argparse.ArgumentParser(description="Lift 2D instance masks onto the Gaussians (fused GPU prototype-contrastive loss)")
    gaussian_views.add_view_arguments(ap, views_help="view names (default: every mask, sorted)")
    ap.add_argument("--masks_dir", required=True, help="per view <name>.png: the 8-bit instance mask")
    ap.add_argument("--dim", type=int, default=16, help="channels of the identity rows (1 .. 64)")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--views_per_step", type=int, default=1)
    how = ap.add_mutually_exclusive_group()
    how.add_argument("--samples", type=int, default=32768, help="pixels drawn per view and step, with replacement")
    how.add_argument("--all_pixels", action="store_true", help="use every pixel once instead of drawing --samples")
    ap.add_argument("--min_count", type=int, default=20, help="an id takes part with more than this many drawn pixels")
    ap.add_argument("--ignore_id", type=int, default=-1, help="a mask value that takes no part (-1: none)")
    ap.add_argument("--weight_contrast", type=float, default=1.0)
    ap.add_argument("--weight_norm", type=float, default=1.0)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True, help="output .pt (LIFTED.pt's schema)")
    return ap


def draw_count(n_pixels, samples, gen):
    """The multiplicity map of ``samples`` pixels drawn with replacement: int32 [n_pixels] on the CPU."""
    draw = torch.randint(0, n_pixels, (samples,), generator=gen)
    return torch.bincount(draw, minlength=n_pixels).to(torch.int32)


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if not 1 <= args.dim <= 64:
        ap.error(f"--dim must lie in [1, 64], not {args.dim}")
    if args.steps < 0 or args.views_per_step < 1 or args.samples < 1 or args.min_count < 0:
        ap.error("--steps and --min_count must be >= 0, --views_per_step and --samples >= 1")
    import splat_autograd
    dev = gaussian_views.require_gpu("lift_instance_features")
    g = gaussian_views.load_gaussians(args.gaussians_ply, dev)
    N = int(g["means"].shape[0])
    names, load_view = gaussian_views.open_mask_views(args, dev)
    gen = torch.Generator().manual_seed(args.seed)
    param = torch.nn.Parameter(torch.randn((N, args.dim), generator=gen).to(dev))
    opt = torch.optim.Adam([param], lr=args.lr)

    def view_loss(name, count):
        vm, K, W, H, ids = load_view(name)
        return splat_autograd.splat_contrastive(g["means"], g["quats"], g["scales"], g["opacities"], param, vm, K, W, H, ids, count,
                                                weight_contrast=args.weight_contrast, weight_norm=args.weight_norm,
                                                min_count=args.min_count, ignore_id=args.ignore_id, check=False)

    def evaluate():
        with torch.no_grad():
            total, ids_seen = 0.0, 0
            for name in names:
                loss, stats = view_loss(name, None)
                total += float(loss)
                ids_seen += int(stats[1])
        return total / len(names), ids_seen

    l0, ids_seen = evaluate()
    how = "every pixel" if args.all_pixels else f"{args.samples} pixels drawn"
    print(f"[IDENTITY] {len(names)} view(s), {N} Gaussians, {args.dim} channels, {ids_seen} mask id(s) over the views, {how} per view")
    print(f"[IDENTITY] before: mean loss {l0:.6f}")
    k = min(args.views_per_step, len(names))
    for _ in range(args.steps):
        pick = gaussian_views.draw_indices(len(names), k, gen)
        opt.zero_grad(set_to_none=True)
        loss = 0
        for i in pick:
            _, _, W, H, _ = load_view(names[i])
            count = None if args.all_pixels else draw_count(W * H, args.samples, gen).reshape(H, W).to(dev)
            loss = loss + view_loss(names[i], count)[0] / k
        loss.backward()
        opt.step()
    l1, _ = evaluate()
    print(f"[IDENTITY] after {args.steps} step(s): mean loss {l1:.6f}")
    lgf.save_lifted(args.out, g["means"], param.detach(), torch.ones(N), names)
    print(f"[IDENTITY] -> {args.out}")
    return dict(loss_before=l0, loss_after=l1, ids=ids_seen)


if __name__ == "__main__":
    main()
