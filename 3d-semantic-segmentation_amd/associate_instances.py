"""Associate per-view instance ids across views: train a code book of global instance labels on the fixed identity rows of
lift_instance_features.py, so that every Gaussian gets one instance id and every view an id map that means the same thing
in all of them.

  associate_instances.py --gaussians_ply point_cloud.ply --cam_params camera_params.json --masks_dir object_mask
      --gauss_feats IDENTITY.pt [--codes 256] [--steps 500] [--lr 5e-4] [--seed 0] [--conf_min 0.2] [--ignore_id -1]
      [--weight_cls 1] [--weight_cluster 1] [--views NAME ...] [--max_images N] [--downsample_factor F]
      [--principal_point center|camera] [--images_dir DIR] --out CODEBOOK.pt [--labels_dir DIR]

Views, cameras, sizes and the pairing of masks with cameras are lift_instance_features.py's (the same helpers of
evaluate_label_maps.py, render_semantics_logits.py and the aggregator; mask value 255 is "no mask").  The rows of
--gauss_feats stay fixed.  The code book B [codes, D] is an fp32 parameter of torch Adam, started uniform in +-1/sqrt(D)
from the seed.  Per step one view is drawn, and:
  1. vp_splat_rasterize renders the rows into the view: the identity image [D,H,W];
  2. vp_proto_contrast with the confidence map's parameters (CONFIDENCE_PARAMS) gives own_prob, the confidence;
  3. vp_codebook_assoc sums the softmax of B . f_p per mask id: the score matrix [256, codes];
  4. voxproj_host.assign_view_ids assigns the view's ids to codes (scipy.optimize.linear_sum_assignment on the host: one
     small device-to-host copy and one host synchronisation per view);
  5. vp_codebook_loss: cross-entropy against the assigned codes and the clustering loss |f_p / |f_p| - B_v| over the pixels
     with own_prob > --conf_min (splat_autograd.codebook_loss); only the code book receives a gradient.
The mean loss over all views is printed before and after.  Every kernel on the path is deterministic, so two runs with the
same arguments write byte-identical files.

Output (--out): codebook f32 [codes, D]; gaussian_ids int32 [N], the argmax of B . row per Gaussian (vp_codebook_assoc on
the rows laid out as an image); views, the names; assign int32 [views, 256], per view the id -> code map (-1: the id does not
occur or received no code).  --labels_dir DIR writes per view <name>_labels.png, an 8-bit image holding the code of every
pixel (the argmax) with 255 where the rendered alpha is below 0.5; evaluate_label_maps.py reads it unchanged (with
--codes 256, code 255 cannot be told from "no label" in such a file).  Runs on the GPU only; there is no CPU path.
"""
import argparse
import io
import math
import os

import torch

import gaussian_views
import lift_gaussian_features as lgf

# the confidence map of the method this follows: the prototype softmax at temperature clip(0.1 spread, 0.1, 1), every id
CONFIDENCE_PARAMS = dict(phi_scale=0.1, phi_min=0.1, phi_max=1.0, min_count=0)
ROW_IMAGE_WIDTH = 4096


def build_parser():
    ap = argparse.ArgumentParser(description="Associate per-view instance ids across views (fused GPU code book kernels)")
    gaussian_views.add_view_arguments(ap, views_help="view names (default: every mask, sorted)")
    ap.add_argument("--masks_dir", required=True, help="per view <name>.png: the 8-bit instance mask")
    ap.add_argument("--gauss_feats", required=True, help="IDENTITY.pt of lift_instance_features.py: one identity row per Gaussian")
    ap.add_argument("--codes", type=int, default=256, help="rows of the code book (1 .. 256)")
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--lr", type=float, default=5e-4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--conf_min", type=float, default=0.2, help="pixels whose confidence is not above it take no part in the loss")
    ap.add_argument("--ignore_id", type=int, default=-1, help="a mask value that takes no part (-1: none)")
    ap.add_argument("--weight_cls", type=float, default=1.0)
    ap.add_argument("--weight_cluster", type=float, default=1.0)
    ap.add_argument("--out", required=True, help="output .pt: codebook, gaussian_ids, views, assign")
    ap.add_argument("--labels_dir", default=None, help="write <name>_labels.png per view: the code of every pixel")
    return ap


def init_codebook(codes, dim, gen):
    """Uniform in +-1/sqrt(dim): what a 1x1 convolution from dim channels starts from by default."""
    return (torch.rand((codes, dim), generator=gen) * 2.0 - 1.0) / math.sqrt(dim)


def gaussian_codes(rows, codebook):
    """int32 [N]: argmax of B . row per Gaussian, through vp_codebook_assoc on the rows laid out as an image."""
    import voxproj_host
    N, D = rows.shape
    W = min(N, ROW_IMAGE_WIDTH)
    H = (N + W - 1) // W
    image = torch.zeros((D, H * W), dtype=torch.float32, device=rows.device)
    image[:, :N] = rows.t()
    ids = torch.zeros((H, W), dtype=torch.int32, device=rows.device)
    _, _, pred, _ = voxproj_host.codebook_assoc(image.reshape(D, H, W), ids, codebook, want_pred=True)
    return pred.reshape(-1)[:N].contiguous()


def save(path, obj):
    """torch.save through a buffer: the archive carries no file name, so equal contents are equal bytes."""
    buf = io.BytesIO()
    torch.save(obj, buf)
    with open(path, "wb") as f:
        f.write(buf.getvalue())


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if not 1 <= args.codes <= 256:
        ap.error(f"--codes must lie in [1, 256], not {args.codes}")
    if args.steps < 0 or not args.lr > 0 or not math.isfinite(args.lr):
        ap.error("--steps must be >= 0 and --lr > 0")
    if not math.isfinite(args.conf_min) or not math.isfinite(args.weight_cls) or not math.isfinite(args.weight_cluster):
        ap.error("--conf_min, --weight_cls and --weight_cluster must be finite")
    import splat_autograd
    import voxproj_host
    dev = gaussian_views.require_gpu("associate_instances")
    g = gaussian_views.load_gaussians(args.gaussians_ply, dev)
    N = int(g["means"].shape[0])
    _, feats, _ = lgf.load_lifted(args.gauss_feats)
    if int(feats.shape[0]) != N or N == 0:
        raise ValueError(f"{args.gauss_feats} has {int(feats.shape[0])} rows, {args.gaussians_ply} has {N} Gaussians")
    D = int(feats.shape[1])
    if not 1 <= D <= 64:
        raise ValueError(f"{args.gauss_feats}: {D} channels outside [1, 64]")
    rows = feats.float().to(dev).contiguous()
    names, load_view = gaussian_views.open_mask_views(args, dev)
    gen = torch.Generator().manual_seed(args.seed)
    param = torch.nn.Parameter(init_codebook(args.codes, D, gen).to(dev))
    opt = torch.optim.Adam([param], lr=args.lr)
    ws, pws, cws = voxproj_host.SplatWorkspace(), voxproj_host.SplatWorkspace(), voxproj_host.SplatWorkspace()

    def view_pass(name):
        """Steps 1 - 5 on one view: (loss, assign int32 [256] numpy, the render)."""
        vm, K, W, H, ids = load_view(name)
        r = voxproj_host.splat_features(g["means"], g["quats"], g["scales"], g["opacities"], rows, vm, K, W, H, want_logits=True,
                                        want_alpha=True, want_confidence=False, workspace=ws, check=False)
        _, _, conf, _ = voxproj_host.proto_contrast(r.logits, ids, None, ignore_id=args.ignore_id, want_own_prob=True,
                                                    workspace=pws, **CONFIDENCE_PARAMS)
        score, id_pixels, _, _ = voxproj_host.codebook_assoc(r.logits, ids, param.detach(), ignore_id=args.ignore_id, workspace=cws)
        assign = voxproj_host.assign_view_ids(score, id_pixels, args.codes)
        loss, _ = splat_autograd.codebook_loss(r.logits, ids, conf, param, torch.from_numpy(assign).to(dev),
                                               weight_cls=args.weight_cls, weight_cluster=args.weight_cluster,
                                               conf_min=args.conf_min, ignore_id=args.ignore_id)
        return loss, assign, r

    def evaluate():
        with torch.no_grad():
            return sum(float(view_pass(name)[0]) for name in names) / len(names)

    l0 = evaluate()
    print(f"[ASSOCIATE] {len(names)} view(s), {N} Gaussians, {D} channels, {args.codes} code(s)")
    print(f"[ASSOCIATE] before: mean loss {l0:.6f}")
    for _ in range(args.steps):
        i = int(torch.randint(0, len(names), (1,), generator=gen))
        opt.zero_grad(set_to_none=True)
        loss, _, _ = view_pass(names[i])
        loss.backward()
        opt.step()
    l1 = evaluate()
    print(f"[ASSOCIATE] after {args.steps} step(s): mean loss {l1:.6f}")
    codebook = param.detach().contiguous()
    assigns = []
    if args.labels_dir:
        os.makedirs(args.labels_dir, exist_ok=True)
    for name in names:
        with torch.no_grad():
            _, assign, r = view_pass(name)
        assigns.append(torch.from_numpy(assign))
        if args.labels_dir:
            from PIL import Image
            everywhere = torch.zeros_like(load_view(name)[4])                  # every pixel valid: its argmax is wanted
            _, _, pred, _ = voxproj_host.codebook_assoc(r.logits, everywhere, codebook, want_pred=True, workspace=cws)
            lab = torch.where(r.alpha < 0.5, torch.full_like(pred, 255), pred).to(torch.uint8).cpu().numpy()
            Image.fromarray(lab, mode="L").save(os.path.join(args.labels_dir, name + "_labels.png"))
    gids = gaussian_codes(rows, codebook)
    save(args.out, {"codebook": codebook.cpu(), "gaussian_ids": gids.cpu(), "views": list(names),
                    "assign": torch.stack(assigns).to(torch.int32)})
    print(f"[ASSOCIATE] -> {args.out}: {int(torch.unique(gids).numel())} code(s) in use over the Gaussians")
    return dict(loss_before=l0, loss_after=l1)


if __name__ == "__main__":
    main()
