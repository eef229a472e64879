"""Score predicted label maps against ground truth: mIoU, fwIoU, pixel accuracy and boundary IoU, counted on the GPU.

  evaluate_label_maps.py --pred DIR --gt DIR --num_classes P [--prompts_npz X.npz] [--views NAME ...]
      [--boundary_ratio 0.02] [--no_boundary] [--resize_pred] --out REPORT.json

Files: both directories (and their ``labels/`` subdirectory, where render_semantics_logits.py puts its maps) are read for
  <name>_labels.npy       integer [H,W], -1 = no label              (query_voxel_features.py views)
  <idx>_labels.pt         {'label_indices': uint8 [H,W]}, 255 = no label (render_semantics_logits.py stores -1 so)
  <name>.png              8-bit single-channel or palette image through PIL: the pixel value is the class, 255 is ignored
In the two 8-bit formats 255 is read as -1, so it is ignored for every --num_classes, 256 included; an .npy map says -1.
and paired by stem: the file name without its extension and without a trailing ``_labels`` (other .npy / .pt files, such as
<name>_confidence.npy, are not label maps).  A ground-truth file without a prediction is an error that names it; --views
restricts the run to the given stems.  A label outside [0, P) is not valid: a pixel whose ground truth is not valid is
skipped, one whose ground truth is valid under a prediction that is not counts in no class (both totals are reported).

The boundary band of a view is max(1, round(boundary_ratio * sqrt(H^2 + W^2))) pixels of the ground truth's size wide.  A
prediction of another size is an error that names both sizes unless --resize_pred is given: then it is resampled to the
ground truth's size, nearest neighbour with src = floor((dst + 0.5) * src_size / dst_size) (PIL's NEAREST).

The report (JSON, byte-identical from run to run) holds the two aggregations of label_metrics.py -- ``dataset``: one
confusion over all views; ``lerf``: per view and class present in its ground truth, averaged over views, then over classes --
plus per-class rows (names from --prompts_npz), the confusion matrix, the skipped totals and one row per view.
The counting runs on the GPU only (voxproj_host.label_scores); there is no CPU path.
"""
import argparse
import json
import os

import numpy as np

import label_metrics

EXTENSIONS = (".npy", ".pt", ".png")


def stem_of(filename):
    """The pairing stem of a label-map file name, None for any other file."""
    base, ext = os.path.splitext(filename)
    if ext.lower() not in EXTENSIONS:
        return None
    labelled = base.endswith("_labels") and len(base) > len("_labels")
    if ext.lower() != ".png" and not labelled:
        return None                                  # <name>_confidence.npy and the like
    return base[:-len("_labels")] if labelled else base


def index_dir(d):
    """{stem: path} of the label maps in ``d`` and ``d/labels``; two files of one stem are an error."""
    if not os.path.isdir(d):
        raise FileNotFoundError(f"{d}: not a directory")
    found = {}
    for sub in (d, os.path.join(d, "labels")):
        if not os.path.isdir(sub):
            continue
        for name in sorted(os.listdir(sub)):
            stem = stem_of(name)
            path = os.path.join(sub, name)
            if stem is None or not os.path.isfile(path):
                continue
            if stem in found:
                raise ValueError(f"{d}: two label maps for '{stem}': {found[stem]} and {path}")
            found[stem] = path
    return found


def pair_files(pred_dir, gt_dir, views=None):
    """[(stem, ground-truth path, prediction path)] sorted by stem."""
    gt, pred = index_dir(gt_dir), index_dir(pred_dir)
    if views:
        missing = [v for v in views if v not in gt]
        if missing:
            raise KeyError(f"{gt_dir}: no ground-truth label map for {', '.join(missing)}")
        gt = {v: gt[v] for v in views}
    if not gt:
        raise ValueError(f"{gt_dir}: no label maps ({', '.join(EXTENSIONS)})")
    pairs = []
    for stem in sorted(gt):
        if stem not in pred:
            raise FileNotFoundError(f"{gt[stem]}: no prediction for '{stem}' in {pred_dir}")
        pairs.append((stem, gt[stem], pred[stem]))
    return pairs


def load_label_map(path):
    """One label map as int32 [H,W]; what the file marks as ignored comes out as a value outside every [0, P)."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        a = np.load(path)
    elif ext == ".pt":
        import torch
        d = torch.load(path)
        if not isinstance(d, dict) or "label_indices" not in d:
            raise ValueError(f"{path}: no 'label_indices' entry")
        a = d["label_indices"].cpu().numpy()
        if a.dtype == np.uint8:
            a = a.astype(np.int32)
            a[a == 255] = -1                           # the renderer's labels.to(uint8) of "no label"
    elif ext == ".png":
        try:
            from PIL import Image
        except ImportError as e:
            raise RuntimeError(f"{path}: reading .png label maps needs PIL, which does not import ({e})") from None
        with Image.open(path) as im:
            if im.mode not in ("L", "P"):
                raise ValueError(f"{path}: mode {im.mode}; a label map is an 8-bit single-channel or palette image")
            a = np.array(im).astype(np.int32)          # (a palette image yields its indices)
        a[a == 255] = -1
    else:
        raise ValueError(f"{path}: unknown label-map format")
    if a.ndim != 2 or not np.issubdtype(a.dtype, np.integer) or a.size == 0:
        raise ValueError(f"{path}: a label map is a non-empty integer [H, W] array, not {a.dtype} {a.shape}")
    a = a.astype(np.int64)
    return np.where((a >= -(1 << 31)) & (a < (1 << 31)), a, -1).astype(np.int32)


def resize_index(dst_size, src_size):
    """src = floor((dst + 0.5) * src_size / dst_size) for dst = 0 .. dst_size - 1, in exact integer arithmetic."""
    dst = np.arange(int(dst_size), dtype=np.int64)
    return np.minimum(((2 * dst + 1) * int(src_size)) // (2 * int(dst_size)), int(src_size) - 1)


def resize_nearest(a, W, H):
    return np.ascontiguousarray(a[resize_index(H, a.shape[0])][:, resize_index(W, a.shape[1])])


def gpu_scorer(device=None):
    """score(pred, gt, P, radius) -> (confusion, skipped, bnd_inter, bnd_union) of that view alone, counted on the GPU."""
    import torch
    import voxproj_host
    if not torch.cuda.is_available():
        raise RuntimeError("evaluate_label_maps counts on the GPU: there is no CPU path")
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    state = dict(ws=voxproj_host.SplatWorkspace(), out=None)

    def score(pred, gt, P, radius):
        if state["out"] is None or state["out"].P != P:
            state["out"] = voxproj_host.LabelScores(P, dev)
        out = state["out"].zero_()
        voxproj_host.label_scores(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), P, radius, out=out,
                                  workspace=state["ws"])
        return out.numpy()
    return score


def evaluate(pairs, P, boundary_ratio=0.02, boundary=True, resize_pred=False, score=None, names=None):
    """The report (a dict of plain Python values) for ``pairs`` of pair_files; ``score`` as gpu_scorer returns it."""
    if not 1 <= int(P) <= 256:
        raise ValueError(f"--num_classes {P} outside [1, 256]")
    P = int(P)
    score = score if score is not None else gpu_scorer()
    if names is not None and len(names) != P:
        raise ValueError(f"{len(names)} class names for {P} classes")
    total = [np.zeros((P, P), np.int64), np.zeros(2, np.int64), np.zeros(P, np.int64), np.zeros(P, np.int64)]
    per_view, rows = [], []
    for stem, gt_path, pred_path in pairs:
        gt, pred = load_label_map(gt_path), load_label_map(pred_path)
        H, W = gt.shape
        resized = pred.shape != gt.shape
        if resized:
            if not resize_pred:
                raise ValueError(f"{pred_path}: the prediction is {pred.shape[1]}x{pred.shape[0]} but the ground truth "
                                 f"{gt_path} is {W}x{H} (--resize_pred resamples it)")
            pred = resize_nearest(pred, W, H)
        radius = label_metrics.boundary_radius(W, H, boundary_ratio) if boundary else 0
        if radius > 4096:
            raise ValueError(f"{gt_path}: a boundary band of {radius} pixels exceeds 4096 (lower --boundary_ratio)")
        conf, skipped, inter, union = (np.asarray(v, np.int64) for v in score(pred, gt, P, radius))
        for acc, part in zip(total, (conf, skipped, inter, union)):
            acc += part
        m = label_metrics.metrics(conf, inter if boundary else None, union if boundary else None)
        per_view.append((conf, inter if boundary else None, union if boundary else None))
        rows.append(dict(name=stem, width=int(W), height=int(H), radius=int(radius), resized=bool(resized), miou=m["miou"],
                         fwiou=m["fwiou"], pixel_accuracy=m["pixel_accuracy"], mbiou=m.get("mbiou"),
                         skipped=[int(v) for v in skipped]))
    d = label_metrics.metrics(total[0], total[2] if boundary else None, total[3] if boundary else None)
    lerf = label_metrics.lerf_aggregate(per_view)
    classes = [dict(index=c, name=str(names[c]) if names is not None else str(c), pixels=d["row"][c], iou=d["iou"][c],
                    biou=d["biou"][c] if boundary else None, lerf_iou=lerf["iou"][c],
                    lerf_biou=lerf["biou"][c] if boundary else None, lerf_views=lerf["views_per_class"][c]) for c in range(P)]
    return dict(num_classes=P, views=len(rows), boundary_ratio=float(boundary_ratio) if boundary else None,
                dataset=dict(miou=d["miou"], fwiou=d["fwiou"], pixel_accuracy=d["pixel_accuracy"], mbiou=d.get("mbiou")),
                lerf=dict(miou=lerf["miou"], mbiou=lerf["mbiou"] if boundary else None),
                classes=classes, confusion=[[int(v) for v in r] for r in total[0]],
                skipped=dict(target_not_valid=int(total[1][0]), prediction_not_valid=int(total[1][1])),
                bnd_inter=[int(v) for v in total[2]] if boundary else None,
                bnd_union=[int(v) for v in total[3]] if boundary else None, per_view=rows)


def write_report(path, report):
    with open(path, "w") as f:
        f.write(json.dumps(report, indent=1, sort_keys=True, allow_nan=False) + "\n")


def build_parser():
    ap = argparse.ArgumentParser(description="Score label maps against ground truth (confusion and boundary IoU on the GPU)")
    ap.add_argument("--pred", required=True, help="directory of predicted label maps")
    ap.add_argument("--gt", required=True, help="directory of ground-truth label maps")
    ap.add_argument("--num_classes", type=int, required=True)
    ap.add_argument("--prompts_npz", default="", help=".npz whose 'prompts' name the classes")
    ap.add_argument("--views", nargs="*", default=None, help="stems to score (default: every ground-truth map)")
    ap.add_argument("--boundary_ratio", type=float, default=0.02, help="band width as a share of the image diagonal")
    ap.add_argument("--no_boundary", action="store_true", help="confusion only")
    ap.add_argument("--resize_pred", action="store_true", help="resample a prediction of another size (nearest neighbour)")
    ap.add_argument("--out", required=True, help="the report (JSON)")
    return ap


def main(argv=None, score=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if not args.boundary_ratio > 0:
        ap.error("--boundary_ratio must be > 0")
    names = None
    if args.prompts_npz:
        d = np.load(args.prompts_npz)
        if "prompts" not in d:
            raise KeyError(f"{args.prompts_npz}: no 'prompts' array")
        names = [str(x) for x in d["prompts"]]
    pairs = pair_files(args.pred, args.gt, args.views)
    report = evaluate(pairs, args.num_classes, args.boundary_ratio, not args.no_boundary, args.resize_pred, score, names)
    write_report(args.out, report)
    fmt = lambda v: "null" if v is None else f"{v:.4f}"  # noqa: E731
    ds, lf = report["dataset"], report["lerf"]
    print(f"[EVAL] {report['views']} view(s), {args.num_classes} classes; skipped {report['skipped']['target_not_valid']} "
          f"unlabelled and {report['skipped']['prediction_not_valid']} unpredicted pixel(s)")
    print(f"[EVAL] dataset: mIoU {fmt(ds['miou'])}, fwIoU {fmt(ds['fwiou'])}, pixel accuracy {fmt(ds['pixel_accuracy'])}, "
          f"mBIoU {fmt(ds['mbiou'])}")
    print(f"[EVAL] lerf:    mIoU {fmt(lf['miou'])}, mBIoU {fmt(lf['mbiou'])}")
    print(f"[EVAL] -> {args.out}")
    return report


if __name__ == "__main__":
    main()
