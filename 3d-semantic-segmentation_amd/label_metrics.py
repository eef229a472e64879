"""From the integer counts of ``voxproj_host.label_scores`` to the report: IoU per class, mIoU, fwIoU, pixel accuracy and
boundary IoU.  Pure host code (numpy, float64); it never loads the library, so it imports without a GPU.

With n the confusion matrix (rows = ground truth), row_c = sum_p n[c,p] and col_c = sum_t n[t,c]:
  iou[c]         = n[c,c] / (row_c + col_c - n[c,c])
  miou           = mean of iou over the classes whose denominator is > 0
  fwiou          = sum_c row_c iou[c] / sum_c row_c
  pixel_accuracy = trace(n) / sum(n)
  biou[c]        = bnd_inter[c] / bnd_union[c],  mbiou = mean over the classes with bnd_union[c] > 0
A value whose denominator is 0 is None (``null`` in JSON), never NaN.

Two aggregations over several views:
  dataset  one confusion (and one pair of boundary counts) summed over all views, then the formulas above: the mIoU / fwIoU
           of semantic segmentation benchmarks.  A class weighs by its pixels.
  lerf     the order of the LERF mask evaluation: for each view and each class present in that view's ground truth, the IoU
           and boundary IoU of that view's own counts; averaged over the views per class, then over the classes.  A small
           view and a small class weigh as much as large ones.
"""
import numpy as np


def _ratio(num, den):
    return float(num) / float(den) if den > 0 else None


def _mean(values):
    vals = [v for v in values if v is not None]
    return float(np.mean(np.asarray(vals, np.float64))) if vals else None


def metrics(confusion, bnd_inter=None, bnd_union=None):
    """The report of one confusion matrix (any integer array [P,P]) and, optionally, its boundary counts ([P] each): a dict
    of 'iou' (list of float or None), 'miou', 'fwiou', 'pixel_accuracy', 'row' (ground-truth pixels per class) and, with
    boundary counts, 'biou' and 'mbiou'."""
    n = np.asarray(confusion).astype(np.float64)
    if n.ndim != 2 or n.shape[0] != n.shape[1]:
        raise ValueError(f"confusion must be [P, P], not {n.shape}")
    row, col, diag = n.sum(1), n.sum(0), np.diag(n)
    iou = [_ratio(diag[c], row[c] + col[c] - diag[c]) for c in range(n.shape[0])]
    total = float(row.sum())
    fw = sum(row[c] * iou[c] for c in range(n.shape[0]) if iou[c] is not None and row[c] > 0)
    out = dict(iou=iou, miou=_mean(iou), fwiou=_ratio(fw, total), pixel_accuracy=_ratio(diag.sum(), total),
               row=[int(v) for v in np.asarray(confusion).sum(1)])
    if bnd_inter is not None and bnd_union is not None:
        bi, bu = np.asarray(bnd_inter).astype(np.float64), np.asarray(bnd_union).astype(np.float64)
        if bi.shape != (n.shape[0],) or bu.shape != (n.shape[0],):
            raise ValueError(f"bnd_inter / bnd_union must be [{n.shape[0]}]")
        out["biou"] = [_ratio(bi[c], bu[c]) for c in range(n.shape[0])]
        out["mbiou"] = _mean(out["biou"])
    return out


def lerf_aggregate(views):
    """``views``: per view a (confusion, bnd_inter or None, bnd_union or None) of that view alone.  For each view and each
    class present in its ground truth (row_c > 0) the view's IoU and boundary IoU; the mean over those views per class, then
    over the classes: dict of 'iou', 'biou' (per class, None for a class no view's ground truth holds), 'miou', 'mbiou',
    'views_per_class'."""
    views = list(views)
    if not views:
        return dict(iou=[], biou=[], miou=None, mbiou=None, views_per_class=[])
    P = np.asarray(views[0][0]).shape[0]
    ious, bious = [[] for _ in range(P)], [[] for _ in range(P)]
    for conf, bi, bu in views:
        m = metrics(conf, bi, bu)
        for c in range(P):
            if m["row"][c] > 0:
                ious[c].append(m["iou"][c])
                if "biou" in m:
                    bious[c].append(m["biou"][c])
    iou, biou = [_mean(v) for v in ious], [_mean(v) for v in bious]
    return dict(iou=iou, biou=biou, miou=_mean(iou), mbiou=_mean(biou), views_per_class=[len(v) for v in ious])


def boundary_radius(W, H, ratio=0.02):
    """Pixels of the boundary band of a W x H map: max(1, round(ratio * diagonal))."""
    return max(1, int(round(float(ratio) * float(np.sqrt(float(H) ** 2 + float(W) ** 2)))))
