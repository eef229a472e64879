"""Scoring one view (vp_label_scores) against a torch composite, one JSON line per class count: seeded piecewise-constant
label maps at 1600x1067 (rectangles and single pixels over a background, ~10 % of the targets unlabelled), the boundary
radius of --ratio (38 pixels at that size), P in {13, 32}.

  scores_ms / confusion_ms        voxproj_host.label_scores with and without the boundary part (HIP events around --steps
                                  calls after --warmup; int32 maps already on the device, nothing read back)
  band_ms                         voxproj_host.label_boundary of one map alone
  torch_scores_ms / torch_confusion_ms   the composite: torch.bincount of t * P + p over the valid pixels, the bands from
                                  max_pool2d on +labels and -labels (window minimum and maximum, separable: a 1 x k pool and a
                                  k x 1 pool, the cheaper way to ask torch for it) plus the image-border frame, the boundary
                                  counts from three more bincounts
All arms run in one process, alternated twice; the smaller reading of each is reported beside both.  Before timing, both
sides' integers (confusion, skipped, bnd_inter, bnd_union and the band itself) are compared and must be equal.
Read scores_ms against the composite and against raster_ms of tools/bench_splat.py at the same view size.

python tools/bench_eval.py [--steps K] [--warmup W] [--p 13 32] [--size 1600x1067] [--ratio 0.02]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import label_metrics  # noqa: E402
import voxproj_host  # noqa: E402


def make_maps(W, H, P, seed):
    """(pred, target) int32 [H,W]: a target of rectangles and dots, ~10 % of it unlabelled (-1 / 255), and a prediction that
    relabels some rectangles and leaves a few pixels outside [0, P)."""
    rng = np.random.default_rng(seed)

    def paint(m, n, frac, values):
        for _ in range(n):
            w, h = int(rng.integers(1, max(2, int(W * frac)))), int(rng.integers(1, max(2, int(H * frac))))
            x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
            m[y:y + h, x:x + w] = values[int(rng.integers(0, len(values)))]

    target = np.full((H, W), int(rng.integers(0, P)), np.int32)
    paint(target, 40, 0.5, list(range(P)))
    paint(target, 300, 0.004, list(range(P)))
    pred = target.copy()
    paint(target, 45, 0.12, [-1, 255])
    paint(pred, 25, 0.2, list(range(P)))
    paint(pred, 6, 0.01, [-1, 255])
    return pred, target


def torch_band(lab, r):
    x = lab.to(torch.float32)[None, None]
    k = 2 * r + 1
    mx = F.max_pool2d(F.max_pool2d(x, (1, k), 1, (0, r)), (k, 1), 1, (r, 0))
    mn = -F.max_pool2d(F.max_pool2d(-x, (1, k), 1, (0, r)), (k, 1), 1, (r, 0))
    band = ((mx != x) | (mn != x))[0, 0]
    band[:r] = True
    band[-r:] = True
    band[:, :r] = True
    band[:, -r:] = True
    return band


def torch_scores(pred, target, P, r):
    tv, pv = (target >= 0) & (target < P), (pred >= 0) & (pred < P)
    both = tv & pv
    conf = torch.bincount((target[both].long() * P + pred[both].long()), minlength=P * P).reshape(P, P)
    skipped = torch.stack([(~tv).sum(), (tv & ~pv).sum()])
    if r == 0:
        return conf, skipped, None, None, None
    pb, tb = torch_band(pred, r), torch_band(target, r)
    inter = torch.bincount(target[both & pb & tb & (pred == target)].long(), minlength=P)
    union = torch.bincount(target[tv & tb].long(), minlength=P) + torch.bincount(pred[both & pb].long(), minlength=P) - inter
    return conf, skipped, inter, union, pb


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--p", type=int, nargs="+", default=[13, 32])
    ap.add_argument("--size", default="1600x1067")
    ap.add_argument("--ratio", type=float, default=0.02)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    W, H = (int(v) for v in args.size.split("x"))
    r = label_metrics.boundary_radius(W, H, args.ratio)
    for P in args.p:
        pred_np, target_np = make_maps(W, H, P, seed=P)
        pred, target = torch.from_numpy(pred_np).to(dev), torch.from_numpy(target_np).to(dev)
        ws = voxproj_host.SplatWorkspace()
        # the same integers from both sides
        ours = voxproj_host.label_scores(pred, target, P, r, workspace=ws)
        conf, skipped, inter, union, pb = torch_scores(pred, target, P, r)
        same = (torch.equal(ours.confusion, conf) and torch.equal(ours.skipped, skipped) and torch.equal(ours.bnd_inter, inter)
                and torch.equal(ours.bnd_union, union)
                and torch.equal(voxproj_host.label_boundary(pred, r, workspace=ws).bool(), pb)
                and torch.equal(voxproj_host.label_scores(pred, target, P).confusion, conf))
        if not same:
            raise SystemExit(f"P = {P}: vp_label_scores and the torch composite disagree")
        out = voxproj_host.LabelScores(P, dev)
        arms = (("scores_ms", lambda: voxproj_host.label_scores(pred, target, P, r, out=out, workspace=ws)),
                ("confusion_ms", lambda: voxproj_host.label_scores(pred, target, P, 0, out=out)),
                ("band_ms", lambda: voxproj_host.label_boundary(pred, r, workspace=ws)),
                ("torch_scores_ms", lambda: torch_scores(pred, target, P, r)),
                ("torch_confusion_ms", lambda: torch_scores(pred, target, P, 0)))
        ms = {k: [] for k, _ in arms}
        for _ in range(2):
            for k, fn in arms:
                ms[k].append(timed(fn, args.steps, args.warmup))
        res = dict(metric="label_scores_ms_per_view", W=W, H=H, P=P, radius=r, integers_equal=True,
                   band_share=round(float(pb.float().mean()), 4), skipped=[int(v) for v in skipped.tolist()])
        for k, _ in arms:
            res[k] = round(min(ms[k]), 4)
            res[k + "_runs"] = [round(v, 4) for v in ms[k]]
        res["scores_over_torch"] = round(res["scores_ms"] / res["torch_scores_ms"], 4)
        res["confusion_over_torch"] = round(res["confusion_ms"] / res["torch_confusion_ms"], 4)
        res.update(steps=args.steps, warmup=args.warmup)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
