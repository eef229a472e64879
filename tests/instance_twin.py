"""lift_instance_features.py's loop in float64 on the CPU, on the scene of tests/codebook_scene.py (600 Gaussians in four
classes, four 64 x 48 views, masks with per-view permuted ids, -1 / 255 where alpha < 0.5).

The geometry is fixed, so a view's render is linear in the identity rows: ``matrices`` builds one dense A_v [H W, N] per view
with a single tests/splat_reference.py splat64 of the identity matrix, and A_v @ rows is splat64 of the rows up to the order
of a float64 sum (tests/test_lift_instance_cpu.py holds it to that).  ``train64`` mirrors lift_instance_features.main step
for step: the start rows are the command line's fp32 draw, the generator is consumed in its order (randn for the start rows,
then per step randperm, then one draw_count per picked view), the loss and its gradient image are
tests/proto_loss_reference.py's statement64, the gradient of the rows is A_v.T @ that image, the mean over the picked views
goes into codebook_scene.adam64.  The loss before and after is evaluate()'s: every pixel of every view.

``seen`` and ``separation`` say how well trained rows tell the classes apart; both the float64 loop here and the command
line on the GPU are asked the same end conditions with them.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import codebook_scene as cs  # noqa: E402
import proto_loss_reference as pref  # noqa: E402
import splat_reference as sref  # noqa: E402

# the two configurations both test files run, as the command line's arguments (all with --dim 8 --lr 0.05 --seed 0)
DIM, LR, SEED = 8, 0.05, 0
CONFIGS = {"A": dict(steps=60, samples=None, views_per_step=1), "B": dict(steps=120, samples=2048, views_per_step=2)}


def cli_args(name):
    """Configuration ``name`` as lift_instance_features.py's arguments (without the files)."""
    c = CONFIGS[name]
    how = ["--all_pixels"] if c["samples"] is None else ["--samples", str(c["samples"])]
    return ["--dim", str(DIM), "--lr", str(LR), "--seed", str(SEED), "--steps", str(c["steps"]), "--views_per_step",
            str(c["views_per_step"])] + how


def _geometry(scene):
    g = scene["g"]
    return g["means"], g["quats"], g["scales"], g["opacities"]


def render64(scene, v, rows):
    """splat64 of ``rows`` [N,D] into view v: f64 [D,H,W]."""
    return sref.splat64(*_geometry(scene), rows, scene["w2c"][v].astype(np.float32), scene["K"].astype(np.float32), cs.W,
                        cs.H)["logits"]


def matrices(scene):
    """[A_v f64 [H W, N]] per view: the render of view v is (A_v @ rows).T as [D,H,W]; one splat64 of np.eye(N) each."""
    eye = np.eye(cs.N)
    return [np.ascontiguousarray(render64(scene, v, eye).reshape(cs.N, cs.H * cs.W).T) for v in range(cs.VIEWS)]


def image_of(A_v, rows):
    return np.ascontiguousarray((A_v @ rows).T).reshape(rows.shape[1], cs.H, cs.W)


def view_loss64(A_v, rows, ids, count=None, *, min_count=20, ignore_id=-1, weight_contrast=1.0, weight_norm=1.0, want_grad=False):
    """splat_autograd.splat_contrastive's statement for one view in float64: (L, dL/drows or None, stats)."""
    ref = pref.statement64(image_of(A_v, rows), ids, count, ignore_id=ignore_id, min_count=min_count,
                           weight_contrast=weight_contrast, weight_norm=weight_norm, want_grad=want_grad)
    s0, K, s2, _ = ref["stats"]
    L = (weight_contrast * s0 / K if K > 0 else 0.0) + weight_norm * s2 / (cs.W * cs.H)
    grad = A_v.T @ ref["grad"].reshape(rows.shape[1], cs.H * cs.W).T if want_grad else None
    return L, grad, ref["stats"]


def start_rows(dim=DIM, seed=SEED):
    """(the command line's start rows as float64 [N,dim], the generator after that draw)."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((cs.N, dim), generator=gen).double().numpy(), gen


def train64(scene, A, *, steps, samples, views_per_step, dim=DIM, lr=LR, seed=SEED, min_count=20, ignore_id=-1, weight_contrast=1.0,
            weight_norm=1.0):
    """lift_instance_features.main in float64; ``samples`` None is --all_pixels.  Returns dict(rows f64 [N,dim], loss_before,
    loss_after, ids (the mask ids that took part, summed over the views, before training))."""
    import lift_instance_features as lif
    kw = dict(min_count=min_count, ignore_id=ignore_id, weight_contrast=weight_contrast, weight_norm=weight_norm)
    P, gen = start_rows(dim, seed)
    state = (np.zeros_like(P), np.zeros_like(P), 0)

    def evaluate(P):
        res = [view_loss64(A[v], P, scene["masks"][v], None, **kw) for v in range(cs.VIEWS)]
        return sum(r[0] for r in res) / cs.VIEWS, int(sum(r[2][1] for r in res))

    l0, ids_seen = evaluate(P)
    k = min(views_per_step, cs.VIEWS)
    for _ in range(steps):
        pick = torch.randperm(cs.VIEWS, generator=gen)[:k].tolist()
        grad = np.zeros_like(P)
        for v in pick:
            count = None if samples is None else lif.draw_count(cs.W * cs.H, samples, gen).reshape(cs.H, cs.W).numpy()
            grad += view_loss64(A[v], P, scene["masks"][v], count, want_grad=True, **kw)[1] / k
        P, state = cs.adam64(P, grad, state, lr)
    return dict(rows=P, loss_before=l0, loss_after=evaluate(P)[0], ids=ids_seen)


def seen(A):
    """bool [N]: the Gaussians some view really shows -- their largest column sum of A_v over the views exceeds 1.0 (one
    pixel's worth of blend weight).  The others get next to no gradient and keep their start rows."""
    return np.max([a.sum(0) for a in A], axis=0) > 1.0


def separation(P, classes, seen):
    """(mean cosine of two different seen rows of one class, mean cosine of two seen rows of different classes, accuracy of
    nearest-class-mean classification of the normalised seen rows)."""
    rows = np.asarray(P, np.float64)[seen]
    cl = np.asarray(classes)[seen]
    rows = rows / np.maximum(np.linalg.norm(rows, axis=1, keepdims=True), 1e-12)
    cos = rows @ rows.T
    eq = cl[:, None] == cl[None, :]
    off = ~np.eye(len(rows), dtype=bool)
    labels = np.unique(cl)
    centres = np.stack([rows[cl == c].mean(0) for c in labels])
    nearest = labels[np.argmin(((rows[:, None, :] - centres[None]) ** 2).sum(-1), axis=1)]
    return float(cos[eq & off].mean()), float(cos[~eq].mean()), float((nearest == cl).mean())


def hand_off(scene, rows):
    """What associate_instances.py gets from a lifter that wrote ``rows``: the scene with the rows rounded to binary16 and the
    four images re-rendered from them with splat64."""
    rows16 = torch.from_numpy(np.asarray(rows)).to(torch.float16).float().numpy()
    return dict(scene, rows=rows16, images=[render64(scene, v, rows16) for v in range(cs.VIEWS)])
