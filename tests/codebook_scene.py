"""The tiny scene of tests/test_gpu_codebook_assoc.py and its float64 twin: a few hundred Gaussians (tests/splat_scenes.py)
in four classes, four 64 x 48 views, identity rows built directly as class direction plus noise (rounded to binary16,
as IDENTITY.pt stores them), and per view the class image with its ids permuted by a seeded generator.  Everything here
runs on the CPU: the images come from tests/splat_reference.py, the training loop is associate_instances.py's five steps
with tests/codebook_reference.py and tests/proto_loss_reference.py in place of the kernels and Adam in float64, drawing the
same views from the same generator.  tests/test_codebook_cpu.py checks that this loop alone reaches the end condition in
STEPS steps; the GPU test then asks the same of the command line.
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import codebook_reference as cref  # noqa: E402
import proto_loss_reference as pref  # noqa: E402
import splat_reference as sref  # noqa: E402
import splat_scenes as scenes  # noqa: E402
import synthetic_gaussians as sg  # noqa: E402

N, CLASSES, D, W, H, VIEWS = 600, 4, 8, 64, 48, 4
CODES, STEPS, LR, NOISE, SEED = 8, 150, 0.02, 0.1, 0      # the step count the float64 loop was shown to need: see the CPU test


def make():
    """dict: g (the Gaussians), rows f32 [N,D] (binary16 values), w2c, K, names, perms [V][CLASSES] (class -> id of the view),
    images f64 [V][D,H,W], alpha [V][H,W], masks int32 [V][H,W] (255 -> -1 where alpha < 0.5)."""
    # the Gaussians fill the first camera's image (splat_scenes.scene_for_camera); a Gaussian's class is the quadrant of that
    # image its centre falls into, so every view, a small turn and shift away, sees four coherent regions
    poses = [((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), ((0.12, -0.05, 0.1), (0.15, -0.05, 0.1)),
             ((-0.1, 0.08, -0.15), (-0.1, 0.1, 0.2)), ((0.05, 0.1, 0.3), (0.05, -0.12, 0.3))]
    cams = [scenes._cam(scenes.euler(*a), t, 0.9 * W, 0.9 * W, 0.5 * W, 0.5 * H) for a, t in poses]
    w2c = np.stack([vm for vm, _ in cams]).astype(np.float64)
    K = cams[0][1].astype(np.float64)
    g = scenes.scene_for_camera(N, D, 5, w2c[0], K, W, H, z=(2.0, 3.0), margin=0.1, scale=0.12, sigma=0.3)
    g["opacities"] = np.maximum(g["opacities"], np.float32(0.5))
    pc = g["means"].astype(np.float64) @ w2c[0][:3, :3].T + w2c[0][:3, 3]
    u, v = K[0, 0] * pc[:, 0] / pc[:, 2] + K[0, 2], K[1, 1] * pc[:, 1] / pc[:, 2] + K[1, 2]
    g["classes"] = ((u > 0.5 * W).astype(np.int64) + 2 * (v > 0.5 * H).astype(np.int64))
    rng = np.random.default_rng(11)
    dirs = np.linalg.qr(rng.normal(size=(D, D)))[0][:CLASSES]
    rows = dirs[g["classes"]] + NOISE * rng.normal(size=(N, D))
    rows = torch.from_numpy(rows).to(torch.float16).float().numpy()
    onehot = np.eye(CLASSES, dtype=np.float32)[g["classes"]]
    images, alphas, masks, perms = [], [], [], []
    for vm in w2c:
        args = (g["means"], g["quats"], g["scales"], g["opacities"])
        cls = sref.splat64(*args, onehot, vm.astype(np.float32), K.astype(np.float32), W, H)
        img = sref.splat64(*args, rows, vm.astype(np.float32), K.astype(np.float32), W, H)
        perm = rng.permutation(CLASSES) + 20 * rng.integers(0, 5)        # ids that mean nothing across views
        ids = perm[cls["label"]].astype(np.int32)
        ids[cls["alpha"] < 0.5] = -1
        images.append(img["logits"]); alphas.append(img["alpha"]); masks.append(ids); perms.append(perm)
    names = [f"DSC{v:05d}.JPG" for v in range(VIEWS)]
    return dict(g=g, rows=rows, w2c=w2c, K=K, names=names, perms=perms, images=images, alpha=alphas, masks=masks)


def write_files(scene, out):
    """The command line's inputs under ``out``: (ply, camera_params.json, masks dir, IDENTITY.pt)."""
    from PIL import Image
    import lift_gaussian_features as lgf
    from gaussian_ply import write_gaussian_ply
    g = scene["g"]
    os.makedirs(os.path.join(out, "object_mask"), exist_ok=True)
    ply, cam, ident = os.path.join(out, "point_cloud.ply"), os.path.join(out, "camera_params.json"), os.path.join(out, "identity.pt")
    op, ls, q = sg.to_ply_fields(g)
    write_gaussian_ply(ply, g["means"], op, ls, q)
    sg.write_camera_params(cam, scene["w2c"], scene["K"], W, H, names=scene["names"])
    for name, ids in zip(scene["names"], scene["masks"]):
        Image.fromarray(np.where(ids < 0, 255, ids).astype(np.uint8), mode="L").save(os.path.join(out, "object_mask", name + ".png"))
    lgf.save_lifted(ident, torch.from_numpy(g["means"]), torch.from_numpy(scene["rows"]), torch.ones(N), scene["names"])
    return ply, cam, os.path.join(out, "object_mask"), ident


def loss64(image, ids, conf, codebook, assign, weight_cls=1.0, weight_cluster=1.0, conf_min=0.2, want_grad=True):
    """splat_autograd.codebook_loss's statement in float64: (L, dL/dB, the statement64 result)."""
    K = codebook.shape[0]
    ref = cref.statement64(image, ids, codebook, assign, conf, conf_min=conf_min, want_grad=want_grad)
    s0, s1, n, mis = ref["stats"]
    on = K > 1 and mis > 0 and n > 0
    sc = weight_cls / (n * math.log(K)) if on else 0.0
    sk = weight_cluster / n if n > 0 else 0.0
    grad = sc * ref["grad_cls"] + sk * ref["grad_cluster"] if want_grad else None
    return sc * s0 + sk * s1, grad, ref


def view_pass64(scene, v, codebook):
    """Steps 2 - 5 of associate_instances.py on view v in float64: (L, dL/dB, assign)."""
    import voxproj_host
    image = scene["images"][v].astype(np.float32)
    ids = scene["masks"][v]
    conf = pref.statement64(image, ids, None, **pref.CONFIDENCE_PARAMS)["own_prob"].reshape(H, W).astype(np.float32)
    ref = cref.statement64(image, ids, codebook)
    assign = voxproj_host.assign_view_ids(ref["score"], ref["id_pixels"], codebook.shape[0])
    L, grad, _ = loss64(image, ids, conf, codebook, assign)
    return L, grad, assign


def adam64(B, grad, state, lr, b1=0.9, b2=0.999, eps=1e-8):
    """One step of torch's Adam in float64; state = (m, v, t)."""
    m, v, t = state
    t += 1
    m = b1 * m + (1 - b1) * grad
    v = b2 * v + (1 - b2) * grad * grad
    B = B - lr * (m / (1 - b1 ** t)) / (np.sqrt(v / (1 - b2 ** t)) + eps)
    return B, (m, v, t)


def train64(scene, codes=CODES, steps=STEPS, lr=LR, seed=SEED):
    """associate_instances.py's loop in float64 (the code book is kept as float32 values between steps only at the start).
    Returns (codebook f64, loss before, loss after, [assign per view])."""
    import associate_instances as ai
    gen = torch.Generator().manual_seed(seed)
    B = ai.init_codebook(codes, D, gen).double().numpy()
    state = (np.zeros_like(B), np.zeros_like(B), 0)

    def mean_loss(B):
        return sum(view_pass64(scene, v, B.astype(np.float32))[0] for v in range(VIEWS)) / VIEWS
    l0 = mean_loss(B)
    for _ in range(steps):
        v = int(torch.randint(0, VIEWS, (1,), generator=gen))
        _, grad, _ = view_pass64(scene, v, B.astype(np.float32))
        B, state = adam64(B, grad, state, lr)
    assigns = [view_pass64(scene, v, B.astype(np.float32))[2] for v in range(VIEWS)]
    return B, l0, mean_loss(B), assigns


def class_to_code(scene, assigns):
    """int [V, CLASSES]: the code every view gives every class (its id -> code map after the view's permutation), -1 where
    the class has no pixel in the view."""
    out = np.full((VIEWS, CLASSES), -1, np.int64)
    for v in range(VIEWS):
        present = np.unique(scene["masks"][v][scene["masks"][v] >= 0])
        for c in range(CLASSES):
            if scene["perms"][v][c] in present:
                out[v, c] = assigns[v][scene["perms"][v][c]]
    return out


def consistent(table):
    """The end condition: every class seen in a view has a code there, and the same code in every view that sees it; two
    classes never share a code."""
    codes = []
    for c in range(table.shape[1]):
        seen = table[:, c][table[:, c] >= 0]
        if len(seen) == 0 or (seen != seen[0]).any():
            return False
        codes.append(int(seen[0]))
    return len(set(codes)) == len(codes)
