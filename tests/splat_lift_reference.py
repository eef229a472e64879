"""The lift's contract (include/voxproj.h, vp_splat_lift) in float64 NumPy, shared by test_splat_lift_cpu.py and
test_gpu_splat_lift.py.  The lift is the transpose of the splatter, and splat_grad_reference.splat_grad64 already states
that transpose: for a loss L = sum G * logits its grad_f[g, c] is sum_p G[c, p] w_g(p), with the forward's decisions (every
Gaussian tried at every pixel in (fp32 z, index) order, skipped when sigma < 0 or a < 1/255, a pixel stopping before the
Gaussian that would take T to <= 1e-4).  So with the upstream G = [m * feat^T ; m] of C + 1 channels and zero features
(grad_o is not used), grad_f is (sum | wsum) and M_f the same sums over absolute values.
"""
import numpy as np

import splat_grad_reference as gref
import splat_reference as ref


def upstream(feats, pixel_weight=None):
    """G [C+1,H,W] float64 of a map [H,W,C] (any float dtype, converted exactly) and pixel weights [H,W] (None: 1).  A pixel
    with weight 0 contributes nothing whatever its map holds (NaN included)."""
    F = np.asarray(feats).astype(np.float64)
    H, W, _ = F.shape
    m = np.ones((H, W)) if pixel_weight is None else np.asarray(pixel_weight).astype(np.float64)
    F = np.where((m > 0)[..., None], F, 0.0)
    return np.concatenate([(m[..., None] * F).transpose(2, 0, 1), m[None]])


def lift64(means, quats, scales, opacities, feats, viewmat, K, W, H, pixel_weight=None, **kw):
    """dict(sum [N,C], wsum [N], M_sum, M_wsum (the magnitude sums), G (the upstream, for grad_bound), fragile bool [H,W],
    visits int [H,W], added int [N]) of one view; ``kw``: near, far, eps2d."""
    G = upstream(feats, pixel_weight)
    C = G.shape[0] - 1
    N = len(np.asarray(means))
    r = gref.splat_grad64(means, quats, scales, opacities, np.zeros((N, C + 1)), viewmat, K, W, H, G=G, **kw)
    return dict(sum=r["grad_f"][:, :C], wsum=r["grad_f"][:, C], M_sum=r["M_f"][:, :C], M_wsum=r["M_f"][:, C], G=G,
                fragile=r["fragile"], visits=r["visits"], added=r["added"])


def fragile_pixels(means, quats, scales, opacities, viewmat, K, W, H, **kw):
    """bool [H,W]: pixels where a decision lies within the oracle's fragile band (fp32 may take it the other way)."""
    N = len(np.asarray(means))
    return ref.splat64(means, quats, scales, opacities, np.zeros((N, 1)), viewmat, K, W, H, **kw)["fragile"]


def added_weights(means, quats, scales, opacities, viewmat, K, W, H, pixels, **kw):
    """The weights w = a T of every added (pixel, Gaussian) pair at the (row, col) ``pixels``, concatenated."""
    rec = ref.records(means, quats, scales, opacities, viewmat, K, W, H, **kw)
    return np.concatenate([ref.pixel64(rec, int(i), int(j), False)["w"] for i, j in pixels] + [np.zeros(0)])


def finish64(sum_, wsum, min_weight):
    """(avg [N,C], valid bool [N]) as GaussianFeatureLifter.finish defines them."""
    valid = (wsum >= min_weight) & (wsum > 0)
    return np.where(valid[:, None], sum_ / np.where(valid, wsum, 1.0)[:, None], 0.0), valid


# ------------------------------------------------------------------------------------------------------------------------
# The end-to-end scene: three well separated clusters of Gaussians, each carrying one of three constant feature vectors,
# seen by two cameras.  The maps are the float64 forward's renders of those features, rounded to fp16.
# ------------------------------------------------------------------------------------------------------------------------
CLASS_W, CLASS_H, CLASS_C = 61, 47, 8
CLASS_MIN_WEIGHT = 0.05


def class_vectors():
    v = np.zeros((3, CLASS_C), np.float32)
    for c in range(CLASS_C):
        v[c % 3, c] = 1.0 + 0.25 * (c // 3)
    return v


def class_scene(n_per=80, seed=5):
    """dict(s (means, quats, scales, opacities), cls int [N], views [(vm, K)] x 2, maps [fp16 [H,W,C]] x 2)."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    centres = np.array([[-0.9, 0.0], [0.0, 0.0], [0.9, 0.0]])
    means, cls = [], []
    for k in range(3):
        xy = centres[k] + rng.uniform(-0.28, 0.28, (n_per, 2)) * np.array([1.0, 2.0])
        means.append(np.concatenate([xy, rng.uniform(2.0, 3.0, (n_per, 1))], 1))
        cls.append(np.full(n_per, k))
    means, cls = np.concatenate(means), np.concatenate(cls)
    n = len(means)
    s = dict(means=means.astype(f32), quats=rng.normal(size=(n, 4)).astype(f32),
             scales=(0.035 * np.exp(rng.normal(0, 0.3, (n, 3)))).astype(f32), opacities=rng.uniform(0.4, 0.9, n).astype(f32))
    feats = class_vectors()[cls]
    views, maps = [], []
    for yaw, tx in ((0.0, 0.0), (0.04, -0.05)):
        vm = np.eye(4)
        cy, sy = np.cos(yaw), np.sin(yaw)
        vm[:3, :3] = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        vm[:3, 3] = (tx, 0.0, 0.0)
        K = np.array([[52.0, 0, CLASS_W / 2], [0, 52.0, CLASS_H / 2], [0, 0, 1]])
        vm, K = vm.astype(f32), K.astype(f32)
        o = ref.splat64(s["means"], s["quats"], s["scales"], s["opacities"], feats, vm, K, CLASS_W, CLASS_H)
        views.append((vm, K))
        maps.append(np.ascontiguousarray(o["logits"].transpose(1, 2, 0)).astype(np.float16))
    return dict(s=s, cls=cls, views=views, maps=maps)


def class_reference(sc):
    """(sum [N,C], wsum [N]) of the float64 lift over the scene's two views."""
    s = sc["s"]
    tot, wt = 0.0, 0.0
    for (vm, K), mp in zip(sc["views"], sc["maps"]):
        r = lift64(s["means"], s["quats"], s["scales"], s["opacities"], mp, vm, K, CLASS_W, CLASS_H)
        tot, wt = tot + r["sum"], wt + r["wsum"]
    return tot, wt
