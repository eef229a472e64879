"""The scenes of test_gpu_splat_scale.py and test_gpu_splat_cameras.py, built here so that test_splat_sampled_cpu.py can check
the oracle and the fp32 twin on the very same inputs without a GPU.  Every scene is a dict(s (the Gaussians and features),
vm, K, W, H, kw (near / far / eps2d where not the defaults), pixels (the sampled (row, col) pixels, or None for all), cap
(the fragile share the scene must stay under)).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

TILE = 16
PROD_W, PROD_H = 1600, 1067


def euler(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    return (np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]]) @
            np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]))


def all_pixels(W, H):
    return np.stack(np.meshgrid(np.arange(H), np.arange(W), indexing="ij"), -1).reshape(-1, 2)


def sample_pixels(W, H, seed, n_scatter, tiles):
    """(row, col) pixels: the whole 16x16 tiles ``tiles`` [(ty, tx)] (clipped to the image: the last ones are partial) plus
    n_scatter distinct pixels of a seeded generator."""
    px = []
    for ty, tx in tiles:
        ii, jj = np.meshgrid(np.arange(ty * TILE, min((ty + 1) * TILE, H)), np.arange(tx * TILE, min((tx + 1) * TILE, W)),
                             indexing="ij")
        px.append(np.stack([ii.ravel(), jj.ravel()], 1))
    rng = np.random.default_rng(seed)
    flat = rng.choice(W * H, n_scatter, replace=False)
    px.append(np.stack([flat // W, flat % W], 1))
    return np.unique(np.concatenate(px), axis=0)


def production(n, D, view, n_views=2, n_scatter=900, few=False):
    """synthetic_gaussians' room as tools/bench_splat.py renders it: 1600x1067, trajectory view ``view`` of n_views."""
    import synthetic_gaussians as sg
    g = sg.make_gaussians(n, seed=0)
    w2c, K = sg.make_views(n_views * 12, g["room"], PROD_W, seed=0)
    s = {k: g[k] for k in ("means", "quats", "scales", "opacities")}
    s["features"] = sg.make_logits(g["classes"], D, seed=0)
    tx_last, ty_last = (PROD_W - 1) // TILE, (PROD_H - 1) // TILE
    tiles = [(ty_last, tx_last)] if few else [(0, 0), (31, tx_last), (ty_last, 47), (ty_last, tx_last), (40, 50)]
    return dict(s=s, vm=w2c[::12][view].astype(np.float32), K=K.astype(np.float32), W=PROD_W, H=PROD_H, kw={},
                pixels=sample_pixels(PROD_W, PROD_H, 100 + view, n_scatter, tiles), cap=0.2)


def scene_for_camera(n, D, seed, vm, K, W, H, z=(1.0, 4.0), margin=0.2, scale=0.05, sigma=0.6):
    """n Gaussians whose centres project into the image widened by ``margin`` on each side, at camera depths z, for any
    camera: pixel and depth are drawn, then taken back to the world."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(-margin * W, (1 + margin) * W, n)
    v = rng.uniform(-margin * H, (1 + margin) * H, n)
    zc = rng.uniform(*z, n)
    vm, K = np.asarray(vm, np.float64), np.asarray(K, np.float64)
    pc = np.stack([(u - K[0, 2]) / K[0, 0] * zc, (v - K[1, 2]) / K[1, 1] * zc, zc], 1)
    means = (pc - vm[:3, 3]) @ vm[:3, :3]
    op = np.where(rng.uniform(size=n) < 0.2, rng.uniform(0.001, 0.05, n), rng.uniform(0.3, 0.99, n))
    f32 = np.float32
    return dict(means=means.astype(f32), quats=rng.normal(size=(n, 4)).astype(f32),
                scales=(scale * np.exp(rng.normal(0, sigma, size=(n, 3)))).astype(f32), opacities=op.astype(f32),
                features=rng.normal(0, 1, size=(n, D)).astype(f32))


def _cam(R, t, fx, fy, cx, cy):
    vm = np.eye(4)
    vm[:3, :3], vm[:3, 3] = R, t
    return vm.astype(np.float32), np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)


CAMERAS = ("anisotropic", "principal_outside", "rolled", "clamped", "near_far", "eps0", "eps005", "eps1")


def camera_scene(name, D=8):
    """The small scenes of the camera and parameter cases (dense oracle)."""
    W, H = 77, 53
    kw, margin, scale, n, z = {}, 0.2, 0.05, 500, (1.0, 4.0)
    R, t = euler(0.05, -0.03, 0.0), (0.02, -0.01, 0.1)
    fx = fy = 0.9 * W
    cx, cy = 0.5 * W + 0.3, 0.5 * H - 0.2
    if name == "anisotropic":
        fx, fy = 1.3 * W, 0.75 * W                       # fx / fy = 1.73
    elif name == "principal_outside":
        cx, cy = -0.35 * W, 1.2 * H                      # outside the image on both axes
    elif name == "rolled":
        R, t = euler(0.9, -1.1, 1.2), (0.3, -0.2, 0.4)
    elif name == "clamped":
        R, margin, scale, z = euler(0.4, 0.3, -0.7), 0.45, 0.3, (1.5, 3.0)   # centres up to 45 % outside: past the 15 % clamp
    elif name == "near_far":
        kw = dict(near=1.6, far=2.9)
    elif name.startswith("eps"):
        kw = dict(eps2d={"eps0": 0.0, "eps005": 0.05, "eps1": 1.0}[name])
    vm, K = _cam(R, t, fx, fy, cx, cy)
    s = scene_for_camera(n, D, CAMERAS.index(name) + 40, vm, K, W, H, z=z, margin=margin, scale=scale)
    if name == "eps0":
        s["scales"][::4] = 0.0                           # no footprint at all without the dilation: culled (det = 0)
        s["scales"][1::4, 2] = 0.0                       # flat discs: a footprint, Sigma of rank 2
    return dict(s=s, vm=vm, K=K, W=W, H=H, kw=kw, pixels=None, cap=0.2)


def ties_scene(D=6, reverse=False):
    """Identity rotation and no translation along z: the fp32 depth is mz exactly.  12 groups of 6 overlapping Gaussians
    with bit-equal mz and substantial opacities, one group of 700 faint ones over one tile (a run of more than 256 equal
    keys), and 150 ordinary ones.  ``reverse`` reverses the index order inside every group (the same Gaussians)."""
    W, H = 48, 40
    rng = np.random.default_rng(77)
    f32 = np.float32
    vm, K = _cam(np.eye(3), (0.0, 0.0, 0.0), 40.0, 40.0, 24.0, 20.0)
    s = scene_for_camera(150, D, 78, vm, K, W, H, z=(1.0, 4.0))
    groups, parts = [], [s]
    at = 150
    for g in range(13):
        n = 700 if g == 12 else 6
        zc = f32(rng.uniform(1.2, 3.5))
        c = rng.uniform(-0.3, 0.3, 2)
        m = np.stack([c[0] + rng.uniform(-0.08, 0.08, n), c[1] + rng.uniform(-0.08, 0.08, n), np.full(n, zc)], 1)
        parts.append(dict(means=m.astype(f32), quats=rng.normal(size=(n, 4)).astype(f32),
                          scales=rng.uniform(*((0.4, 0.6) if g == 12 else (0.1, 0.2)), (n, 3)).astype(f32),
                          opacities=(rng.uniform(0.006, 0.015, n) if g == 12 else rng.uniform(0.4, 0.9, n)).astype(f32),
                          features=rng.normal(0, 1, (n, D)).astype(f32)))
        if g == 12:                                          # the front half pulls channel 0, the back half channel 1
            parts[-1]["features"][:n // 2, 0] += 3.0
            parts[-1]["features"][n // 2:, 1] += 3.0
        groups.append(np.arange(at, at + n))
        at += n
    s = {k: np.concatenate([p[k] for p in parts]) for k in s}
    s["means"][:, 2] = s["means"][:, 2].astype(f32)
    if reverse:
        perm = np.arange(at)
        for g in groups:
            perm[g] = g[::-1]
        s = {k: v[perm] for k, v in s.items()}
    return dict(s=s, vm=vm, K=K, W=W, H=H, kw={}, pixels=None, cap=0.5, groups=groups)


def _rot_z_quat(angle):
    return np.array([np.cos(angle / 2), 0.0, 0.0, np.sin(angle / 2)])


HARD = ("needles", "floaters", "beyond_near", "long_needle")


def hard_scene(name, D=5):
    """The badly conditioned shapes (sampled reference, conditioning-aware bound)."""
    rng = np.random.default_rng(HARD.index(name) + 90)
    f32 = np.float32
    W = H = 256
    vm, K = _cam(np.eye(3), (0.0, 0.0, 0.0), 120.0, 120.0, 128.0, 128.0)
    bg = scene_for_camera(200, D, 95, vm, K, W, H, z=(3.0, 5.0), scale=0.15, sigma=0.3)
    if name == "needles":
        # aspect 1000 .. 2000 at many angles about the view axis, a few tilted out of the image plane
        n = 36
        ang = np.concatenate([np.deg2rad([0, 30, 45, 60, 90, 135] * 5), rng.uniform(0, np.pi, 6)])
        q = np.stack([_rot_z_quat(a) for a in ang])
        q[30:] += rng.normal(0, 0.15, (6, 4))
        new = dict(means=np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.5, 1.5, n), rng.uniform(1.8, 2.5, n)], 1),
                   quats=q, scales=np.stack([rng.uniform(1.0, 2.0, n), np.full(n, 0.001), np.full(n, 0.001)], 1),
                   opacities=rng.uniform(0.5, 0.95, n))
    elif name == "floaters":
        # 12 faint floaters, each wider than the image, in front of 600 Gaussians about a pixel wide
        n = 612
        sc = np.concatenate([rng.uniform(4.0, 10.0, (12, 3)), rng.uniform(0.008, 0.03, (600, 3))])
        zz = np.concatenate([rng.uniform(1.0, 1.5, 12), rng.uniform(2.0, 3.0, 600)])
        uv = rng.uniform(-1.0, 1.0, (n, 2))
        new = dict(means=np.stack([uv[:, 0] * zz, uv[:, 1] * zz, zz], 1), quats=rng.normal(size=(n, 4)), scales=sc,
                   opacities=np.concatenate([rng.uniform(0.05, 0.25, 12), rng.uniform(0.5, 0.99, 600)]))
    elif name == "beyond_near":
        # just past near = 0.01: a scale of 0.003 .. 0.02 is 40 .. 240 px there
        n = 40
        zz = rng.uniform(0.0101, 0.02, n)
        uv = rng.uniform(-1.3, 1.3, (n, 2))
        new = dict(means=np.stack([uv[:, 0] * zz, uv[:, 1] * zz, zz], 1), quats=rng.normal(size=(n, 4)),
                   scales=rng.uniform(0.003, 0.02, (n, 3)), opacities=rng.uniform(0.05, 0.4, n))
    else:
        # one needle at 45 degrees from corner to corner: its box is the whole image, its support a thin diagonal
        new = dict(means=np.array([[0.0, 0.0, 2.0]]), quats=_rot_z_quat(np.pi / 4)[None], scales=np.array([[3.0, 0.002, 0.002]]),
                   opacities=np.array([0.9]))
    new["features"] = rng.normal(0, 1, (len(new["means"]), D))
    s = {k: np.concatenate([new[k].astype(f32), bg[k]]) for k in bg}
    tiles = [(0, 0), (7, 8), (15, 15), (4, 11)]
    return dict(s=s, vm=vm, K=K, W=W, H=H, kw={}, pixels=sample_pixels(W, H, 5, 1500, tiles), cap=0.5, n_new=len(new["means"]))
