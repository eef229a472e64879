"""Synthetic 3D Gaussian scenes for the splatting path (vp_splat_*, render_semantics_logits.py): Gaussians on the surfaces of a
room (floor, ceiling, four walls) and on a few boxes standing on the floor, cameras from synthetic_scene.make_trajectory.

Every Gaussian has a class: the surface or box it lies on (mod n_classes).  Its logits are label-correlated: a gain on its
own class plus Gaussian noise, so rendered labels form regions.  Scales are log-normal (a flattened axis along the surface
normal), opacities mixed (a fifth nearly transparent, some below 1/255), quaternions random.
"""
import json
import os

import numpy as np

from synthetic_scene import DSLR, _look_at, make_trajectory


def make_gaussians(n, room=(6.0, 5.0, 2.8), n_classes=13, seed=0, scale_median=0.025):
    """dict(means f32 [n,3], quats f32 [n,4] (unit), scales f32 [n,3], opacities f32 [n], classes int64 [n], room)."""
    rng = np.random.default_rng(seed)
    a, b, c = room
    # surfaces: (origin, u axis, v axis, normal); the boxes' tops and sides follow
    surf = [((0, 0, 0), (a, 0, 0), (0, b, 0), (0, 0, 1)), ((0, 0, c), (a, 0, 0), (0, b, 0), (0, 0, -1)),
            ((0, 0, 0), (a, 0, 0), (0, 0, c), (0, 1, 0)), ((0, b, 0), (a, 0, 0), (0, 0, c), (0, -1, 0)),
            ((0, 0, 0), (0, b, 0), (0, 0, c), (1, 0, 0)), ((a, 0, 0), (0, b, 0), (0, 0, c), (-1, 0, 0))]
    for k in range(6):
        x0, y0 = rng.uniform(0.15, 0.75) * a, rng.uniform(0.15, 0.75) * b
        w, d, h = rng.uniform(0.3, 0.8), rng.uniform(0.3, 0.8), rng.uniform(0.3, 1.0)
        surf += [((x0, y0, h), (w, 0, 0), (0, d, 0), (0, 0, 1)), ((x0, y0, 0), (w, 0, 0), (0, 0, h), (0, -1, 0)),
                 ((x0, y0, 0), (0, d, 0), (0, 0, h), (-1, 0, 0))]
    surf = [tuple(np.asarray(v, np.float64) for v in s) for s in surf]
    area = np.array([np.linalg.norm(np.cross(s[1], s[2])) for s in surf])
    which = rng.choice(len(surf), size=n, p=area / area.sum())
    uv = rng.uniform(0.0, 1.0, size=(n, 2))
    o = np.stack([surf[k][0] for k in which])
    u = np.stack([surf[k][1] for k in which])
    v = np.stack([surf[k][2] for k in which])
    nrm = np.stack([surf[k][3] for k in which])
    means = o + uv[:, :1] * u + uv[:, 1:] * v + nrm * rng.normal(0.0, 0.005, size=(n, 1))
    classes = np.where(which < 6, which, 6 + (which - 6) // 3) % n_classes
    scales = scale_median * np.exp(rng.normal(0.0, 0.6, size=(n, 3)))
    scales[:, 2] *= 0.2
    quats = rng.normal(size=(n, 4))
    quats /= np.linalg.norm(quats, axis=1, keepdims=True)
    op = np.where(rng.uniform(size=n) < 0.2, rng.uniform(0.001, 0.05, size=n), rng.uniform(0.3, 0.99, size=n))
    return dict(means=means.astype(np.float32), quats=quats.astype(np.float32), scales=scales.astype(np.float32),
                opacities=op.astype(np.float32), classes=classes.astype(np.int64), room=room)


def make_logits(classes, n_classes, seed=0, gain=3.0, noise=1.0):
    """f32 [n, n_classes]: gain on each Gaussian's class plus N(0, noise)."""
    rng = np.random.default_rng(seed + 101)
    lg = rng.normal(0.0, noise, size=(len(classes), n_classes))
    lg[np.arange(len(classes)), classes] += gain
    return lg.astype(np.float32)


def make_views(n_views, room, width, seed=0):
    """(w2c f64 [V,4,4] world-to-camera, K f64 [3,3]): trajectory cameras; the DSLR's intrinsics scaled to ``width``."""
    P, F = make_trajectory(n_views, room, seed=seed)
    w2c = np.stack([np.linalg.inv(_look_at(p, f)) for p, f in zip(P, F)])
    s = width / DSLR["w"]
    K = np.array([[DSLR["fx"] * s, 0.0, DSLR["cx"] * s], [0.0, DSLR["fy"] * s, DSLR["cy"] * s], [0.0, 0.0, 1.0]])
    return w2c, K


def write_camera_params(path, w2c, K, width, height, names=None):
    """The project's camera_params.json (images {i: name, camera_id, R, tvec}, cameras {1: params fx fy cx cy, width,
    height}) for the views ``w2c``; names default to DSC00000.JPG, ..."""
    names = names or [f"DSC{v:05d}.JPG" for v in range(len(w2c))]
    images = {str(v): {"name": nm, "camera_id": 1, "R": w2c[v][:3, :3].tolist(), "tvec": w2c[v][:3, 3].tolist()}
              for v, nm in enumerate(names)}
    cams = {"1": {"params": [float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])], "width": int(width),
                  "height": int(height)}}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"images": images, "cameras": cams}, f)
    return names


def to_ply_fields(g):
    """(opacity logits, log scales, rotations) of a make_gaussians scene: the raw values a 3DGS .ply stores."""
    op = np.clip(g["opacities"].astype(np.float64), 1e-7, 1 - 1e-7)
    return np.log(op / (1 - op)), np.log(g["scales"].astype(np.float64)), g["quats"]

