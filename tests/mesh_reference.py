"""The mesh rasterizer's contract in NumPy (include/voxproj_mesh.h repeats it; the kernels of csrc/vp_mesh.h replay it bit
for bit) and a brute-force float64 ray caster to judge the contract itself against.

render() is the twin: float64 arithmetic on the fp32 inputs in exactly the written order (Python floats and NumPy element-wise
operations: IEEE double, no contraction), int64 (Python integers) for everything that decides coverage.  ray_cast() shares
nothing with it but the camera: Moller-Trumbore on the pixel-centre rays against the unclipped, unsnapped triangles."""
import math

import numpy as np

GUARD = 2.0 ** 29
NOTHING_ID, NOTHING_LABEL = -1, 255


def camera_f32(viewmat, K):
    """What the library sees: the pose and fx, fy, cx, cy rounded to fp32, as Python floats."""
    vm = np.asarray(viewmat, np.float64).astype(np.float32).astype(np.float64).reshape(4, 4)
    k = np.asarray(K, np.float64)
    fx, fy, cx, cy = (float(np.float32(v)) for v in (k[0, 0], k[1, 1], k[0, 2], k[1, 2]))
    return vm, fx, fy, cx, cy


def camera_space(verts, vm):
    """c[k] = ((R[k][0] x + R[k][1] y) + R[k][2] z) + t[k] in float64, [V,3]."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.stack([((vm[k, 0] * v[:, 0] + vm[k, 1] * v[:, 1]) + vm[k, 2] * v[:, 2]) + vm[k, 3] for k in range(3)], axis=1)


def face_labels(faces, vertex_labels):
    """The majority of a face's three vertex labels, the smallest when all differ (np.bincount(t).argmax())."""
    t = np.asarray(vertex_labels, np.uint8)[np.asarray(faces)]
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    return np.where((a == b) | (a == c), a, np.where(b == c, b, np.minimum(a, np.minimum(b, c)))).astype(np.uint8)


def _snap(x, y, z, fx, fy, cx, cy):
    """(X, Y) in 1/256 pixel, or None when a coordinate is not finite or beyond the guard band."""
    sx, sy = (fx * (x / z) + cx) * 256.0 + 0.5, (fy * (y / z) + cy) * 256.0 + 0.5
    if not (math.isfinite(sx) and math.isfinite(sy)):
        return None
    sx, sy = math.floor(sx), math.floor(sy)
    if abs(sx) > GUARD or abs(sy) > GUARD:
        return None
    return sx, sy


def clip_and_snap(c, near, fx, fy, cx, cy):
    """The face's sub-triangles as lists of three snapped points (positive area), or 'guard'.  c: its three camera-space
    vertices as Python floats; at least one has z >= near."""
    inside = [p[2] >= near for p in c]
    pts = []
    for e in range(3):
        a, b = c[e], c[(e + 1) % 3]
        if inside[e]:
            pts.append(a)
        if inside[e] != inside[(e + 1) % 3]:
            s, o = (a, b) if inside[e] else (b, a)          # always from the inside end to the outside end
            tt = (near - s[2]) / (o[2] - s[2])
            pts.append((s[0] + tt * (o[0] - s[0]), s[1] + tt * (o[1] - s[1]), near))
    q = [_snap(p[0], p[1], p[2], fx, fy, cx, cy) for p in pts]
    if any(p is None for p in q):
        return "guard"
    subs = []
    for tri in ([q[0], q[1], q[2]],) + (([q[0], q[2], q[3]],) if len(q) == 4 else ()):
        (x0, y0), (x1, y1), (x2, y2) = tri
        area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
        if area == 0:
            continue
        subs.append(tri if area > 0 else [tri[0], tri[2], tri[1]])
    return subs


def _covered(tri, j0, j1, i0, i1):
    """Coverage of the pixels [j0, j1] x [i0, i1] by one positively oriented sub-triangle: bool [i1-i0+1, j1-j0+1]."""
    PX = (256 * np.arange(j0, j1 + 1, dtype=np.int64) + 128)[None, :]
    PY = (256 * np.arange(i0, i1 + 1, dtype=np.int64) + 128)[:, None]
    cov = np.ones((i1 - i0 + 1, j1 - j0 + 1), bool)
    for e in range(3):
        (ax, ay), (bx, by) = tri[e], tri[(e + 1) % 3]
        dx, dy = bx - ax, by - ay
        E = dx * (PY - ay) - dy * (PX - ax)                  # below 2^61: int64 is exact
        cov &= (E >= 0) if (dy < 0 or (dy == 0 and dx > 0)) else (E > 0)
    return cov


def render(verts, faces, vertex_labels, viewmat, K, W, H, near=0.01, far=100.0, want_cover=False):
    """The twin: dict(face_ids i32 [H,W], depth f32 [H,W], labels u8 [H,W] or None, counters i32 [3] = {bad index,
    non-finite, guard band}; with want_cover also cover i32 [H,W]: how many faces took the sample before the depth test)."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    vm, fx, fy, cx, cy = camera_f32(viewmat, K)
    near, far = float(np.float32(near)), float(np.float32(far))
    cam = camera_space(verts, vm)
    finite = np.isfinite(verts).all(axis=1)
    ids = np.full((H, W), NOTHING_ID, np.int32)
    best = np.full((H, W), np.inf, np.float32)
    cover = np.zeros((H, W), np.int32)
    counters = np.zeros(3, np.int32)
    rx_all = ((np.arange(W, dtype=np.float64) + 0.5) - cx) / fx
    ry_all = ((np.arange(H, dtype=np.float64) + 0.5) - cy) / fy
    for f, idx in enumerate(faces.tolist()):
        if any(i < 0 or i >= len(verts) for i in idx):
            counters[0] += 1
            continue
        if not finite[idx].all():
            counters[1] += 1
            continue
        c = [tuple(float(v) for v in cam[i]) for i in idx]
        if not any(p[2] >= near for p in c):
            continue
        subs = clip_and_snap(c, near, fx, fy, cx, cy)
        if subs == "guard":
            counters[2] += 1
            continue
        (c0, c1, c2) = c
        ax, ay, az = c1[0] - c0[0], c1[1] - c0[1], c1[2] - c0[2]
        bx, by, bz = c2[0] - c0[0], c2[1] - c0[1], c2[2] - c0[2]
        nx, ny, nz = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
        d = (nx * c0[0] + ny * c0[1]) + nz * c0[2]
        zmin, zmax = min(c0[2], c1[2], c2[2]), max(c0[2], c1[2], c2[2])
        for tri in subs:
            xs, ys = [p[0] for p in tri], [p[1] for p in tri]
            j0, j1 = max((min(xs) + 127) >> 8, 0), min((max(xs) - 128) >> 8, W - 1)
            i0, i1 = max((min(ys) + 127) >> 8, 0), min((max(ys) - 128) >> 8, H - 1)
            if j0 > j1 or i0 > i1:
                continue
            cov = _covered(tri, j0, j1, i0, i1)
            if not cov.any():
                continue
            with np.errstate(all="ignore"):
                zr = d / ((nx * rx_all[None, j0:j1 + 1] + ny * ry_all[i0:i1 + 1, None]) + nz)
                z = np.minimum(np.maximum(zr, zmin), zmax)
                keep = cov & ~np.isnan(zr) & (z >= near) & (z <= far)
                zf = np.where(keep, z, np.inf).astype(np.float32)
            cover[i0:i1 + 1, j0:j1 + 1] += keep
            win = keep & (zf < best[i0:i1 + 1, j0:j1 + 1])            # strict: the lower face index keeps a tie
            best[i0:i1 + 1, j0:j1 + 1][win] = zf[win]
            ids[i0:i1 + 1, j0:j1 + 1][win] = f
    drawn = ids >= 0
    out = dict(face_ids=ids, depth=np.where(drawn, best, np.float32(0)).astype(np.float32), labels=None, counters=counters)
    if vertex_labels is not None:
        fl = face_labels(np.where((faces < 0) | (faces >= len(verts)), 0, faces), vertex_labels) if len(faces) else np.zeros(0, np.uint8)
        out["labels"] = np.where(drawn, fl[np.maximum(ids, 0)] if len(fl) else 0, NOTHING_LABEL).astype(np.uint8)
    if want_cover:
        out["cover"] = cover
    return out


def ray_cast(verts, faces, viewmat, K, W, H, near=0.01, far=100.0, eps=1e-9, chunk=512):
    """Brute force in float64: every pixel-centre ray against every triangle (Moller-Trumbore, both sides, barycentric
    tolerance eps so that no ray slips between two triangles), nearest z in [near, far].  (face_ids i32, depth f64; -1 / inf
    where no triangle is hit)."""
    vm, fx, fy, cx, cy = camera_f32(viewmat, K)
    cam = camera_space(verts, vm)
    faces = np.asarray(faces)
    v0, v1, v2 = cam[faces[:, 0]], cam[faces[:, 1]], cam[faces[:, 2]]
    e1, e2 = v1 - v0, v2 - v0
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    dirs = np.stack([((jj + 0.5) - cx) / fx, ((ii + 0.5) - cy) / fy, np.ones_like(jj, np.float64)], axis=-1).reshape(-1, 3)
    ids = np.full(len(dirs), -1, np.int32)
    depth = np.full(len(dirs), np.inf)
    for s in range(0, len(dirs), chunk):
        dch = dirs[s:s + chunk][:, None, :]                           # [P,1,3]; the origin is the camera centre
        pv = np.cross(dch, e2[None])
        det = (e1[None] * pv).sum(-1)
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            tv = -v0[None]
            u = (tv * pv).sum(-1) * inv
            qv = np.cross(tv, e1[None])
            v = (dch * qv).sum(-1) * inv
            t = (e2[None] * qv).sum(-1) * inv                          # dir.z = 1: t is the depth
            hit = (np.abs(det) > 0) & (u >= -eps) & (v >= -eps) & (u + v <= 1 + eps) & (t >= near) & (t <= far)
        t = np.where(hit, t, np.inf)
        k = t.argmin(axis=1)
        tk = t[np.arange(len(k)), k]
        ids[s:s + chunk] = np.where(np.isfinite(tk), k, -1)
        depth[s:s + chunk] = tk
    return ids.reshape(H, W), depth.reshape(H, W)
