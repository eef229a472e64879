"""Seeded meshes and cameras for the mesh rasterizer's tests: closed rooms seen from close to a wall, many tiny faces, one
face over the whole image, the shared-edge and coincident cases.  Everything is generated, nothing is read from disk."""
import numpy as np

ROOM_GRID = 14          # vertices per wall side: 6 walls x 13 x 13 x 2 = 2028 faces
ROOM_SIZE = (5.0, 4.0, 2.6)
ROOM_DISTANCES = (0.05, 0.3, 0.8, 1.5)      # camera to the nearest wall, per seed


def intrinsics(W, H, fx=None, fy=None, cx=None, cy=None):
    fx = 0.85 * W if fx is None else fx
    return np.array([[fx, 0.0, W / 2.0 if cx is None else cx], [0.0, fx if fy is None else fy, H / 2.0 if cy is None else cy],
                     [0.0, 0.0, 1.0]])


def look_at(pos, target, up=(0.0, 0.0, 1.0)):
    """World-to-camera [4,4] f32: x right, y down, z forward."""
    pos, target, up = (np.asarray(v, np.float64) for v in (pos, target, up))
    z = target - pos
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    vm = np.eye(4)
    vm[:3, :3] = np.stack([x, y, z])
    vm[:3, 3] = -vm[:3, :3] @ pos
    return vm.astype(np.float32)


def _wall(origin, du, dv, rng, n=ROOM_GRID):
    """n x n vertices over the rectangle origin + a du + b dv; the inner ones jittered within the wall's plane, the border ones
    exactly on the grid, so that two walls get identical points along the edge they share."""
    a = np.linspace(0.0, 1.0, n)
    A, B = np.meshgrid(a, a, indexing="ij")
    step = 1.0 / (n - 1)
    inner = np.zeros((n, n), bool)
    inner[1:-1, 1:-1] = True
    A = A + inner * rng.uniform(-0.3, 0.3, (n, n)) * step
    B = B + inner * rng.uniform(-0.3, 0.3, (n, n)) * step
    v = origin[None, None] + A[..., None] * du[None, None] + B[..., None] * dv[None, None]
    idx = np.arange(n * n).reshape(n, n)
    q = np.stack([idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]], axis=-1).reshape(-1, 4)
    flip = rng.random(len(q)) < 0.5                                  # either diagonal
    tris = np.where(flip[:, None, None], np.stack([q[:, [0, 1, 3]], q[:, [1, 2, 3]]], axis=1),
                    np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], axis=1)).reshape(-1, 3)
    return v.reshape(-1, 3), tris


def room(seed, size=ROOM_SIZE):
    """A closed room: (verts f32 [6 n^2, 3], faces i32 [2028, 3], vertex_labels u8): six jittered walls, labels in patches."""
    rng = np.random.default_rng(1000 + seed)
    L = np.asarray(size, np.float64)
    e = np.eye(3)
    verts, faces, labels = [], [], []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, 1):
            origin = e[axis] * L[axis] * side
            wv, wt = _wall(origin, e[u] * L[u], e[v] * L[v], rng)
            faces.append(wt + sum(len(x) for x in verts))
            verts.append(wv)
            patch = (np.arange(ROOM_GRID)[:, None] // 5) * 3 + np.arange(ROOM_GRID)[None, :] // 5
            labels.append((patch.reshape(-1) * 7 + 2 * axis + side + rng.integers(0, 2, ROOM_GRID ** 2) * 40) % 200)
    return (np.concatenate(verts).astype(np.float32), np.concatenate(faces).astype(np.int32),
            np.concatenate(labels).astype(np.uint8))


def room_camera(seed, size=ROOM_SIZE):
    """A camera inside the room, ROOM_DISTANCES[seed] from the wall x = 0, looking along that wall and a little towards
    it: the wall behind the image plane crosses the near plane and is seen at a grazing angle."""
    rng = np.random.default_rng(2000 + seed)
    L = np.asarray(size, np.float64)
    pos = np.array([ROOM_DISTANCES[seed % len(ROOM_DISTANCES)], rng.uniform(0.3, 0.7) * L[1], rng.uniform(0.3, 0.7) * L[2]])
    target = pos + np.array([rng.uniform(-0.25, 0.1), rng.choice([-1.0, 1.0]), rng.uniform(-0.3, 0.3)])
    return look_at(pos, target)


def tiny_faces(n=20000, seed=5):
    """n small triangles in front of the identity camera: from far below a pixel to a few pixels across at 64 x 48."""
    rng = np.random.default_rng(seed)
    centre = np.stack([rng.uniform(-2.4, 2.4, n), rng.uniform(-1.8, 1.8, n), rng.uniform(2.0, 6.0, n)], axis=1)
    size = rng.uniform(0.005, 0.25, n)[:, None, None]
    verts = (centre[:, None, :] + rng.normal(size=(n, 3, 3)) * size).reshape(-1, 3).astype(np.float32)
    faces = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    return verts, faces, rng.integers(0, 50, 3 * n).astype(np.uint8)


def whole_image_face():
    """One triangle at z = 3 that covers every sample of any image the identity camera sees."""
    verts = np.array([[-100.0, -100.0, 3.0], [300.0, -100.0, 3.5], [-100.0, 300.0, 2.5]], np.float32)
    return verts, np.array([[0, 1, 2]], np.int32), np.array([7, 9, 9], np.uint8)


def exact_camera():
    """viewmat = identity, fx = fy = 1, cx = cy = 0: a vertex (x, y, 1) projects to the image point (x, y) exactly."""
    return np.eye(4, dtype=np.float32), np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])


def diagonal_quad(swap=False):
    """The square [2, 10]^2 at z = 1, split along the diagonal (2,2)-(10,10), which passes exactly through the samples
    (j + 0.5, j + 0.5); with ``swap`` the two faces change places."""
    verts = np.array([[2, 2, 1], [10, 2, 1], [10, 10, 1], [2, 10, 1]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    return verts, faces[::-1].copy() if swap else faces, np.array([1, 2, 2, 4], np.uint8)


def coincident_faces():
    """The same triangle twice (once wound the other way): the lower face index wins every sample."""
    verts = np.array([[1, 1, 2], [11, 2, 2], [3, 11, 2]], np.float32) * np.array([2, 2, 1], np.float32)
    return verts, np.array([[0, 1, 2], [0, 2, 1]], np.int32), np.array([5, 5, 6], np.uint8)
