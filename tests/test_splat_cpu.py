"""CPU tests of the Gaussian splatting path: known answers of the float64 oracle (tests/splat_reference.py), the support
half-extents, the 3DGS PLY reader, render_semantics_logits.py's padding / size / camera / palette rules, and the host-side
refusals of vp_splat_* and voxproj_host's splat wrappers (fake device pointers, never dereferenced)."""
import ctypes
import os

import numpy as np
import pytest

import splat_reference as ref

FAKE = 0x7000_0000_0000
WS = 0x7100_0000_0000             # 256-byte aligned
ID = np.eye(4, dtype=np.float32)


def K_(f, W, H):
    return np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], np.float32)


def one(mu, s, o, f, q=(1, 0, 0, 0)):
    return dict(means=np.array([mu], np.float32), quats=np.array([q], np.float32), scales=np.array([s], np.float32),
                opacities=np.array([o], np.float32), features=np.array([f], np.float32))


def cat(*gs):
    return {k: np.concatenate([g[k] for g in gs]) for k in gs[0]}


def render(g, W=9, H=9, f=10.0, **kw):
    return ref.splat64(g["means"], g["quats"], g["scales"], g["opacities"], g["features"], ID, K_(f, W, H), W, H, **kw)


def closed_alpha(W, H, f, z, s, o, eps2d=0.3):
    v = (f * s / z) ** 2 + eps2d
    jj, ii = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    d2 = (jj - W / 2) ** 2 + (ii - H / 2) ** 2
    a = np.minimum(0.999, o * np.exp(-d2 / (2 * v)))
    return np.where(a >= 1 / 255, a, 0.0)


def test_single_isotropic_gaussian_closed_form():
    g = one((0, 0, 2.0), (0.1, 0.1, 0.1), 0.7, [1.0])
    r = render(g, W=15, H=11)
    a = closed_alpha(15, 11, 10.0, 2.0, 0.1, 0.7)
    assert np.abs(r["alpha"] - a).max() < 1e-6
    assert np.abs(r["logits"][0] - a).max() < 1e-6
    assert (r["visits"] == (a > 0)).all() and (a > 0).sum() > 20


@pytest.mark.parametrize("front", [0, 1])
def test_two_gaussians_both_depth_orders(front):
    z = (2.0, 3.0) if front == 0 else (3.0, 2.0)
    g = cat(one((0, 0, z[0]), (0.2,) * 3, 0.6, [1.0, 0.0]), one((0, 0, z[1]), (0.2,) * 3, 0.5, [0.0, 1.0]))
    r = render(g)
    a0 = closed_alpha(9, 9, 10.0, z[0], 0.2, 0.6)
    a1 = closed_alpha(9, 9, 10.0, z[1], 0.2, 0.5)
    af, ab = (a0, a1) if front == 0 else (a1, a0)
    # the front one is added with T = 1, the back one behind it
    exp_front = af
    exp_back = ab * (1 - af)
    got = r["logits"][front], r["logits"][1 - front]
    assert np.abs(got[0] - exp_front).max() < 1e-6 and np.abs(got[1] - exp_back).max() < 1e-6
    assert (r["label"][4, 4] == front)


def test_saturation_stops_before_the_crossing_gaussian():
    # alpha 0.98 at the centre pixel: T = 0.02, 4e-4, then 8e-6 <= 1e-4 -> the third is not added
    gs = [one((0, 0, 2.0 + k), (0.3,) * 3, 0.98, np.eye(3)[k]) for k in range(3)]
    g = cat(*gs)
    W = H = 9
    # mean2d lands on (4.5, 4.5), the centre pixel's sample: sigma = 0 there
    r = render(g, W=W, H=H)
    c = r["logits"][:, 4, 4]
    assert r["visits"][4, 4] == 2
    assert abs(c[0] - 0.98) < 1e-6 and abs(c[1] - 0.98 * 0.02) < 1e-6 and c[2] == 0.0
    assert abs(r["alpha"][4, 4] - (1 - 0.02 * 0.02)) < 1e-9


def test_behind_near_plane_and_faint_gaussians_reach_nothing():
    for g in (one((0, 0, 0.005), (0.1,) * 3, 0.9, [1.0]), one((0, 0, -1.0), (0.1,) * 3, 0.9, [1.0]),
              one((0, 0, 2.0), (0.3,) * 3, 0.0039, [1.0]), one((0, 0, 2.0), (0.3,) * 3, 0.9, [1.0], q=(0, 0, 0, 0))):
        r = render(g)
        assert (r["visits"] == 0).all() and (r["alpha"] == 0).all() and (r["label"] == 0).all()


def test_equal_depths_resolved_by_index():
    g = cat(one((0, 0, 2.0), (0.2,) * 3, 0.6, [1.0, 0.0]), one((0.001, 0, 2.0), (0.2,) * 3, 0.6, [0.0, 1.0]))
    assert ref.depth32(g["means"], ID)[0] == ref.depth32(g["means"], ID)[1]
    r = render(g)
    # index 0 first: its weight is alpha0 (T = 1), index 1 gets alpha1 * (1 - alpha0) < alpha0 at the centre
    assert r["logits"][0, 4, 4] > r["logits"][1, 4, 4] and list(r["order"]) == [0, 1]
    g2 = {k: v[::-1].copy() for k, v in g.items()}
    r2 = render(g2)
    assert r2["logits"][1, 4, 4] > r2["logits"][0, 4, 4]


def test_half_extents_bound_the_support():
    rng = np.random.default_rng(0)
    for _ in range(200):
        a, c = rng.uniform(0.3, 40, 2)
        b = rng.uniform(-0.95, 0.95) * np.sqrt(a * c)
        o = rng.uniform(1 / 255, 1.0)
        cov = np.array([a, b, c])
        rx, ry = ref.half_extents(o, cov)
        det = a * c - b * b
        A, B, C = c / det, -b / det, a / det
        xs = np.linspace(-3 * rx - 1, 3 * rx + 1, 301)
        ys = np.linspace(-3 * ry - 1, 3 * ry + 1, 301)
        dx, dy = np.meshgrid(xs, ys)
        sig = 0.5 * (A * dx * dx + C * dy * dy) + B * dx * dy
        inside = o * np.exp(-sig) >= 1 / 255
        assert inside.any()
        assert (np.abs(dx[inside]) <= rx * (1 + 1e-9)).all() and (np.abs(dy[inside]) <= ry * (1 + 1e-9)).all()


def test_fragile_mask_flags_threshold_pixels():
    # opacity exactly at the clamp: every reached pixel's raw alpha at the centre sits on 0.999
    g = one((0, 0, 2.0), (0.2,) * 3, 0.999, [1.0, 0.5])
    r = render(g)
    assert r["fragile"][4, 4] and not r["fragile"][0, 0]


def test_ply_round_trip(tmp_path):
    from gaussian_ply import read_gaussian_ply, write_gaussian_ply
    rng = np.random.default_rng(1)
    n = 57
    mu = rng.normal(size=(n, 3)).astype(np.float32)
    op = rng.normal(size=n).astype(np.float32)
    ls = rng.normal(-3, 1, size=(n, 3)).astype(np.float32)
    rot = rng.normal(size=(n, 4)).astype(np.float32)
    p = str(tmp_path / "point_cloud.ply")
    write_gaussian_ply(p, mu, op, ls, rot, f_dc=rng.normal(size=(n, 3)))
    g = read_gaussian_ply(p)
    assert np.array_equal(g["means"], mu)
    assert np.allclose(g["opacities"], 1 / (1 + np.exp(-op.astype(np.float64))), rtol=1e-6)
    assert np.allclose(g["scales"], np.exp(ls.astype(np.float64)), rtol=1e-6)
    assert np.allclose(g["quats"], rot / np.linalg.norm(rot.astype(np.float64), axis=1, keepdims=True), atol=1e-7)
    with open(p, "rb") as f:
        data = f.read()
    bad = str(tmp_path / "ascii.ply")
    with open(bad, "wb") as f:
        f.write(data.replace(b"binary_little_endian", b"ascii", 1))
    with pytest.raises(ValueError, match="binary_little_endian"):
        read_gaussian_ply(bad)


def test_cli_padding_size_camera_palette(tmp_path):
    import render_semantics_logits as rsl
    from PIL import Image
    from query_reference import palette as palette_ref
    lg = np.arange(26, dtype=np.float32).reshape(2, 13)
    p = rsl.pad_logits(lg)
    assert p.shape == (2, 32) and (p[:, :13] == lg).all() and (p[:, 13:] == 0).all()
    wide = np.ones((3, 40), np.float32)
    assert rsl.pad_logits(wide).shape == (3, 32) and rsl.pad_logits(wide, 8).shape == (3, 8)
    assert rsl.render_size(1752, 1168) == (1600, 1066)
    assert rsl.render_size(876, 584) == (876, 584)
    assert rsl.render_size(1752, 1168, 0.5) == (876, 584)
    entry = {"R": np.eye(3).tolist(), "tvec": [1.0, 2.0, 3.0], "camera_id": 1}
    cams = {"1": {"params": [600.0, 610.0, 870.0, 580.0]}}
    vm, K = rsl.camera(entry, cams, 1752, 1168, 876, 584)
    assert np.allclose(K, [[300, 0, 438], [0, 305, 292], [0, 0, 1]]) and np.allclose(vm[:3, 3], [1, 2, 3])
    _, Kc = rsl.camera(entry, cams, 1752, 1168, 876, 584, principal_point="camera")
    assert np.allclose(Kc[:2, 2], [435, 290])
    lab = (np.arange(60).reshape(6, 10) % 15).astype(np.uint8)
    png = str(tmp_path / "00000_mask_color.png")
    rsl.save_palette_png(png, lab, 13)
    im = Image.open(png)
    assert im.mode == "P" and np.array_equal(np.asarray(im), lab)
    assert im.getpalette()[:39] == palette_ref(13).reshape(-1).tolist()
    args = rsl.build_parser().parse_args(["--gaussians_ply", "a", "--logit_path", "b", "--cam_params", "c"])
    assert args.channels == 32 and args.principal_point == "center" and args.downsample_factor is None and not args.no_logits


@pytest.fixture(scope="module")
def lib():
    import voxproj_host
    voxproj_host.build()
    return voxproj_host.lib()


def _proj(lib, n=10, means=FAKE, viewmat=None, fx=100.0, fy=100.0, W=64, H=48, near=0.01, far=1e10, eps=0.3, ws=WS,
          ws_bytes=None):
    vp = ctypes.c_void_p
    vm = (ctypes.c_float * 16)(*np.eye(4).reshape(-1)) if viewmat is None else viewmat
    if ws_bytes is None:
        ws_bytes = lib.vp_splat_workspace_bytes(max(n, 0), W, H, 0) or (1 << 30)
    return lib.vp_splat_project(vp(means), vp(FAKE), vp(FAKE), vp(FAKE), n, vm, fx, fy, 32.0, 24.0, W, H, near, far, eps,
                                None, None, vp(ws), ws_bytes, None)


@pytest.mark.parametrize("kw,code,msg", [
    (dict(n=-1), -1, b"n_gaussians"),
    (dict(n=1 << 31), -1, b"n_gaussians"),
    (dict(means=0), -1, b"null pointer"),
    (dict(W=0), -1, b"image"),
    (dict(H=40000), -1, b"image"),
    (dict(fx=0.0), -1, b"fx, fy"),
    (dict(fy=float("nan")), -1, b"fx, fy"),
    (dict(near=0.0), -1, b"near"),
    (dict(far=0.001), -1, b"near"),
    (dict(eps=-1.0), -1, b"eps2d"),
    (dict(viewmat=(ctypes.c_float * 16)(*([float("inf")] + [0.0] * 15))), -1, b"viewmat[0]"),
    (dict(ws=0), -2, b"workspace is NULL"),
    (dict(ws=WS + 16), -2, b"256-byte aligned"),
])
def test_project_refusals(lib, kw, code, msg):
    assert _proj(lib, **kw) == code
    assert msg in lib.vp_last_error()


def _rast(lib, feats=FAKE, D=32, stride=32, n=10, W=64, H=48, cap=100, labels=FAKE, ws=WS, ws_bytes=None):
    vp = ctypes.c_void_p
    if ws_bytes is None:
        ws_bytes = lib.vp_splat_workspace_bytes(max(n, 0), W, H, max(cap, 0)) or (1 << 30)
    return lib.vp_splat_rasterize(vp(feats), D, stride, n, W, H, cap, vp(labels), None, None, None, None, vp(ws), ws_bytes,
                                  None)


@pytest.mark.parametrize("kw,code,msg", [
    (dict(labels=0), -1, b"null pointer"),
    (dict(feats=0), -1, b"null pointer"),
    (dict(D=0, stride=0), -1, b"D = 0"),
    (dict(D=65, stride=65), -1, b"D = 65"),
    (dict(stride=31), -1, b"row_stride"),
    (dict(cap=-1), -1, b"capacity"),
    (dict(W=33000), -1, b"image"),
    (dict(n=-2), -1, b"n_gaussians"),
    (dict(ws=0), -2, b"workspace is NULL"),
    (dict(ws=WS + 64), -2, b"256-byte aligned"),
])
def test_rasterize_refusals(lib, kw, code, msg):
    assert _rast(lib, **kw) == code
    assert msg in lib.vp_last_error()


def test_workspace_bytes_refusals(lib):
    # the sizes themselves need the device (rocPRIM's scratch): test_gpu_splat.py checks them
    for args in ((-1, 64, 48, 0), (1000, 0, 48, 0), (1000, 64, 40000, 0), (1000, 64, 48, -1), (1 << 31, 64, 48, 0)):
        assert lib.vp_splat_workspace_bytes(*args) == 0


def test_symbols_in_exports_and_header():
    import voxproj_host
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "voxproj.h")).read()
    for name in ("vp_splat_workspace_bytes", "vp_splat_project", "vp_splat_rasterize"):
        assert name in voxproj_host.EXPORTS and f" {name}(" in hdr
    assert voxproj_host.VP_ABI_VERSION == 4


def test_python_refusals_before_device_work():
    import torch
    import voxproj_host
    m = torch.zeros(4, 3)
    q = torch.zeros(4, 4)
    s = torch.zeros(4, 3)
    o = torch.zeros(4)
    f = torch.zeros(4, 8)
    vm, K = np.eye(4), K_(10, 16, 16)
    with pytest.raises(ValueError, match="CUDA tensor"):
        voxproj_host.splat_features(m, q, s, o, f, vm, K, 16, 16)
    with pytest.raises(ValueError, match="float32"):
        voxproj_host.splat_features(m, q, s, o, f.double(), vm, K, 16, 16)
    with pytest.raises(ValueError, match="D = 65"):
        voxproj_host.splat_features(m, q, s, o, torch.zeros(4, 65), vm, K, 16, 16)
    with pytest.raises(ValueError, match="one row per Gaussian"):
        voxproj_host.splat_features(m, q, s, o, torch.zeros(5, 8), vm, K, 16, 16)
    with pytest.raises(ValueError, match="float32"):
        voxproj_host.splat_project(m.half(), q, s, o, vm, K, 16, 16)
