"""CPU tests of the splatting backward: the float64 gradient reference (tests/splat_grad_reference.py) against central finite
differences of the float64 forward, and the host-side refusals of vp_splat_backward_workspace_bytes /
vp_splat_rasterize_backward and of the Python entry points (fake device pointers, never dereferenced)."""
import ctypes
import os

import numpy as np
import pytest

import splat_grad_reference as gref
import splat_reference as ref

FAKE = 0x7000_0000_0000
WS = 0x7100_0000_0000             # 256-byte aligned
BWS = 0x7200_0000_0000
ID = np.eye(4, dtype=np.float32)


def K_(f, W, H):
    return np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], np.float32)


def small_scene(n, D, seed, W=20, H=16):
    rng = np.random.default_rng(seed)
    means = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.4, 0.4, n), rng.uniform(1.5, 3.0, n)], 1)
    s = dict(means=means.astype(np.float32), quats=rng.normal(size=(n, 4)).astype(np.float32),
             scales=(0.15 * np.exp(rng.normal(0, 0.3, (n, 3)))).astype(np.float32),
             opacities=rng.uniform(0.3, 0.9, n).astype(np.float32), features=rng.normal(size=(n, D)))
    G = rng.normal(size=(D, H, W))
    Ga = rng.normal(size=(H, W))
    return s, K_(12.0, W, H), W, H, G, Ga


def args(s):
    return s["means"], s["quats"], s["scales"], s["opacities"], s["features"]


@pytest.mark.parametrize("seed", [0, 1])
def test_feature_gradient_is_exact(seed):
    # the logits are linear in the features: a central difference of any step is exact up to rounding
    s, K, W, H, G, Ga = small_scene(6, 3, seed)
    r = gref.splat_grad64(*args(s), ID, K, W, H, G=G, G_alpha=Ga)
    assert (r["added"] > 0).sum() >= 4
    fd = np.zeros_like(r["grad_f"])
    for g in range(6):
        for c in range(3):
            hi, lo = dict(s), dict(s)
            hi["features"] = s["features"].copy()
            lo["features"] = s["features"].copy()
            hi["features"][g, c] += 1.0
            lo["features"][g, c] -= 1.0
            fd[g, c] = (gref.loss64(*args(hi), ID, K, W, H, G, Ga) - gref.loss64(*args(lo), ID, K, W, H, G, Ga)) / 2.0
    assert np.abs(fd - r["grad_f"]).max() <= 1e-9 * (1 + np.abs(fd).max())
    assert (np.abs(r["grad_f"]) > 1e-3).sum() >= 10


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_opacity_gradient_finite_differences(seed):
    # pixels with a decision within 1 % of its threshold get no upstream gradient, so a step of 2^-12 cannot flip one
    s, K, W, H, G, Ga = small_scene(6, 3, seed)
    frag = gref.splat_grad64(*args(s), ID, K, W, H, G=G, G_alpha=Ga, fragile_rel=1e-2)["fragile"]
    G[:, frag] = 0.0
    Ga[frag] = 0.0
    assert (~frag).sum() >= 0.5 * W * H
    r = gref.splat_grad64(*args(s), ID, K, W, H, G=G, G_alpha=Ga)
    h = 2.0 ** -12
    fd = np.zeros(6)
    for g in range(6):
        hi, lo = dict(s), dict(s)
        hi["opacities"] = s["opacities"].copy()
        lo["opacities"] = s["opacities"].copy()
        hi["opacities"][g] += np.float32(h)
        lo["opacities"][g] -= np.float32(h)
        fd[g] = (gref.loss64(*args(hi), ID, K, W, H, G, Ga) - gref.loss64(*args(lo), ID, K, W, H, G, Ga)) / (2 * h)
    assert np.abs(fd - r["grad_o"]).max() <= 1e-5 * (r["M_o"].max() + 1e-12), (fd, r["grad_o"])
    assert (np.abs(r["grad_o"]) > 1e-3 * np.abs(r["grad_o"]).max()).sum() >= 4


def test_alpha_only_and_logits_only_add_up():
    s, K, W, H, G, Ga = small_scene(6, 3, 5)
    both = gref.splat_grad64(*args(s), ID, K, W, H, G=G, G_alpha=Ga)
    lo = gref.splat_grad64(*args(s), ID, K, W, H, G=G)
    al = gref.splat_grad64(*args(s), ID, K, W, H, G_alpha=Ga)
    assert np.allclose(lo["grad_o"] + al["grad_o"], both["grad_o"], rtol=1e-12, atol=1e-12)
    assert (al["grad_f"] == 0).all() and np.array_equal(lo["grad_f"], both["grad_f"])


def test_behind_the_stop_and_at_the_clamp():
    # three opaque Gaussians on the axis: the third is behind the stop at the centre; the front one's opacity is clamped
    def one(z, o, f):
        return dict(means=np.array([[0, 0, z]], np.float32), quats=np.array([[1, 0, 0, 0]], np.float32),
                    scales=np.array([[0.3] * 3], np.float32), opacities=np.array([o], np.float32),
                    features=np.array([f], np.float64))
    gs = [one(2.0, 0.98, [1, 0, 0]), one(3.0, 0.98, [0, 1, 0]), one(4.0, 0.98, [0, 0, 1])]
    s = {k: np.concatenate([g[k] for g in gs]) for k in gs[0]}
    W = H = 9
    G = np.zeros((3, H, W))
    G[:, 4, 4] = 1.0
    r = gref.splat_grad64(*args(s), ID, K_(10.0, W, H), W, H, G=G, G_alpha=np.ones((H, W)))
    assert r["visits"][4, 4] == 2
    assert r["grad_f"][2, 2] == 0.0 and r["grad_f"][0, 0] == pytest.approx(0.98) and r["grad_f"][1, 1] == pytest.approx(0.98 * 0.02)
    s["opacities"][0] = 1.0                              # raw alpha above 0.999 at the centre: da/do = 0 there
    G2 = np.zeros((3, H, W))
    G2[:, 4, 4] = 1.0
    r2 = gref.splat_grad64(*args(s), ID, K_(10.0, W, H), W, H, G=G2)
    assert r2["grad_o"][0] == 0.0


@pytest.fixture(scope="module")
def lib():
    import voxproj_host
    voxproj_host.build()
    return voxproj_host.lib()


def _bwd(lib, feats=FAKE, D=32, stride=32, n=10, W=64, H=48, cap=100, ws=WS, ws_bytes=1 << 30, bws=BWS, bws_bytes=None):
    vp = ctypes.c_void_p
    if bws_bytes is None:
        bws_bytes = lib.vp_splat_backward_workspace_bytes(max(cap, 0), D) or (1 << 30)
    return lib.vp_splat_rasterize_backward(vp(feats), D, stride, n, W, H, cap, vp(FAKE), None, vp(FAKE), vp(FAKE), None,
                                           vp(ws), ws_bytes, vp(bws), bws_bytes, None)


@pytest.mark.parametrize("kw,code,msg", [
    (dict(feats=0), -1, b"null pointer"),
    (dict(D=0, stride=0), -1, b"D = 0"),
    (dict(D=65, stride=65), -1, b"D = 65"),
    (dict(stride=31), -1, b"row_stride"),
    (dict(cap=-1), -1, b"capacity"),
    (dict(W=33000), -1, b"image"),
    (dict(H=0), -1, b"image"),
    (dict(n=-2), -1, b"n_gaussians"),
    (dict(n=1 << 31), -1, b"n_gaussians"),
    (dict(ws=0), -2, b"workspace is NULL"),
    (dict(ws=WS + 64), -2, b"256-byte aligned"),
    (dict(bws=0), -2, b"backward workspace is NULL"),
    (dict(bws=BWS + 16), -2, b"backward workspace must be 256-byte aligned"),
    (dict(bws_bytes=100 * 33 * 4 - 1), -2, b"backward workspace has"),
])
def test_backward_refusals(lib, kw, code, msg):
    assert _bwd(lib, **kw) == code
    assert msg in lib.vp_last_error()


def test_backward_workspace_bytes(lib):
    up = lambda v: -(-v // 256) * 256  # noqa: E731
    assert lib.vp_splat_backward_workspace_bytes(1000, 13) == up(1000 * 14 * 4)
    assert lib.vp_splat_backward_workspace_bytes(2_700_000, 64) == up(2_700_000 * 65 * 4)
    assert lib.vp_splat_backward_workspace_bytes(0, 1) == 256
    for cap, D in ((-1, 8), (1 << 31, 8), (100, 0), (100, 65)):
        assert lib.vp_splat_backward_workspace_bytes(cap, D) == 0


def test_symbols_in_exports_and_header():
    import voxproj_host
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "voxproj.h")).read()
    for name in ("vp_splat_backward_workspace_bytes", "vp_splat_rasterize_backward"):
        assert name in voxproj_host.EXPORTS and f" {name}(" in hdr
    assert voxproj_host.VP_ABI_VERSION == 4


def test_python_refusals_before_device_work():
    import torch
    import splat_autograd
    import voxproj_host
    m, q, s, o, f = torch.zeros(4, 3), torch.zeros(4, 4), torch.zeros(4, 3), torch.zeros(4), torch.zeros(4, 8)
    vm, K = np.eye(4), K_(10, 16, 16)
    with pytest.raises(ValueError, match="CUDA tensor"):
        splat_autograd.splat_features(m, q, s, o, f.requires_grad_(), vm, K, 16, 16)
    for name, t in (("means", m), ("quats", q), ("scales", s)):
        g = dict(means=m, quats=q, scales=s)
        g[name] = t.clone().requires_grad_()
        with pytest.raises(ValueError, match="geometry gradients are not implemented"):
            splat_autograd.splat_features(g["means"], g["quats"], g["scales"], o, f, vm, K, 16, 16)
    with pytest.raises(ValueError, match="float32"):
        splat_autograd.splat_features(m, q, s, o, f.double(), vm, K, 16, 16)
    with pytest.raises(ValueError, match="CUDA tensor"):
        voxproj_host.splat_rasterize_backward(f, 4, 16, 16, 10, voxproj_host.SplatWorkspace())
