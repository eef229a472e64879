"""vp_densify_accumulate on the GPU: which Gaussians it touches (the projection's tile rule, from the float64 oracle), the
statistic against the twin's formula applied to the device's own grad_screen bit for bit, two views in a row, the screen
radius against the oracle's float64 covariance, canaries, and the same through splat_photometric(densify_stats=...).

Fails on a library without vp_densify_accumulate."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "3d-semantic-segmentation_amd")
for p in (HERE, ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import densify_reference as dr  # noqa: E402
import splat_reference as sr  # noqa: E402
import splat_scenes  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257, 1000)
IMAGES = ((40, 24), (96, 64))
D = 3
PAD = 16                                                          # canary elements on each side of every output
F32 = np.float32


def cameras(W, H):
    """Two views of the same cloud."""
    a = splat_scenes._cam(splat_scenes.euler(0.05, -0.03, 0.0), (0.02, -0.01, 0.1), 0.9 * W, 0.9 * W, 0.5 * W + 0.3, 0.5 * H - 0.2)
    b = splat_scenes._cam(splat_scenes.euler(-0.1, 0.06, 0.2), (-0.05, 0.03, 0.3), 1.1 * W, 0.8 * W, 0.45 * W, 0.55 * H)
    return a, b


def scene(n, W, H):
    """scene_for_camera's cloud (centres up to 20 % off the image, a fifth of the opacities around 1/255) plus, from 63
    Gaussians on, some behind the camera and some non-finite."""
    (vm, K), _ = cameras(W, H)
    s = splat_scenes.scene_for_camera(n, D, 7 * n + W, vm, K, W, H)
    if n == 1:
        s["opacities"][:] = 0.8
    if n >= 63:
        vm64 = np.asarray(vm, np.float64)
        for i in range(3, n, 17):                                 # behind the camera: mirror the camera-space point in z
            pc = vm64[:3, :3] @ s["means"][i].astype(np.float64) + vm64[:3, 3]
            pc[2] = -pc[2]
            s["means"][i] = ((pc - vm64[:3, 3]) @ vm64[:3, :3]).astype(F32)
        s["means"][5, 1] = np.nan
        s["scales"][11, 0] = np.inf
        s["opacities"][13] = np.nan
        s["opacities"][19] = 0.003                                # below 1/255
    return s


def visible_twin(s, vm, K, W, H):
    rec = sr.records(s["means"], s["quats"], s["scales"], s["opacities"], vm, K, W, H)
    count, close = sr.tile_counts(rec, s["opacities"])
    return count > 0, close, rec


def with_canaries(n, dtype, dev, fill):
    buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=dev)
    return buf, buf[PAD:PAD + n]


@pytest.fixture(scope="module")
def scenes():
    """Every (n, W, H): the cloud and, per view, the oracle's visible set; computed once and left unchanged."""
    out = {}
    for n in SIZES:
        for W, H in IMAGES:
            s = scene(n, W, H)
            views = []
            for vm, K in cameras(W, H):
                vis, close, rec = visible_twin(s, vm, K, W, H)
                assert close.sum() <= 0.01 * n, (n, W, H, int(close.sum()))
                views.append((vm, K, vis, close, rec))
            out[(n, W, H)] = (s, views)
    assert any(v[2].any() and not v[2].all() for _, vs in out.values() for v in vs)
    return out


@pytest.mark.parametrize("W,H", IMAGES)
@pytest.mark.parametrize("n", SIZES)
def test_accumulate_against_the_twin(scenes, n, W, H):
    import voxproj_host
    dev = torch.device("cuda:0")
    s, views = scenes[(n, W, H)]
    t = {k: torch.from_numpy(v).to(dev) for k, v in s.items()}
    stats = voxproj_host.DensifyStats(n, dev, want_radius=True)
    bufs = {}
    for name, dtype, fill in (("grad_accum", torch.float32, 0.0), ("denom", torch.int32, 0), ("max_radius", torch.float32, 0.0)):
        bufs[name], view = with_canaries(n, dtype, dev, 77)
        view.zero_()
        setattr(stats, name, view)
    ga, dn = np.zeros(n, F32), np.zeros(n, np.int32)
    rad = np.zeros(n, np.float64)
    rng = np.random.default_rng(n + W)
    for vi, (vm, K, vis, close, rec) in enumerate(views):
        ws = voxproj_host.SplatWorkspace()
        r = voxproj_host.splat_features(t["means"], t["quats"], t["scales"], t["opacities"], t["features"], vm, K, W, H,
                                        want_logits=True, workspace=ws, check=False)
        G = torch.from_numpy(rng.normal(size=(D, H, W)).astype(F32)).to(dev)
        g = voxproj_host.splat_rasterize_backward_geometry(t["means"], t["quats"], t["scales"], t["features"], vm, K, W, H,
                                                           r.n_isect, ws, G, None, want_screen=True)
        scale = (1.0, 3.0)[vi]
        before = stats.denom.cpu().numpy().copy()
        voxproj_host.densify_accumulate(stats, g["screen"], ws, W, H, scale=scale,
                                        geometry=(t["means"], t["quats"], t["scales"], vm, K))
        touched = stats.denom.cpu().numpy() != before
        sure = ~close
        assert np.array_equal(touched[sure], vis[sure]), (n, W, H, vi)
        # the formula on the device's own grad_screen and the device's own visible set, in order: bit for bit
        ga, dn = dr.accumulate(ga, dn, g["screen"].cpu().numpy(), touched, W, H, scale)
        assert stats.grad_accum.cpu().numpy().tobytes() == ga.tobytes(), (n, W, H, vi)
        assert stats.denom.cpu().numpy().tobytes() == dn.tobytes(), (n, W, H, vi)
        rad = np.where(touched, np.maximum(rad, dr.screen_radius(rec["cov2d"])), rad)
        got = stats.max_radius.cpu().numpy().astype(np.float64)
        assert (got[~touched & (dn == 0)] == 0).all()
        rel = np.abs(got - rad)[dn > 0] / rad[dn > 0] if (dn > 0).any() else np.zeros(1)
        print(f"n {n} {W}x{H} view {vi}: {int(touched.sum())} visible, {int(close.sum())} close, max radius error "
              f"{rel.max():.3e} (allowed {2.0 ** -22:.3e})", flush=True)
        assert (rel <= 2.0 ** -22).all()
    assert n < 63 or (dn.max() == 2 and (dn == 0).any())
    for name, buf in bufs.items():
        assert bool((buf[:PAD] == 77).all()) and bool((buf[PAD + n:] == 77).all()), name
    # without max_radius the geometry is not needed and the statistic is the same
    plain = voxproj_host.DensifyStats(n, dev)
    voxproj_host.densify_accumulate(plain, g["screen"], ws, W, H, scale=3.0)
    e_ga, e_dn = dr.accumulate(np.zeros(n, F32), np.zeros(n, np.int32), g["screen"].cpu().numpy(), touched, W, H, 3.0)
    assert plain.grad_accum.cpu().numpy().tobytes() == e_ga.tobytes() and plain.denom.cpu().numpy().tobytes() == e_dn.tobytes()
    assert plain.max_radius is None
    with pytest.raises(ValueError):
        voxproj_host.densify_accumulate(stats, g["screen"], ws, W, H)          # max_radius without the geometry


@pytest.mark.parametrize("train", ("all", "colors"))
def test_through_splat_photometric(scenes, train):
    import splat_autograd
    import voxproj_host
    dev = torch.device("cuda:0")
    n, W, H = 1000, 96, 64
    s, views = scenes[(n, W, H)]
    vm, K = views[0][:2]
    s = {k: v.copy() for k, v in s.items()}
    for k in ("means", "scales", "opacities"):                    # splat_photometric's check=False still wants finite input
        bad = ~np.isfinite(s[k]).reshape(n, -1).all(1)
        s[k][bad] = 0.5
    target = torch.from_numpy(np.random.default_rng(1).uniform(0, 1, (D, H, W)).astype(F32)).to(dev)
    names = ("means", "quats", "scales", "opacities", "features")

    def run(stats, scale):
        t = [torch.from_numpy(s[k]).to(dev).requires_grad_(train == "all" or k == "features") for k in names]
        loss, _ = splat_autograd.splat_photometric(*t, vm, K, W, H, target, check=False, densify_stats=stats, stats_scale=scale)
        loss.backward()
        return loss.detach().cpu().numpy().tobytes(), [None if v.grad is None else v.grad.cpu().numpy().tobytes() for v in t]

    stats = voxproj_host.DensifyStats(n, dev, want_radius=True)
    base = run(None, 1.0)
    with_stats = run(stats, 2.0)
    assert base == with_stats
    assert (train == "all") == all(g is not None for g in base[1]) and base[1][4] is not None
    # the direct call on the same view
    t = {k: torch.from_numpy(s[k]).to(dev) for k in names}
    ws = voxproj_host.SplatWorkspace()
    r = voxproj_host.splat_features(t["means"], t["quats"], t["scales"], t["opacities"], t["features"], vm, K, W, H,
                                    want_logits=True, want_confidence=False, workspace=ws, check=False)
    _, _, lws = voxproj_host.photo_loss(r.logits, target)
    G = voxproj_host.photo_loss_gradient(r.logits, target, lws, lambda_dssim=0.2, grad_loss=torch.ones(1, device=dev))
    g = voxproj_host.splat_rasterize_backward_geometry(t["means"], t["quats"], t["scales"], t["features"], vm, K, W, H,
                                                       r.n_isect, ws, G, None, want_screen=True)
    direct = voxproj_host.DensifyStats(n, dev, want_radius=True)
    voxproj_host.densify_accumulate(direct, g["screen"], ws, W, H, scale=2.0, geometry=(t["means"], t["quats"], t["scales"], vm, K))
    for name in ("grad_accum", "denom", "max_radius"):
        assert getattr(stats, name).cpu().numpy().tobytes() == getattr(direct, name).cpu().numpy().tobytes(), name
    assert int(stats.denom.sum()) > 100 and float(stats.grad_accum.max()) > 0
