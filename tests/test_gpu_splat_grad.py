"""The splatting backward (vp_splat_rasterize_backward, voxproj_host.splat_rasterize_backward, splat_autograd) on the GPU
against the float64 reference of tests/splat_grad_reference.py.

Bound: |grad - grad64| <= 1e-4 M + 1e-6 max|G| per entry, M the reference's magnitude scale (the same sums with every
product replaced by its absolute value).  Pixels the forward's oracle marks fragile get zero upstream gradient (G and
G_alpha), so a threshold decision that fp32 may take the other way cannot reach a gradient.  Every case asserts a minimum
number of nonzero reference entries, so it cannot pass vacuously.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import splat_grad_reference as gref  # noqa: E402
import splat_reference as ref  # noqa: E402
import voxproj_host  # noqa: E402
from test_gpu_splat import camera, scene  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def tens(s):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in s.items()}


def upstream(s, vm, K, W, H, mode, seed):
    """G [D,H,W] and G_alpha [H,W] (None when the mode leaves it out), zero on the oracle's fragile pixels."""
    D = s["features"].shape[1]
    o = ref.splat64(s["means"], s["quats"], s["scales"], s["opacities"], s["features"], vm, K, W, H)
    rng = np.random.default_rng(seed + 1000)
    G = rng.normal(size=(D, H, W)).astype(np.float32) if mode in ("logits", "both") else None
    Ga = rng.normal(size=(H, W)).astype(np.float32) if mode in ("alpha", "both") else None
    if G is not None:
        G[:, o["fragile"]] = 0.0
    if Ga is not None:
        Ga[o["fragile"]] = 0.0
    return G, Ga


def run_backward(s, vm, K, W, H, G, Ga, feats=None, capacity=None, status=None, ws=None, bws=None):
    t = tens(s)
    f = feats if feats is not None else t["features"]
    ws = ws if ws is not None else voxproj_host.SplatWorkspace()
    r = voxproj_host.splat_features(t["means"], t["quats"], t["scales"], t["opacities"], f, vm, K, W, H, want_logits=True,
                                    want_alpha=True, workspace=ws, check=False)
    cap = r.n_isect if capacity is None else capacity
    gt = torch.from_numpy(G).to(DEV) if G is not None else None
    gat = torch.from_numpy(Ga).to(DEV) if Ga is not None else None
    gf, go = voxproj_host.splat_rasterize_backward(f, f.shape[0], W, H, cap, ws, gt, gat, status=status, bwd_workspace=bws)
    torch.cuda.synchronize()
    return gf, go, r


def compare(s, vm, K, W, H, G, Ga, gf, go, min_nonzero=1):
    r = gref.splat_grad64(s["means"], s["quats"], s["scales"], s["opacities"], s["features"], vm, K, W, H, G=G, G_alpha=Ga)
    bf = gref.grad_bound(r["M_f"], [G, Ga])
    bo = gref.grad_bound(r["M_o"], [G, Ga])
    ef = np.abs(gf.cpu().numpy().astype(np.float64) - r["grad_f"])
    eo = np.abs(go.cpu().numpy().astype(np.float64) - r["grad_o"])
    nz = int((r["grad_f"] != 0).sum() + (r["grad_o"] != 0).sum())
    assert nz >= min_nonzero, f"only {nz} nonzero reference entries"
    assert (ef <= bf).all(), f"grad_f error {ef.max():.3e} over its bound at {np.unravel_index((ef - bf).argmax(), ef.shape)}"
    assert (eo <= bo).all(), f"grad_o error {eo.max():.3e} over its bound at {(eo - bo).argmax()}"
    return r


@pytest.mark.parametrize("mode", ["logits", "alpha", "both"])
@pytest.mark.parametrize("D", [1, 3, 8, 9, 13, 16, 17, 32, 33, 64])
def test_random_scenes(D, mode):
    W, H = 61, 47
    s = scene(400, D, D)
    vm, K = camera(W, H)
    G, Ga = upstream(s, vm, K, W, H, mode, D)
    gf, go, _ = run_backward(s, vm, K, W, H, G, Ga)
    r = compare(s, vm, K, W, H, G, Ga, gf, go, min_nonzero=200)
    if G is None:
        assert (gf == 0).all()


@pytest.mark.parametrize("size", [(37, 23), (1, 1)])
def test_odd_sizes(size):
    W, H = size
    s = scene(300, 5, 3, spread=0.3 if W == 1 else 1.2, scale=0.4 if W == 1 else 0.05)
    vm, K = camera(W, H)
    G, Ga = upstream(s, vm, K, W, H, "both", 3)
    gf, go, _ = run_backward(s, vm, K, W, H, G, Ga)
    compare(s, vm, K, W, H, G, Ga, gf, go, min_nonzero=10)


def test_tile_with_more_gaussians_than_one_batch():
    W, H = 32, 32
    rng = np.random.default_rng(11)
    n = 3000
    s = scene(n, 32, 11)
    s["means"] = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), rng.uniform(1.5, 3.0, n)], 1).astype(np.float32)
    s["scales"] = np.full((n, 3), 0.3, np.float32)
    s["opacities"] = rng.uniform(0.01, 0.03, n).astype(np.float32)
    vm, K = np.eye(4, dtype=np.float32), np.array([[30, 0, 16], [0, 30, 16], [0, 0, 1]], np.float32)
    G, Ga = upstream(s, vm, K, W, H, "both", 11)
    gf, go, _ = run_backward(s, vm, K, W, H, G, Ga)
    r = compare(s, vm, K, W, H, G, Ga, gf, go, min_nonzero=2000)
    assert r["visits"].max() > 2 * 256


def test_saturating_stack_and_clamp():
    # 40 opaque Gaussians stacked on the axis: pixels stop after a few; the ones behind every stop get rows of exactly 0.
    # The front ones have o = 1: their raw alpha passes the 0.999 clamp near the centre (da/do = 0 there)
    W, H = 40, 30
    n = 40
    rng = np.random.default_rng(4)
    s = dict(means=np.stack([rng.uniform(-0.05, 0.05, n), rng.uniform(-0.05, 0.05, n), np.linspace(2.0, 4.0, n)], 1).astype(np.float32),
             quats=np.tile(np.float32([[1, 0, 0, 0]]), (n, 1)), scales=np.full((n, 3), 3.0, np.float32),
             opacities=np.where(np.arange(n) < 3, 1.0, 0.95).astype(np.float32), features=rng.normal(size=(n, 8)).astype(np.float32))
    vm, K = np.eye(4, dtype=np.float32), np.array([[20, 0, 20], [0, 20, 15], [0, 0, 1]], np.float32)
    G, Ga = upstream(s, vm, K, W, H, "both", 4)
    # the backward scratch starts as NaN: the zero partials written after every pixel of a tile has stopped are checked
    bws = voxproj_host.SplatWorkspace()
    bws.ensure(voxproj_host.lib().vp_splat_backward_workspace_bytes(4096, 8), DEV)
    bws.buf.fill_(255)
    gf, go, _ = run_backward(s, vm, K, W, H, G, Ga, bws=bws)
    r = compare(s, vm, K, W, H, G, Ga, gf, go, min_nonzero=10)
    behind = r["added"] == 0
    assert behind.sum() >= 10
    assert (gf.cpu().numpy()[behind] == 0).all() and (go.cpu().numpy()[behind] == 0).all()


def test_culled_nan_and_empty_give_zero_rows():
    W, H = 61, 47
    s = scene(300, 6, 4)
    s["means"][3, 1] = np.nan
    s["scales"][10, 0] = np.inf
    s["opacities"][20] = np.nan
    s["means"][30] = (0, 0, -2.0)                       # behind the camera
    s["quats"][40] = 0.0
    s["opacities"][50] = 0.001
    vm, K = camera(W, H)
    G, Ga = upstream(s, vm, K, W, H, "both", 4)
    gf, go, _ = run_backward(s, vm, K, W, H, G, Ga)
    compare(s, vm, K, W, H, G, Ga, gf, go, min_nonzero=200)
    for i in (3, 10, 20, 30, 40, 50):
        assert (gf[i] == 0).all() and go[i] == 0
    empty = dict(means=np.zeros((0, 3), np.float32), quats=np.zeros((0, 4), np.float32), scales=np.zeros((0, 3), np.float32),
                 opacities=np.zeros(0, np.float32), features=np.zeros((0, 6), np.float32))
    culled = dict(scene(200, 6, 2), means=np.tile(np.float32([[0, 0, -2.0]]), (200, 1)))
    for e in (empty, culled):
        G, Ga = np.ones((6, H, W), np.float32), np.ones((H, W), np.float32)
        gf, go, _ = run_backward(e, vm, K, W, H, G, Ga)
        assert gf.shape == (len(e["means"]), 6) and (gf == 0).all() and (go == 0).all()


def test_row_stride_above_d():
    W, H = 61, 47
    s = scene(300, 13, 3)
    vm, K = camera(W, H)
    wide = torch.zeros((300, 20), device=DEV)
    wide[:, :13] = torch.from_numpy(s["features"]).to(DEV)
    wide[:, 13:] = float("nan")                      # never read
    G, Ga = upstream(s, vm, K, W, H, "both", 3)
    gf, go, _ = run_backward(s, vm, K, W, H, G, Ga, feats=wide[:, :13])
    compare(s, vm, K, W, H, G, Ga, gf, go, min_nonzero=200)


def test_too_small_capacity_writes_nothing():
    W, H = 61, 47
    s = scene(400, 8, 1)
    vm, K = camera(W, H)
    t = tens(s)
    ws = voxproj_host.SplatWorkspace()
    total = int(voxproj_host.splat_project(t["means"], t["quats"], t["scales"], t["opacities"], vm, K, W, H, workspace=ws).item())
    assert total > 10
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    voxproj_host.splat_rasterize(t["features"], 400, W, H, total - 1, ws, want_logits=True, want_alpha=True, status=status)
    G = torch.ones((8, H, W), device=DEV)
    L = voxproj_host.lib()
    bw = voxproj_host.SplatWorkspace()
    bptr = bw.ensure(L.vp_splat_backward_workspace_bytes(total - 1, 8), DEV)
    gf = torch.full((400, 8), -7.0, device=DEV)
    go = torch.full((400,), -7.0, device=DEV)
    status.zero_()
    voxproj_host.check(L.vp_splat_rasterize_backward(t["features"].data_ptr(), 8, 8, 400, W, H, total - 1, G.data_ptr(), None,
                                                     gf.data_ptr(), go.data_ptr(), status.data_ptr(), ws.ptr(), ws.capacity(),
                                                     bptr, bw.capacity(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert int(status.item()) == 1
    assert (gf == -7).all() and (go == -7).all(), "a too-small capacity must not write gradients"
    with pytest.raises(voxproj_host.VoxprojError, match="backward workspace"):
        voxproj_host.check(L.vp_splat_rasterize_backward(t["features"].data_ptr(), 8, 8, 400, W, H, total - 1, G.data_ptr(),
                                                         None, gf.data_ptr(), go.data_ptr(), None, ws.ptr(), ws.capacity(),
                                                         bptr, 256, torch.cuda.current_stream().cuda_stream))


def test_bit_identical_runs():
    W, H = 90, 70
    s = scene(4000, 32, 6, scale=0.04)
    vm, K = camera(W, H)
    G, Ga = upstream(s, vm, K, W, H, "both", 6)
    a = run_backward(s, vm, K, W, H, G, Ga)
    b = run_backward(s, vm, K, W, H, G, Ga)
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes()
    assert a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()


def test_linearity_identity_at_scale():
    # sum_{g,c} grad_f f = sum_p G . C (the logits are linear in f); bounded by the same sums of absolute values
    import synthetic_gaussians as sg
    W, H = 876, 584
    g = sg.make_gaussians(200_000, seed=0)
    f = torch.from_numpy(sg.make_logits(g["classes"], 13, seed=0)).to(DEV)
    t = {k: torch.from_numpy(g[k]).to(DEV) for k in ("means", "quats", "scales", "opacities")}
    w2c, K = sg.make_views(24, g["room"], W, seed=0)
    ws = voxproj_host.SplatWorkspace()
    r = voxproj_host.splat_features(t["means"], t["quats"], t["scales"], t["opacities"], f, w2c[12], K, W, H, want_logits=True,
                                    workspace=ws, check=False)
    G = torch.randn((13, H, W), device=DEV, generator=torch.Generator(DEV).manual_seed(0))
    gf, _ = voxproj_host.splat_rasterize_backward(f, f.shape[0], W, H, r.n_isect, ws, G, None, want_opacities=False)
    rabs = voxproj_host.splat_features(t["means"], t["quats"], t["scales"], t["opacities"], f.abs(), w2c[12], K, W, H,
                                       want_logits=True, check=False)
    lhs = (gf.double() * f.double()).sum().item()
    rhs = (G.double() * r.logits.double()).sum().item()
    scale = (G.double().abs() * rabs.logits.double()).sum().item()
    assert r.n_isect > 100_000 and scale > 0
    assert abs(lhs - rhs) <= 1e-4 * scale, (lhs, rhs, scale)


# ------------------------------------------------------------------------------------------------ autograd
def test_autograd_matches_abi_and_forward():
    import splat_autograd
    W, H = 61, 47
    s = scene(500, 13, 2)
    vm, K = camera(W, H)
    t = tens(s)
    f = t["features"].clone().requires_grad_()
    o = t["opacities"].clone().requires_grad_()
    logits, alpha, labels, conf = splat_autograd.splat_features(t["means"], t["quats"], t["scales"], o, f, vm, K, W, H)
    plain = voxproj_host.splat_features(t["means"], t["quats"], t["scales"], t["opacities"], t["features"], vm, K, W, H,
                                        want_logits=True, want_alpha=True)
    for x, y in ((logits, plain.logits), (alpha, plain.alpha), (labels, plain.labels), (conf, plain.confidence)):
        assert x.detach().cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert not labels.requires_grad and not conf.requires_grad
    G, Ga = upstream(s, vm, K, W, H, "both", 2)
    Gt, Gat = torch.from_numpy(G).to(DEV), torch.from_numpy(Ga).to(DEV)
    ((logits * Gt).sum() + (alpha * Gat).sum()).backward()
    gf, go, _ = run_backward(s, vm, K, W, H, G, Ga)
    assert f.grad.cpu().numpy().tobytes() == gf.cpu().numpy().tobytes()
    assert o.grad.cpu().numpy().tobytes() == go.cpu().numpy().tobytes()


def test_autograd_two_views_accumulate():
    import splat_autograd
    W, H = 61, 47
    s = scene(500, 8, 5)
    t = tens(s)
    cams = [camera(W, H), camera(W, H, yaw=-0.08, pitch=0.02, t=(-0.05, 0.02, 0.0))]
    f = t["features"].clone().requires_grad_()
    o = t["opacities"].clone().requires_grad_()
    single = []
    for vm, K in cams:
        ff = t["features"].clone().requires_grad_()
        oo = t["opacities"].clone().requires_grad_()
        lg, al, _, _ = splat_autograd.splat_features(t["means"], t["quats"], t["scales"], oo, ff, vm, K, W, H)
        (lg.square().sum() + al.sum()).backward()
        single.append((ff.grad, oo.grad))
    loss = 0
    for vm, K in cams:
        lg, al, _, _ = splat_autograd.splat_features(t["means"], t["quats"], t["scales"], o, f, vm, K, W, H)
        loss = loss + lg.square().sum() + al.sum()
    loss.backward()
    # autograd adds the two views' gradients in an order of its own: equal up to one rounding
    for got, a, b in ((f.grad, single[0][0], single[1][0]), (o.grad, single[0][1], single[1][1])):
        assert torch.allclose(got, a + b, rtol=1e-6, atol=1e-6)
        assert (a != 0).any() and (b != 0).any()


def test_autograd_geometry_requiring_grad_raises():
    import splat_autograd
    W, H = 16, 16
    t = tens(scene(20, 4, 0))
    vm, K = camera(W, H)
    for name in ("means", "quats", "scales"):
        g = {k: t[k] for k in ("means", "quats", "scales")}
        g[name] = g[name].clone().requires_grad_()
        with pytest.raises(ValueError, match="geometry gradients are not implemented"):
            splat_autograd.splat_features(g["means"], g["quats"], g["scales"], t["opacities"], t["features"], vm, K, W, H)


def test_refinement_loop_converges():
    # per-Gaussian logits as parameters, refined against labels rendered from the true logits over 4 views
    import splat_autograd
    import synthetic_gaussians as sg
    W, H, D = 96, 64, 13
    g = sg.make_gaussians(20000, n_classes=D, seed=3, scale_median=0.08)
    true = torch.from_numpy(sg.make_logits(g["classes"], D, seed=3)).to(DEV)
    t = {k: torch.from_numpy(g[k]).to(DEV) for k in ("means", "quats", "scales", "opacities")}
    w2c, K = sg.make_views(4 * 6, g["room"], W, seed=3)
    views = w2c[::6]
    targets = []
    for vm in views:
        r = voxproj_host.splat_features(t["means"], t["quats"], t["scales"], t["opacities"], true, vm, K, W, H,
                                        want_alpha=True, want_logits=True)
        srt = r.logits.sort(dim=0).values
        mask = (r.alpha > 0.5) & (srt[-1] - srt[-2] > 1e-3)        # covered pixels without a near tie
        targets.append((r.labels.long(), mask))
    assert all(int(m.sum()) > 0.1 * W * H for _, m in targets)
    gen = torch.Generator(DEV).manual_seed(0)
    param = torch.nn.Parameter(true + 2.5 * torch.randn(true.shape, device=DEV, generator=gen))
    opt = torch.optim.Adam([param], lr=0.1)

    def step(train):
        loss, agree, total = 0.0, 0, 0
        for vm, (lab, mask) in zip(views, targets):
            lg, _, labels, _ = splat_autograd.splat_features(t["means"], t["quats"], t["scales"], t["opacities"], param, vm, K,
                                                             W, H)
            ce = torch.nn.functional.cross_entropy(lg.reshape(D, -1).T[mask.reshape(-1)], lab.reshape(-1)[mask.reshape(-1)])
            loss = loss + ce / len(views)
            agree += int((labels.long() == lab)[mask].sum())
            total += int(mask.sum())
        if train:
            opt.zero_grad()
            loss.backward()
            opt.step()
        return float(loss.detach()), agree / total

    l0, a0 = step(False)
    for _ in range(50):
        step(True)
    l1, a1 = step(False)
    assert l1 <= 0.5 * l0, (l0, l1)
    assert a1 > a0, (a0, a1)
