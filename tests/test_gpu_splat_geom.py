"""The geometry backward (vp_splat_rasterize_backward_geometry, voxproj_host.splat_rasterize_backward_geometry,
splat_autograd.splat_gaussians) on the GPU against the float64 reference of tests/splat_geom_reference.py.

Bounds, per entry:
  grad_screen [N,5]   |err| <= 1e-4 M + 1e-6 max|G| (splat_grad_reference.grad_bound, the criterion of the existing backward
                      for this very sweep), M the same sums with every product replaced by its absolute value.
  grad_means / grad_quats / grad_scales
                      derived, not chosen: the chain is float64 on the device, so the error is the screen sums' error carried
                      through the chain's Jacobian plus one fp32 rounding of the result,
                      |err| <= sum_k |d s_k / d theta| bound(s_k) + 2^-23 |grad64|  (splat_geom_reference.theta_bound).
  grad_features / grad_opacities
                      bit-identical to vp_splat_rasterize_backward's, which test_gpu_splat_grad.py holds to its bound.
Pixels the forward's oracle marks fragile get zero upstream gradient.  Every case asserts a minimum number of nonzero
reference entries and prints its worst err / bound (profiles/r10_splat_geometry_accuracy.txt keeps one run's figures).
"""
import itertools
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

import splat_geom_reference as geo  # noqa: E402
import splat_grad_reference as gref  # noqa: E402
import voxproj_host  # noqa: E402
from test_gpu_splat import camera, scene  # noqa: E402
from test_gpu_splat_grad import tens, upstream  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
OUTS = ("means", "quats", "scales", "features", "opacities", "screen")
ALL = {f"want_{k}": True for k in OUTS}


def forward(s, vm, K, W, H, ws=None):
    t = tens(s)
    ws = ws if ws is not None else voxproj_host.SplatWorkspace()
    r = voxproj_host.splat_features(t["means"], t["quats"], t["scales"], t["opacities"], t["features"], vm, K, W, H,
                                    want_logits=True, want_alpha=True, workspace=ws, check=False)
    return t, ws, r


def run_geometry(s, vm, K, W, H, G, Ga, capacity=None, status=None, bws=None, **want):
    t, ws, r = forward(s, vm, K, W, H)
    gt = torch.from_numpy(G).to(DEV) if G is not None else None
    gat = torch.from_numpy(Ga).to(DEV) if Ga is not None else None
    g = voxproj_host.splat_rasterize_backward_geometry(t["means"], t["quats"], t["scales"], t["features"], vm, K, W, H,
                                                       r.n_isect if capacity is None else capacity, ws, gt, gat, status=status,
                                                       bwd_workspace=bws, **(want or ALL))
    old = voxproj_host.splat_rasterize_backward(t["features"], len(s["means"]), W, H, r.n_isect, ws, gt, gat)
    torch.cuda.synchronize()
    return g, old


def compare(name, s, vm, K, W, H, G, Ga, g, old, min_nonzero=1):
    r = geo.splat_geom64(s["means"], s["quats"], s["scales"], s["opacities"], s["features"], vm, K, W, H, G=G, G_alpha=Ga)
    assert torch.equal(g["features"], old[0]) and torch.equal(g["opacities"], old[1]), "not the existing backward's bits"
    bs = gref.grad_bound(r["M_screen"], [G, Ga])
    es = np.abs(g["screen"].cpu().numpy().astype(np.float64) - r["grad_screen"])
    theta64 = np.concatenate([r["grad_means"], r["grad_quats"], r["grad_scales"]], 1)
    theta = torch.cat([g["means"], g["quats"], g["scales"]], 1).cpu().numpy().astype(np.float64)
    bt = geo.theta_bound(r["jac"], bs, theta64)
    et = np.abs(theta - theta64)
    nz_s, nz_t = int((r["grad_screen"] != 0).sum()), int((theta64 != 0).sum())
    ratio = lambda e, b: float((e / np.maximum(b, 1e-300)).max()) if e.size else 0.0  # noqa: E731
    print(f"geom-accuracy {name}: screen err/bound {ratio(es, bs):.4f} means {ratio(et[:, :3], bt[:, :3]):.4f} "
          f"quats {ratio(et[:, 3:7], bt[:, 3:7]):.4f} scales {ratio(et[:, 7:], bt[:, 7:]):.4f} "
          f"nonzero {nz_s} + {nz_t}", flush=True)
    assert nz_s >= min_nonzero and nz_t >= min_nonzero, f"only {nz_s} + {nz_t} nonzero reference entries"
    assert (es <= bs).all(), f"grad_screen error {es.max():.3e} over its bound at {np.unravel_index((es - bs).argmax(), es.shape)}"
    assert (et <= bt).all(), f"geometry error {et.max():.3e} over its bound at {np.unravel_index((et - bt).argmax(), et.shape)}"
    zero = r["added"] == 0
    for k in OUTS:
        assert (g[k][torch.from_numpy(zero).to(DEV)] == 0).all(), f"grad_{k}: a Gaussian no pixel added has a nonzero row"
    return r


@pytest.mark.parametrize("mode", ["logits", "alpha", "both"])
@pytest.mark.parametrize("D", [1, 3, 8, 9, 13, 16, 17, 32, 33, 64])
def test_random_scenes(D, mode):
    W, H = 61, 47
    s = scene(400, D, D)
    vm, K = camera(W, H)
    G, Ga = upstream(s, vm, K, W, H, mode, D)
    g, old = run_geometry(s, vm, K, W, H, G, Ga)
    compare(f"random D={D} {mode}", s, vm, K, W, H, G, Ga, g, old, min_nonzero=200)


@pytest.mark.parametrize("size", [(37, 23), (1, 1)])
def test_odd_sizes(size):
    W, H = size
    s = scene(300, 5, 3, spread=0.3 if W == 1 else 1.2, scale=0.4 if W == 1 else 0.05)
    vm, K = camera(W, H)
    G, Ga = upstream(s, vm, K, W, H, "both", 3)
    g, old = run_geometry(s, vm, K, W, H, G, Ga)
    compare(f"odd {W}x{H}", s, vm, K, W, H, G, Ga, g, old, min_nonzero=10)


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
    g, old = run_geometry(s, vm, K, W, H, G, Ga)
    r = compare("deep tile", s, vm, K, W, H, G, Ga, g, old, min_nonzero=2000)
    assert r["visits"].max() > 2 * 256


def test_saturating_stack_and_clamp():
    # 40 opaque Gaussians stacked on the axis: pixels stop after a few; the ones behind every stop get rows of exactly 0.
    # The front ones have o = 1: their raw alpha passes the 0.999 clamp near the centre (q = 0 there)
    W, H = 40, 30
    n = 40
    rng = np.random.default_rng(4)
    s = dict(means=np.stack([rng.uniform(-0.05, 0.05, n), rng.uniform(-0.05, 0.05, n), np.linspace(2.0, 4.0, n)], 1).astype(np.float32),
             quats=np.tile(np.float32([[1, 0, 0, 0]]), (n, 1)), scales=np.full((n, 3), 3.0, np.float32),
             opacities=np.where(np.arange(n) < 3, 1.0, 0.95).astype(np.float32), features=rng.normal(size=(n, 8)).astype(np.float32))
    vm, K = np.eye(4, dtype=np.float32), np.array([[20, 0, 20], [0, 20, 15], [0, 0, 1]], np.float32)
    G, Ga = upstream(s, vm, K, W, H, "both", 4)
    # the scratch starts as NaN: the zero partials written after every pixel of a tile has stopped are checked
    bws = voxproj_host.SplatWorkspace()
    bws.ensure(voxproj_host.lib().vp_splat_geometry_backward_workspace_bytes(4096, 8), DEV)
    bws.buf.fill_(255)
    g, old = run_geometry(s, vm, K, W, H, G, Ga, bws=bws)
    r = compare("saturating stack", s, vm, K, W, H, G, Ga, g, old, min_nonzero=10)
    assert (r["added"] == 0).sum() >= 10


def test_clamped_jacobian_branch():
    # wide Gaussians whose centres project beyond the Jacobian's clamp (p_x / z or p_y / z past the image by more than 15 %)
    # and still reach into the image, among ordinary ones
    W, H = 61, 47
    s = scene(300, 6, 9)
    rng = np.random.default_rng(9)
    n = 60
    z = rng.uniform(1.5, 3.0, n)
    side = rng.integers(0, 4, n)
    u = np.where(side < 2, rng.uniform(0.75, 0.85, n) * np.where(side == 0, 1, -1), rng.uniform(-0.4, 0.4, n))
    v = np.where(side >= 2, rng.uniform(0.62, 0.72, n) * np.where(side == 2, 1, -1), rng.uniform(-0.3, 0.3, n))
    vm, K = np.eye(4, dtype=np.float32), camera(W, H)[1]
    s["means"][:n] = np.stack([u * z, v * z, z], 1)
    s["scales"][:n] = rng.uniform(0.25, 0.5, (n, 3))
    s["opacities"][:n] = rng.uniform(0.5, 0.9, n)
    G, Ga = upstream(s, vm, K, W, H, "both", 9)
    g, old = run_geometry(s, vm, K, W, H, G, Ga)
    r = compare("clamped Jacobian", s, vm, K, W, H, G, Ga, g, old, min_nonzero=200)
    hit = r["clamped"] & (r["added"] > 0)
    assert hit.sum() >= 20, f"only {hit.sum()} Gaussians on the clamped branch were added by a pixel"
    assert (np.abs(r["grad_means"][hit]).max(1) > 0).sum() >= 20


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
    g, old = run_geometry(s, vm, K, W, H, G, Ga)
    compare("culled", s, vm, K, W, H, G, Ga, g, old, min_nonzero=200)
    for i in (3, 10, 20, 30, 40, 50):
        assert all((g[k][i] == 0).all() for k in OUTS)
    empty = dict(means=np.zeros((0, 3), np.float32), quats=np.zeros((0, 4), np.float32), scales=np.zeros((0, 3), np.float32),
                 opacities=np.zeros(0, np.float32), features=np.zeros((0, 6), np.float32))
    culled = dict(scene(200, 6, 2), means=np.tile(np.float32([[0, 0, -2.0]]), (200, 1)))
    for e in (empty, culled):
        G, Ga = np.ones((6, H, W), np.float32), np.ones((H, W), np.float32)
        g, _ = run_geometry(e, vm, K, W, H, G, Ga)
        assert g["means"].shape == (len(e["means"]), 3) and all((g[k] == 0).all() for k in OUTS)


def test_bit_identical_runs_and_every_subset_of_outputs():
    W, H = 90, 70
    s = scene(2000, 13, 6, scale=0.04)
    vm, K = camera(W, H)
    G, Ga = upstream(s, vm, K, W, H, "both", 6)
    a, old = run_geometry(s, vm, K, W, H, G, Ga)
    b, _ = run_geometry(s, vm, K, W, H, G, Ga)
    assert torch.equal(a["features"], old[0]) and torch.equal(a["opacities"], old[1])
    assert all(torch.equal(a[k], b[k]) for k in OUTS) and all((a[k] != 0).any() for k in OUTS)
    t, ws, r = forward(s, vm, K, W, H)
    gt, gat = torch.from_numpy(G).to(DEV), torch.from_numpy(Ga).to(DEV)
    bws = voxproj_host.SplatWorkspace()
    for mask in itertools.product((False, True), repeat=len(OUTS)):
        g = voxproj_host.splat_rasterize_backward_geometry(t["means"], t["quats"], t["scales"], t["features"], vm, K, W, H,
                                                           r.n_isect, ws, gt, gat, bwd_workspace=bws,
                                                           **{f"want_{k}": w for k, w in zip(OUTS, mask)})
        for k, w in zip(OUTS, mask):
            assert (g[k] is not None) == w and (not w or torch.equal(g[k], a[k])), (mask, k)


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
    bptr = bw.ensure(L.vp_splat_geometry_backward_workspace_bytes(total - 1, 8), DEV)
    outs = [torch.full((400, n), -7.0, device=DEV) for n in (3, 4, 3, 8, 1, 5)]
    vmc, (fx, fy, cx, cy) = voxproj_host._splat_camera(vm, K, W, H)
    status.zero_()

    def call(bwd_bytes, st):
        return L.vp_splat_rasterize_backward_geometry(
            t["means"].data_ptr(), t["quats"].data_ptr(), t["scales"].data_ptr(), t["features"].data_ptr(), 8, 8, 400, vmc, fx,
            fy, cx, cy, W, H, 0.3, total - 1, G.data_ptr(), None, *(o.data_ptr() for o in outs), st, ws.ptr(), ws.capacity(),
            bptr, bwd_bytes, torch.cuda.current_stream().cuda_stream)
    voxproj_host.check(call(bw.capacity(), status.data_ptr()))
    torch.cuda.synchronize()
    assert int(status.item()) == 1
    assert all((o == -7).all() for o in outs), "a too-small capacity must not write gradients"
    with pytest.raises(voxproj_host.VoxprojError, match="backward workspace"):
        voxproj_host.check(call(256, None))


# ------------------------------------------------------------------------------------------------ autograd
def leaves(t, names):
    return {k: (t[k].clone().requires_grad_() if k in names else t[k]) for k in ("means", "quats", "scales", "opacities", "features")}


def test_autograd_forward_and_all_five_gradients():
    import splat_autograd
    W, H, D = 61, 47, 13
    s = scene(500, D, 2)
    vm, K = camera(W, H)
    t = tens(s)
    p = leaves(t, ("means", "quats", "scales", "opacities", "features"))
    out = splat_autograd.splat_gaussians(p["means"], p["quats"], p["scales"], p["opacities"], p["features"], vm, K, W, H)
    plain = splat_autograd.splat_features(t["means"], t["quats"], t["scales"], t["opacities"], t["features"], vm, K, W, H)
    assert all(torch.equal(x.detach(), y) for x, y in zip(out, plain))
    logits, alpha, labels, conf = out
    assert not labels.requires_grad and not conf.requires_grad
    target = torch.randint(0, D, (H * W,), device=DEV, generator=torch.Generator(DEV).manual_seed(0))
    lg = logits.detach().clone().requires_grad_()
    al = alpha.detach().clone().requires_grad_()
    loss = lambda l, a: torch.nn.functional.cross_entropy(l.reshape(D, -1).T, target) + a.mean()  # noqa: E731
    loss(lg, al).backward()
    loss(logits, alpha).backward()
    _, ws, r = forward(s, vm, K, W, H)
    g = voxproj_host.splat_rasterize_backward_geometry(t["means"], t["quats"], t["scales"], t["features"], vm, K, W, H,
                                                       r.n_isect, ws, lg.grad, al.grad)
    for k in ("means", "quats", "scales", "opacities", "features"):
        assert torch.equal(p[k].grad, g[k]) and (p[k].grad != 0).any(), k


@pytest.mark.parametrize("names", [("means",), ("scales", "features"), ("quats", "opacities"), ("features", "opacities"),
                                   ("opacities",)])
def test_autograd_needs_input_grad_subsets(names):
    import splat_autograd
    W, H = 61, 47
    s = scene(400, 8, 5)
    vm, K = camera(W, H)
    t = tens(s)
    full = leaves(t, ("means", "quats", "scales", "opacities", "features"))
    part = leaves(t, names)
    for p in (full, part):
        lg, al, _, _ = splat_autograd.splat_gaussians(p["means"], p["quats"], p["scales"], p["opacities"], p["features"], vm, K,
                                                      W, H)
        (lg.square().sum() + al.sum()).backward()
    for k in full:
        if k in names:
            assert torch.equal(part[k].grad, full[k].grad) and (part[k].grad != 0).any(), k
        else:
            assert part[k].grad is None, k


def test_autograd_two_calls_keep_separate_workspaces():
    import splat_autograd
    W, H = 61, 47
    s = scene(400, 8, 5)
    t = tens(s)
    cams = [camera(W, H), camera(W, H, yaw=-0.08, pitch=0.02, t=(-0.05, 0.02, 0.0))]
    single = []
    for vm, K in cams:
        p = leaves(t, ("means", "scales"))
        lg, al, _, _ = splat_autograd.splat_gaussians(p["means"], p["quats"], p["scales"], p["opacities"], p["features"], vm, K,
                                                      W, H)
        (lg.square().sum() + al.sum()).backward()
        single.append(p)
    p = leaves(t, ("means", "scales"))
    outs = [splat_autograd.splat_gaussians(p["means"], p["quats"], p["scales"], p["opacities"], p["features"], vm, K, W, H)
            for vm, K in cams]                            # both forwards before either backward
    sum(lg.square().sum() + al.sum() for lg, al, _, _ in outs).backward()
    for k in ("means", "scales"):
        a, b = single[0][k].grad, single[1][k].grad
        assert (a != 0).any() and (b != 0).any() and not torch.equal(a, b)
        assert torch.allclose(p[k].grad, a + b, rtol=1e-5, atol=1e-6 * float((a + b).abs().max()))


def test_geometry_refinement_lowers_the_loss():
    # render a target, displace the means and scales, then Adam on the geometry (and, in both loops, on the features and
    # opacities): the loss after the loop must be below the initial one; printed beside the same loop with the geometry frozen
    import splat_autograd
    W, H, D = 96, 64, 6
    s = scene(1500, D, 21, scale=0.06)
    t = tens(s)
    cams = [camera(W, H), camera(W, H, yaw=-0.1, pitch=0.04, t=(-0.08, 0.03, 0.05))]
    with torch.no_grad():
        targets = [splat_autograd.splat_gaussians(t["means"], t["quats"], t["scales"], t["opacities"], t["features"], vm, K, W,
                                                  H)[:2] for vm, K in cams]
    gen = torch.Generator(DEV).manual_seed(1)
    means0 = t["means"] + 0.02 * torch.randn(t["means"].shape, device=DEV, generator=gen)
    logs0 = t["scales"].log() + 0.2 * torch.randn(t["scales"].shape, device=DEV, generator=gen)

    def loop(train_geometry, steps=60):
        means, logs, quats = (torch.nn.Parameter(x.clone()) for x in (means0, logs0, t["quats"]))
        feats, opl = torch.nn.Parameter(t["features"].clone()), torch.nn.Parameter(torch.logit(t["opacities"].clamp(1e-4, 1 - 1e-4)))
        groups = [dict(params=[feats, opl], lr=1e-2)]
        if train_geometry:
            groups += [dict(params=[means], lr=1e-3), dict(params=[logs, quats], lr=1e-2)]
        opt = torch.optim.Adam(groups)

        def loss_of():
            total = 0.0
            for (vm, K), (tl, ta) in zip(cams, targets):
                lg, al, _, _ = splat_autograd.splat_gaussians(means, quats, logs.exp(), opl.sigmoid(), feats, vm, K, W, H)
                total = total + (lg - tl).square().mean() + (al - ta).square().mean()
            return total
        first = float(loss_of().detach())
        for _ in range(steps):
            opt.zero_grad()
            loss_of().backward()
            opt.step()
        return first, float(loss_of().detach())

    l0, l1 = loop(True)
    f0, f1 = loop(False)
    print(f"geom-refinement: initial {l0:.6f} final {l1:.6f} geometry frozen {f1:.6f}", flush=True)
    assert f0 == l0
    assert l1 < l0, (l0, l1)
