"""splat_autograd.splat_photometric on the GPU: the rasterizer, the photometric loss, its gradient image and the rasterizer's
backward as one differentiable call, on a synthetic_gaussians scene of 400 Gaussians at 96 x 64 with three colour channels.

The kernels themselves are held to float64 in test_gpu_photo_loss.py (the loss) and test_gpu_splat_backward*.py (the
backward); here the chain is checked bit for bit against its pieces: it adds no arithmetic, so there is no tolerance.  Every
test here fails on a tree without splat_photometric."""
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

import splat_autograd  # noqa: E402
import synthetic_gaussians as sg  # noqa: E402
import voxproj_host  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
W, H, N = 96, 64, 400
GEO = ("means", "quats", "scales", "opacities", "colors")
LAMBDA = 0.2
_SCENE = {}


def setup():
    if not _SCENE:
        g = sg.make_gaussians(N, seed=5, scale_median=0.15)
        w2c, K = sg.make_views(6, g["room"], W, seed=5)
        rng = np.random.default_rng(5)
        s = dict(means=g["means"], quats=g["quats"], scales=g["scales"], opacities=g["opacities"],
                 colors=rng.uniform(0, 1, (N, 3)).astype(np.float32))
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        target = np.stack([0.5 + 0.4 * np.sin(0.1 * xx + c) * np.cos(0.13 * yy) for c in range(3)]).astype(np.float32)
        _SCENE.update(s=s, vm=w2c[2], K=K, target=torch.from_numpy(target).to(DEV))
    return _SCENE


def tensors(sc, grads):
    return {k: torch.from_numpy(sc["s"][k]).to(DEV).requires_grad_(k in grads) for k in GEO}


@pytest.mark.parametrize("grads", [GEO, ("colors",), ("colors", "opacities"), ("means",), ("scales", "quats")],
                         ids=lambda g: "+".join(g))
def test_stats_and_gradients_equal_the_pieces(grads, monkeypatch):
    sc = setup()
    calls = []
    for name in ("splat_rasterize_backward", "splat_rasterize_backward_geometry"):
        real = getattr(voxproj_host, name)
        monkeypatch.setattr(voxproj_host, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    t = tensors(sc, grads)
    loss, stats = splat_autograd.splat_photometric(*(t[k] for k in GEO), sc["vm"], sc["K"], W, H, sc["target"],
                                                   lambda_dssim=LAMBDA, check=False)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.requires_grad
    assert stats.dtype == torch.float64 and tuple(stats.shape) == (3,) and not stats.requires_grad
    (3.0 * loss).backward()
    geometry = any(k in grads for k in ("means", "quats", "scales"))
    assert calls == ["splat_rasterize_backward_geometry" if geometry else "splat_rasterize_backward"], calls
    # the pieces: the image splat_features renders, photo_loss on it, the gradient image into splat_gaussians' backward
    d = {k: v.detach() for k, v in t.items()}
    r = voxproj_host.splat_features(d["means"], d["quats"], d["scales"], d["opacities"], d["colors"], sc["vm"], sc["K"], W, H,
                                    want_logits=True, want_alpha=False, want_confidence=False, check=False)
    assert float(r.logits.abs().max()) > 0.1, "the view is empty"
    stats2, _, lws = voxproj_host.photo_loss(r.logits, sc["target"])
    assert torch.equal(stats, stats2)
    n = 3 * W * H
    want_loss = ((1.0 - LAMBDA) * stats2[0] / n + LAMBDA * (1.0 - stats2[2] / n)).float()
    assert float(loss.detach()) == float(want_loss)
    G = voxproj_host.photo_loss_gradient(r.logits, sc["target"], lws, lambda_dssim=LAMBDA,
                                         grad_loss=torch.full((1,), 3.0, device=DEV))
    t2 = tensors(sc, grads)
    logits, _, _, _ = splat_autograd.splat_gaussians(*(t2[k] for k in GEO), sc["vm"], sc["K"], W, H, check=False)
    assert torch.equal(logits.detach(), r.logits)
    logits.backward(G)
    for k in GEO:
        if k in grads:
            assert t[k].grad is not None and torch.isfinite(t[k].grad).all() and float(t[k].grad.abs().max()) > 0, k
            assert torch.equal(t[k].grad, t2[k].grad), f"{k}: the chain's gradient is not its pieces'"
        else:
            assert t[k].grad is None, f"{k} was not asked for"


def test_loss_falls_when_the_colours_are_trained():
    sc = setup()
    t = tensors(sc, ("colors",))
    opt = torch.optim.Adam([t["colors"]], lr=0.05)
    first = last = None
    for _ in range(15):
        opt.zero_grad(set_to_none=True)
        loss, _ = splat_autograd.splat_photometric(*(t[k] for k in GEO), sc["vm"], sc["K"], W, H, sc["target"], check=False)
        loss.backward()
        opt.step()
        last = float(loss.detach())
        first = last if first is None else first
    assert last < first, (first, last)


def test_arguments_are_checked():
    sc = setup()
    t = tensors(sc, ())
    with pytest.raises(ValueError):
        splat_autograd.splat_photometric(*(t[k] for k in GEO), sc["vm"], sc["K"], W, H, sc["target"], lambda_dssim=1.5)
    with pytest.raises(ValueError):
        splat_autograd.splat_photometric(*(t[k] for k in GEO), sc["vm"], sc["K"], W, H, sc["target"][:, :10])
    with pytest.raises(ValueError):
        splat_autograd.splat_photometric(*(t[k] for k in GEO), sc["vm"], sc["K"], W, H, sc["target"].clone().requires_grad_(True))
