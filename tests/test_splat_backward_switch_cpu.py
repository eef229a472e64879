"""Which backward entry splat_autograd calls for which ``requires_grad`` mask, without a GPU: voxproj_host is replaced by
a stub that records every call and hands back marked tensors, so the call tables below and the order of the returned
gradients are checked on CPU tensors.

The tables are read off the backward of each autograd function: a geometry gradient (means, quats or scales), or the
screen-space sums that ``densify_stats`` asks for, takes splat_rasterize_backward_geometry with exactly the asked want_*
flags; features and opacities alone take splat_rasterize_backward; the two losses call their gradient kernel first, and
splat_photometric adds the view to the statistics after the geometry backward, with the sums that call returned."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import splat_autograd  # noqa: E402

N, D, W, H, CAP = 6, 3, 5, 4, 17
NAMES = ("means", "quats", "scales", "opacities", "features")
SHAPES = dict(means=(N, 3), quats=(N, 4), scales=(N, 3), opacities=(N,), features=(N, D))
MARK = dict(means=1.0, quats=2.0, scales=3.0, opacities=4.0, features=5.0, screen=6.0)


class Stats:
    def __init__(self, n):
        self.n = n


class Host:
    """The part of voxproj_host the three functions touch.  ``calls``: (entry, what it was asked for)."""
    DensifyStats = Stats

    def __init__(self):
        self.calls = []
        self.workspaces = []

    def SplatWorkspace(self):
        self.workspaces.append(object())
        return self.workspaces[-1]

    def _require(self, cond, msg):
        if not cond:
            raise ValueError(msg)

    def _require_tensors(self, *specs):
        for t, name, dtypes in specs:
            assert isinstance(t, torch.Tensor) and t.dtype in dtypes, name

    def splat_features(self, m, q, s, o, f, viewmat, K, W_, H_, *, workspace, **kw):
        assert workspace is self.workspaces[-1] and not any(t.requires_grad for t in (m, q, s, o, f))
        self.calls.append(("splat_features", None))
        return types.SimpleNamespace(logits=torch.ones((D, H_, W_)), alpha=torch.ones((H_, W_)), n_isect=CAP,
                                     labels=torch.zeros((H_, W_), dtype=torch.int32), confidence=torch.zeros((H_, W_)))

    def proto_contrast(self, image, ids, count, **proto):
        self.calls.append(("proto_contrast", None))
        return torch.tensor([3.0, 2.0, 1.0, 9.0], dtype=torch.float64), None, None, "lws"

    def photo_loss(self, image, target):
        self.calls.append(("photo_loss", None))
        return torch.tensor([3.0, 2.0, 1.0], dtype=torch.float64), None, "lws"

    def _gradient_image(self, entry, lws, grad_loss):
        assert lws == "lws" and grad_loss.dtype == torch.float32 and tuple(grad_loss.shape) == (1,)
        self.calls.append((entry, None))
        self.G = torch.full((D, H, W), 0.5)
        return self.G

    def proto_contrast_gradient(self, image, ids, count, lws, *, weight_contrast, weight_norm, grad_loss):
        return self._gradient_image("proto_contrast_gradient", lws, grad_loss)

    def photo_loss_gradient(self, image, target, lws, *, lambda_dssim, grad_loss):
        return self._gradient_image("photo_loss_gradient", lws, grad_loss)

    def splat_rasterize_backward(self, f, n, W_, H_, cap, ws, grad_logits=None, grad_alpha=None, *, want_features=True,
                                 want_opacities=True):
        assert (n, W_, H_, cap) == (N, W, H, CAP) and ws is self.workspaces[-1] and tuple(f.shape) == (N, D)
        self.grads_in = (grad_logits, grad_alpha)
        self.calls.append(("splat_rasterize_backward", dict(features=want_features, opacities=want_opacities)))
        return (torch.full((N, D), MARK["features"]) if want_features else None,
                torch.full((N,), MARK["opacities"]) if want_opacities else None)

    def splat_rasterize_backward_geometry(self, m, q, s, f, viewmat, K, W_, H_, cap, ws, grad_logits=None, grad_alpha=None, *,
                                          eps2d=0.3, want_means=True, want_quats=True, want_scales=True, want_features=True,
                                          want_opacities=True, want_screen=False):
        assert (W_, H_, cap, eps2d) == (W, H, CAP, 0.25) and ws is self.workspaces[-1]
        assert [tuple(t.shape) for t in (m, q, s, f)] == [SHAPES[k] for k in ("means", "quats", "scales", "features")]
        assert viewmat is VIEWMAT and K is KMAT
        self.grads_in = (grad_logits, grad_alpha)
        want = dict(means=want_means, quats=want_quats, scales=want_scales, opacities=want_opacities, features=want_features,
                    screen=want_screen)
        self.calls.append(("splat_rasterize_backward_geometry", want))
        self.out = {k: torch.full(SHAPES.get(k, (N, 5)), MARK[k]) if on else None for k, on in want.items()}
        return self.out

    def densify_accumulate(self, stats, grad_screen, ws, W_, H_, scale=1.0, geometry=None):
        assert grad_screen is self.out["screen"] and ws is self.workspaces[-1] and (W_, H_) == (W, H)
        assert len(geometry) == 6 and geometry[3] is VIEWMAT and geometry[4] is KMAT and geometry[5] == 0.25
        self.calls.append(("densify_accumulate", dict(stats=stats, scale=scale)))


VIEWMAT, KMAT = np.eye(4), np.eye(3)


def tensors(mask):
    return [torch.zeros(SHAPES[k]).requires_grad_(k in mask) for k in NAMES]


def gaussians(t, **kw):
    logits, alpha, _, _ = splat_autograd.splat_gaussians(*t, VIEWMAT, KMAT, W, H, eps2d=0.25)
    return 2.0 * logits.sum() + 3.0 * alpha.sum()


def contrastive(t, **kw):
    ids = torch.zeros((H, W), dtype=torch.int32)
    return splat_autograd.splat_contrastive(*t, VIEWMAT, KMAT, W, H, ids, eps2d=0.25)[0]


def photometric(t, **kw):
    return splat_autograd.splat_photometric(*t, VIEWMAT, KMAT, W, H, torch.zeros((D, H, W)), eps2d=0.25, **kw)[0]


FORWARD = {gaussians: ["splat_features"], contrastive: ["splat_features", "proto_contrast"],
           photometric: ["splat_features", "photo_loss"]}
GRADIENT = {gaussians: [], contrastive: ["proto_contrast_gradient"], photometric: ["photo_loss_gradient"]}
OFF = dict(means=False, quats=False, scales=False, opacities=False, features=False, screen=False)
# requires_grad mask -> (backward entry, what it is asked for)
TABLE = [
    (("features",), "splat_rasterize_backward", dict(features=True, opacities=False)),
    (("means",), "splat_rasterize_backward_geometry", dict(OFF, means=True)),
    (NAMES, "splat_rasterize_backward_geometry", dict(OFF, means=True, quats=True, scales=True, opacities=True, features=True)),
]


@pytest.fixture
def host(monkeypatch):
    h = Host()
    monkeypatch.setattr(splat_autograd, "_host", h)
    return h


@pytest.mark.parametrize("mask, entry, want", TABLE, ids=["features", "means", "everything"])
@pytest.mark.parametrize("fn", [gaussians, contrastive, photometric], ids=lambda f: f.__name__)
def test_backward_entry_and_gradient_order(host, fn, mask, entry, want):
    t = tensors(mask)
    loss = fn(t)
    assert [c[0] for c in host.calls] == FORWARD[fn]
    loss.backward()
    assert host.calls[len(FORWARD[fn]):] == [(e, None) for e in GRADIENT[fn]] + [(entry, want)]
    # every tensor gets its own gradient, and only those that asked
    for name, x in zip(NAMES, t):
        if name in mask:
            assert tuple(x.grad.shape) == SHAPES[name] and bool((x.grad == MARK[name]).all()), name
        else:
            assert x.grad is None, name
    gl, ga = host.grads_in
    if fn is gaussians:                                        # the upstream images, in fp32
        assert gl.dtype == torch.float32 and bool((gl == 2.0).all()) and bool((ga == 3.0).all())
    else:                                                      # the loss's gradient image, and no alpha gradient
        assert gl is host.G and ga is None


@pytest.mark.parametrize("fn", [gaussians, contrastive, photometric], ids=lambda f: f.__name__)
def test_nothing_asked_for_launches_nothing(host, fn):
    t = tensors(())
    loss = fn(t)
    assert not loss.requires_grad and [c[0] for c in host.calls] == FORWARD[fn]


def test_statistics_take_the_geometry_backward_and_are_fed_after_it(host):
    stats = Stats(N)
    t = tensors(("features",))
    loss = photometric(t, densify_stats=stats, stats_scale=4.0)
    loss.backward()
    assert host.calls[2:] == [("photo_loss_gradient", None),
                              ("splat_rasterize_backward_geometry", dict(OFF, features=True, screen=True)),
                              ("densify_accumulate", dict(stats=stats, scale=4.0))]
    assert bool((t[4].grad == MARK["features"]).all()) and all(x.grad is None for x in t[:4])
    with pytest.raises(ValueError, match="densify_stats must be"):
        photometric(tensors(("features",)), densify_stats=Stats(N + 1))


def test_features_first_signature_maps_the_two_gradients(host):
    """splat_features: SplatFeatures.forward takes (features, opacities, geometry ...); each still gets its own gradient."""
    for mask, want in ((("features",), dict(features=True, opacities=False)), (("opacities",), dict(features=False, opacities=True)),
                       (("opacities", "features"), dict(features=True, opacities=True))):
        host.calls.clear()
        t = tensors(mask)
        logits, alpha, _, _ = splat_autograd.splat_features(*t, VIEWMAT, KMAT, W, H)
        (logits.sum() + alpha.sum()).backward()
        assert host.calls == [("splat_features", None), ("splat_rasterize_backward", want)]
        for name, x in zip(NAMES, t):
            assert (x.grad is None) if name not in mask else bool((x.grad == MARK[name]).all()), name
    with pytest.raises(ValueError, match="scales requires grad, but geometry gradients are not implemented"):
        splat_autograd.splat_features(*tensors(("scales",)), VIEWMAT, KMAT, W, H)
