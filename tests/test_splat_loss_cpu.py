"""The float64 statement of the fused splatting cross-entropy (tests/splat_loss_reference.py) checked on the CPU: its value
against torch's F.cross_entropy on splat64's logits, its analytic gradients against central finite differences of its own
loss (test_splat_grad_cpu.py's method), and the header's declarations."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import splat_loss_reference as lref  # noqa: E402
import splat_reference as ref  # noqa: E402
from test_gpu_splat import camera, scene  # noqa: E402


def maps(D, W, H, seed, weights=True):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, D, (H, W)).astype(np.int32)
    t[rng.uniform(size=(H, W)) < 0.15] = -1
    t[rng.uniform(size=(H, W)) < 0.05] = D + 3
    t[0, 0] = 255
    w = rng.uniform(0.1, 2.0, (H, W)).astype(np.float32) if weights else None
    if weights:
        w[rng.uniform(size=(H, W)) < 0.05] = 0.0
    return t, w


@pytest.mark.parametrize("D", [1, 3, 13])
@pytest.mark.parametrize("weights", [False, True])
def test_value_equals_torch_cross_entropy(D, weights):
    W, H = 29, 23
    s = scene(150, D, D + 1)
    vm, K = camera(W, H)
    t, w = maps(D, W, H, D, weights)
    o64 = ref.splat64(s["means"], s["quats"], s["scales"], s["opacities"], s["features"], vm, K, W, H)
    r = lref.loss64(s["means"], s["quats"], s["scales"], s["opacities"], s["features"], vm, K, W, H, t, w, grads=False)
    assert np.abs(r["logits"] - o64["logits"]).max() <= 1e-11 * max(1.0, np.abs(o64["logits"]).max())
    u = lref.upstream64(o64["logits"], t, w, "mean")
    tt = torch.from_numpy(np.where((t >= 0) & (t < D), t, -100).astype(np.int64)).reshape(-1)
    ce = torch.nn.functional.cross_entropy(torch.from_numpy(o64["logits"]).reshape(D, -1).T, tt, reduction="none",
                                           ignore_index=-100).numpy().reshape(H, W)
    ww = np.ones((H, W)) if w is None else w.astype(np.float64)
    ww = np.where((t >= 0) & (t < D), ww, 0.0)
    assert u["valid"].sum() > 0.5 * W * H and (~u["valid"]).sum() > 20
    assert np.abs(u["pixel_loss"] - ww * ce).max() <= 1e-12
    assert abs(u["stats"][0] - (ww * ce).sum()) <= 1e-10 and abs(u["stats"][1] - ww.sum()) <= 1e-10
    assert abs(u["loss"] - (ww * ce).sum() / ww.sum()) <= 1e-12
    assert abs(lref.upstream64(o64["logits"], t, w, "sum")["loss"] - (ww * ce).sum()) <= 1e-10
    # a pixel nothing reaches: l = log D
    empty = (o64["visits"] == 0) & u["valid"]
    if empty.any():
        assert np.abs(u["l"][empty] - np.log(D)).max() <= 1e-12


def test_all_ignored_is_zero():
    W, H, D = 17, 11, 4
    s = scene(60, D, 2)
    vm, K = camera(W, H)
    t = np.full((H, W), -1, np.int32)
    for red in ("mean", "sum"):
        r = lref.loss64(s["means"], s["quats"], s["scales"], s["opacities"], s["features"], vm, K, W, H, t, None, red)
        assert r["loss"] == 0.0 and (r["stats"] == 0).all() and (r["G"] == 0).all()
        assert all((r[k] == 0).all() for k in ("grad_f", "grad_o", "grad_means", "grad_quats", "grad_scales"))


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_analytic_gradients_match_finite_differences(reduction):
    W, H, D = 21, 17, 4
    s = {k: v.astype(np.float64) for k, v in scene(40, D, 9, scale=0.12).items()}
    vm, K = camera(W, H)
    t, w = maps(D, W, H, 5)
    args = lambda q: (q["means"], q["quats"], q["scales"], q["opacities"], q["features"], vm, K, W, H, t, w, reduction)  # noqa: E731
    r = lref.loss64(*args(s), grad_loss=1.7, round_records=False)
    # pixels where a threshold decision could flip within the step are taken out of the loss on both sides
    t = np.where(r["fragile"], -1, t).astype(np.int32)
    r = lref.loss64(*args(s), grad_loss=1.7, round_records=False)
    f = lambda q: 1.7 * lref.loss64(*args(q), round_records=False, grads=False)["loss"]  # noqa: E731
    rng = np.random.default_rng(0)
    checked = 0
    for name, key, h, picks in (("features", "grad_f", 1e-5, 12), ("opacities", "grad_o", 1e-6, 10),
                                ("means", "grad_means", 1e-6, 6), ("scales", "grad_scales", 1e-6, 6)):
        g = r[key]
        nz = np.argwhere(g != 0)
        assert len(nz) >= picks, name
        for idx in nz[rng.choice(len(nz), picks, replace=False)]:
            idx = tuple(idx)
            hi, lo = {k: v.copy() for k, v in s.items()}, {k: v.copy() for k, v in s.items()}
            hi[name][idx] += h
            lo[name][idx] -= h
            fd = (f(hi) - f(lo)) / (2 * h)
            assert abs(fd - g[idx]) <= 1e-5 * max(abs(g[idx]), abs(fd)) + 1e-8, (name, idx, fd, g[idx])
            checked += 1
    assert checked == 34


def test_bounds_are_small_and_positive():
    D = 13
    C = np.random.default_rng(1).normal(size=(D, 5, 7))
    t = np.zeros((5, 7), np.int32)
    u = lref.upstream64(C, t)
    u["logits"] = C
    b = lref.pixel_loss_bound(u, 1e-4)
    assert (b > 2e-4).all() and (b < 2.1e-4).all()
    assert np.allclose(lref.loss_grad_bound(np.ones(3), [u["G"]], 1e-4), 1e-4 + 2e-4 + 1e-6 * np.abs(u["G"]).max())


def test_header_declares_the_loss_symbols():
    text = open(os.path.join(ROOT, "include", "voxproj.h")).read()
    for sym in ("vp_splat_loss_workspace_bytes", "vp_splat_rasterize_loss", "vp_splat_loss_backward"):
        assert re.search(r"\b(size_t|int)\s+" + sym + r"\s*\(", text), sym
    assert "VP_LOSS_SUM" in text and "VP_LOSS_MEAN" in text
    assert re.search(r"#define\s+VP_ABI_VERSION\s+4\b", text)
    import voxproj_host
    for sym in ("vp_splat_loss_workspace_bytes", "vp_splat_rasterize_loss", "vp_splat_loss_backward"):
        assert sym in voxproj_host.EXPORTS
