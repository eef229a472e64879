"""The feature loss without a GPU: the library's three symbols and their host-side refusals, the Python wrappers' argument
checks, the float64 reference against finite differences and an independent analytic gradient, the exponent rule against
quantize_gradient_map, and the host side of distill_gaussian_features.py.  Everything that touches the library or the new
modules fails on a tree without vp_feature_loss."""
import ctypes
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

import feature_loss_reference as fref  # noqa: E402
import voxproj_host  # noqa: E402

SYMBOLS = ("vp_feature_loss_workspace_bytes", "vp_feature_loss", "vp_feature_loss_gradient")
EINVAL, EWORKSPACE = -1, -2                              # VP_EINVAL, VP_EWORKSPACE of include/voxproj.h


def test_library_exports_the_three_symbols():
    L = voxproj_host.lib()
    hdr = open(os.path.join(ROOT, "include", "voxproj.h")).read()
    for name in SYMBOLS:
        assert name in voxproj_host.EXPORTS and f" {name}(" in hdr
        assert hasattr(L, name), f"libvoxproj.so has no {name}"
    assert L.vp_abi_version() == voxproj_host.VP_ABI_VERSION == 4       # detected by symbol: the version did not move
    assert (voxproj_host.VP_FEATURE_LOSS_COSINE, voxproj_host.VP_FEATURE_LOSS_L2) == (0, 1)
    assert "#define VP_FEATURE_LOSS_COSINE 0" in hdr and "#define VP_FEATURE_LOSS_L2     1" in hdr


def test_workspace_size_function():
    size = voxproj_host.feature_loss_workspace_bytes
    for W, H in [(0, 5), (5, 0), (-1, 5), (32769, 1), (1, 32769)]:
        assert size(W, H) == 0
    last = 0
    for W, H in [(1, 1), (16, 16), (37, 19), (130, 67), (1600, 1067), (32768, 32768)]:
        b = size(W, H)
        assert b > 0 and b % 256 == 0 and b >= last
        assert b >= 16 * W * H                                         # the per-pixel coefficients alone
        last = b
    assert size(32768, 32768) > 2 ** 34                                # a size_t, not an int


def _fake_buffers():
    buf = ctypes.create_string_buffer(8192 + 256)
    ws = (ctypes.addressof(buf) + 255) & ~255            # never dereferenced: every call below is refused before a launch
    return buf, ws


def test_loss_call_host_side_refusals_need_no_gpu():
    L = voxproj_host.lib()
    buf, ws = _fake_buffers()
    C = 24
    need = voxproj_host.feature_loss_workspace_bytes(8, 4)
    assert need <= 8192
    order = ("image", "f16", "pix_stride", "target", "tgt_stride", "C", "W", "H", "weight", "alpha", "min_alpha", "kind", "stats",
             "pixel_loss", "ws", "ws_bytes")

    def call(**over):
        a = dict(image=ws, f16=1, pix_stride=C, target=ws, tgt_stride=C, C=C, W=8, H=4, weight=None, alpha=None, min_alpha=0.0,
                 kind=0, stats=ws, pixel_loss=None, ws=ws, ws_bytes=8192)
        assert set(over) <= set(a), over
        a.update(over)
        return L.vp_feature_loss(*[a[k] for k in order], None)

    for rc, over in [(EINVAL, dict(image=None)), (EINVAL, dict(target=None)), (EINVAL, dict(stats=None)), (EINVAL, dict(kind=2)),
                     (EINVAL, dict(kind=-1)), (EINVAL, dict(f16=2)), (EINVAL, dict(f16=-1)), (EINVAL, dict(C=0)),
                     (EINVAL, dict(C=4097, pix_stride=4097, tgt_stride=4097)), (EINVAL, dict(W=0)), (EINVAL, dict(W=32769)),
                     (EINVAL, dict(H=0)), (EINVAL, dict(H=32769)), (EINVAL, dict(pix_stride=C - 1)),
                     (EINVAL, dict(tgt_stride=C - 1)), (EWORKSPACE, dict(ws=None)), (EWORKSPACE, dict(ws=ws + 16)),
                     (EWORKSPACE, dict(ws_bytes=need - 1))]:
        assert call(**over) == rc, over
        assert voxproj_host.last_error()
    assert buf.raw == bytes(len(buf)), "a refused call wrote into its buffers"


def test_gradient_call_host_side_refusals_need_no_gpu():
    L = voxproj_host.lib()
    buf, ws = _fake_buffers()
    C = 24
    need = voxproj_host.feature_loss_workspace_bytes(8, 4)
    order = ("image", "f16", "pix_stride", "target", "tgt_stride", "C", "W", "H", "stats", "reduction", "grad_loss", "grad",
             "grad_stride", "k", "ws", "ws_bytes")

    def call(**over):
        a = dict(image=ws, f16=0, pix_stride=C, target=ws, tgt_stride=C, C=C, W=8, H=4, stats=ws, reduction=1, grad_loss=None,
                 grad=ws, grad_stride=C, k=ws, ws=ws, ws_bytes=8192)
        assert set(over) <= set(a), over
        a.update(over)
        return L.vp_feature_loss_gradient(*[a[k] for k in order], None)

    for rc, over in [(EINVAL, dict(image=None)), (EINVAL, dict(target=None)), (EINVAL, dict(stats=None)), (EINVAL, dict(grad=None)),
                     (EINVAL, dict(k=None)), (EINVAL, dict(reduction=2)), (EINVAL, dict(reduction=-1)), (EINVAL, dict(f16=2)),
                     (EINVAL, dict(C=0)), (EINVAL, dict(C=4097, pix_stride=4097, tgt_stride=4097, grad_stride=4097)),
                     (EINVAL, dict(W=0)), (EINVAL, dict(W=32769)), (EINVAL, dict(H=0)), (EINVAL, dict(H=32769)),
                     (EINVAL, dict(pix_stride=C - 1)), (EINVAL, dict(tgt_stride=C - 1)), (EINVAL, dict(grad_stride=C - 1)),
                     (EWORKSPACE, dict(ws=None)), (EWORKSPACE, dict(ws=ws + 16)), (EWORKSPACE, dict(ws_bytes=need - 1))]:
        assert call(**over) == rc, over
        assert voxproj_host.last_error()
    assert buf.raw == bytes(len(buf)), "a refused call wrote into its buffers"


def test_python_wrappers_check_their_arguments_before_the_gpu():
    img = torch.zeros((4, 8, 16), dtype=torch.float16)
    with pytest.raises(ValueError, match="kind"):
        voxproj_host.feature_loss(img, img, kind="l1")
    with pytest.raises(ValueError, match="CUDA"):                      # there is no CPU path
        voxproj_host.feature_loss(img, img)
    with pytest.raises(ValueError, match="float16"):
        voxproj_host.feature_loss(img, img.float())                    # the map is binary16
    with pytest.raises(ValueError, match="reduction"):
        voxproj_host.feature_loss_gradient(img, img, torch.zeros(2, dtype=torch.float64), voxproj_host.SplatWorkspace(),
                                           reduction="max")
    with pytest.raises(ValueError, match="CUDA"):
        voxproj_host.feature_loss_gradient(img, img, torch.zeros(2, dtype=torch.float64), voxproj_host.SplatWorkspace())
    import splat_autograd
    z, q, o = torch.zeros((5, 3)), torch.zeros((5, 4)), torch.zeros(5)
    rows = torch.zeros((5, 16), dtype=torch.float16)
    args = (np.eye(4), np.eye(3), 8, 4, img)
    with pytest.raises(ValueError, match="rows only"):
        splat_autograd.splat_feature_loss(z.clone().requires_grad_(), q, z, o, rows, *args)
    with pytest.raises(ValueError, match="rows only"):
        splat_autograd.splat_feature_loss(z, q, z, o.clone().requires_grad_(), rows, *args)
    with pytest.raises(ValueError, match="kind"):
        splat_autograd.splat_feature_loss(z, q, z, o, rows, *args, kind="huber")
    with pytest.raises(ValueError, match="reduction"):
        splat_autograd.splat_feature_loss(z, q, z, o, rows, *args, reduction="none")
    with pytest.raises(ValueError, match="dtype"):
        splat_autograd.splat_feature_loss(z, q, z, o, rows, *args, dtype=torch.float64)
    with pytest.raises(ValueError, match="CUDA"):
        splat_autograd.splat_feature_loss(z, q, z, o, rows, *args)


def small_maps(seed=0, H=3, W=4, C=5):
    rng = np.random.default_rng(seed)
    image = rng.normal(size=(H, W, C)).astype(np.float32)
    target = rng.normal(size=(H, W, C)).astype(np.float16)
    weight = rng.uniform(0.5, 2.0, size=(H, W)).astype(np.float32)
    alpha = rng.uniform(0.3, 1.0, size=(H, W)).astype(np.float32)
    weight[0, 1] = 0.0
    weight[1, 2] = -1.0
    alpha[2, 0] = 0.1                                                  # below min_alpha = 0.25
    image[2, 3] = 0.0                                                  # a pixel nothing reaches: invalid for the cosine only
    return image, target, weight, alpha


@pytest.mark.parametrize("kind", fref.KINDS)
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_reference_gradient_agrees_with_finite_differences(kind, reduction):
    image, target, weight, alpha = small_maps()
    r = fref.feature_loss64(image, target, weight, alpha, 0.25, kind)
    assert r["valid"].sum() == (8 if kind == "cosine" else 9)
    assert not r["valid"][0, 1] and not r["valid"][1, 2] and not r["valid"][2, 0]
    s = 1.0 / r["stats"][1] if reduction == "mean" else 1.0
    G = fref.gradient64(r, s)

    def total(img):
        q = fref.feature_loss64(img, target, weight, alpha, 0.25, kind)
        return fref.mean_loss(q) if reduction == "mean" else q["stats"][0]

    h = 1e-6
    img64 = image.astype(np.float64)
    worst = 0.0
    for idx in np.ndindex(*image.shape):
        if not image[idx[0], idx[1]].any():
            continue                                                   # the zero row: the cosine is not differentiable there
        up, dn = img64.copy(), img64.copy()
        up[idx] += h
        dn[idx] -= h
        fd = (total(up) - total(dn)) / (2 * h)   # float64 perturbations stay float64
        worst = max(worst, abs(fd - G[idx]))
    assert worst <= 1e-8, worst
    assert not G[0, 1].any() and not G[1, 2].any() and not G[2, 0].any()


@pytest.mark.parametrize("kind", fref.KINDS)
def test_coefficients_are_the_analytic_gradient(kind):
    image, target, _, _ = small_maps(seed=1, H=3, W=4, C=7)
    image[2, 3] = 1.0                                                  # no zero row here
    r = fref.feature_loss64(image, target, kind=kind)
    o = torch.from_numpy(image.astype(np.float64)).requires_grad_()
    t = torch.from_numpy(target.astype(np.float64))
    if kind == "cosine":
        l = 1.0 - torch.nn.functional.cosine_similarity(o, t, dim=2, eps=0.0)
    else:
        l = ((o - t) ** 2).mean(dim=2)
    l.sum().backward()
    assert np.allclose(l.detach().numpy(), r["l"], rtol=1e-13, atol=1e-15)
    assert np.allclose(o.grad.numpy(), r["v"], rtol=1e-12, atol=1e-14)          # v = A t + B o, m = 1
    # the cosine's gradient is orthogonal to the row it is taken at; the L2's points from the map to the image
    if kind == "cosine":
        assert np.abs((r["v"] * r["o"]).sum(-1)).max() <= 1e-14
    else:
        assert np.allclose(r["v"], 2.0 / 7 * (r["o"] - r["t"]), rtol=1e-14)


def test_reference_invalid_pixels_ignore_nan_and_inf():
    image, target, weight, alpha = small_maps(seed=2)
    base = fref.feature_loss64(image, target, weight, alpha, 0.25, "cosine")
    image, target = image.copy(), target.copy()
    image[0, 1, 2] = np.nan                                            # weight 0
    target[1, 2, 0] = np.inf                                           # weight < 0
    image[2, 0, 1] = -np.inf                                           # alpha below the threshold
    r = fref.feature_loss64(image, target, weight, alpha, 0.25, "cosine")
    assert r["stats"] == base["stats"] and np.array_equal(r["v"], base["v"]) and np.isfinite(r["v"]).all()


@pytest.mark.parametrize("scale", [1.0, 1e-7, 3.1e-7, 2.0 ** -20, 6e4, 1e-30])
def test_exponent_rule_is_quantize_gradient_maps(scale):
    import splat_autograd
    rng = np.random.default_rng(5)
    G = (rng.normal(size=(7, 5, 3)) * scale).astype(np.float32)
    if scale in (1e-7, 2.0 ** -20):
        G = np.clip(G, -scale, scale)
        G[0, 0, 0] = scale                                             # a map whose maximum is 1e-7 / an exact power of two
    _, k = splat_autograd.quantize_gradient_map(torch.from_numpy(G))
    assert fref.exponent(np.abs(G).max()) == int(k)
    top = float(np.abs(G).max()) * 2.0 ** int(k)
    assert 2.0 ** 13 < top <= 2.0 ** 14
    if scale == 1e-7:
        assert int(k) == 37                                            # 2^-24 < 1e-7 <= 2^-23: 14 + 23


def test_exponent_rule_of_an_all_zero_map_and_the_cap():
    import splat_autograd
    _, k = splat_autograd.quantize_gradient_map(torch.zeros((4, 3, 2)))
    assert fref.exponent(0.0) == int(k) == 0
    _, k = splat_autograd.quantize_gradient_map(torch.full((1, 1, 1), 1e-40))
    assert fref.exponent(float(np.float32(1e-40))) == int(k) == 126
    assert fref.near_power_of_two(2.0 ** -7 * (1 + 1e-6)) and fref.near_power_of_two(2.0 ** 5 * (1 - 1e-6))
    assert not fref.near_power_of_two(1.5) and not fref.near_power_of_two(0.0)


def test_distill_cli_parser_and_output_schema(tmp_path):
    import distill_gaussian_features as dgf
    import lift_gaussian_features as lgf
    base = ["--gaussians_ply", "p.ply", "--cam_params", "c.json", "--features_dir", "f", "--out", "o.pt"]
    a = dgf.build_parser().parse_args(base)
    assert (a.init, a.loss, a.min_alpha, a.steps, a.views_per_step, a.seed) == (None, "cosine", 0.5, 200, 4, 0)
    assert (a.views, a.max_images, a.downsample_factor, a.principal_point, a.images_dir, a.weights_dir) == \
        (None, None, None, "center", "", None)
    a = dgf.build_parser().parse_args(base + ["--init", "l.pt", "--loss", "l2", "--min_alpha", "0.25", "--steps", "7",
                                              "--views_per_step", "2", "--lr", "0.5", "--seed", "3", "--views", "v0", "v1"])
    assert (a.init, a.loss, a.min_alpha, a.steps, a.views_per_step, a.lr, a.seed, a.views) == \
        ("l.pt", "l2", 0.25, 7, 2, 0.5, 3, ["v0", "v1"])
    for drop in range(0, 8, 2):
        with pytest.raises(SystemExit):
            dgf.build_parser().parse_args(base[:drop] + base[drop + 2:])
    with pytest.raises(SystemExit):
        dgf.build_parser().parse_args(base + ["--loss", "l1"])
    # the view arguments are the lift's, option for option and default for default
    lift = vars(lgf.build_parser().parse_args(base))
    mine = vars(dgf.build_parser().parse_args(base))
    shared = set(lift) - {"min_weight"}
    assert shared <= set(mine) and all(mine[k] == lift[k] for k in shared)
    assert set(mine) - set(lift) == {"init", "loss", "min_alpha", "steps", "views_per_step", "lr", "seed"}
    with pytest.raises(SystemExit):
        dgf.main(base + ["--steps", "-1"])
    with pytest.raises(SystemExit):
        dgf.main(base + ["--min_alpha", "1.5"])
    # the output is LIFTED.pt's schema: fp32 rows go out as f16 and come back through the lift's reader
    rows = torch.linspace(-2, 2, 20).reshape(5, 4)
    lgf.save_lifted(str(tmp_path / "d.pt"), torch.zeros((5, 3)), rows, torch.ones(5), ["v0", "v1"])
    xyz, feats, weight = lgf.load_lifted(str(tmp_path / "d.pt"))
    assert feats.dtype == torch.float16 and torch.equal(feats, rows.half()) and xyz.shape == (5, 3) and weight.shape == (5,)
    assert torch.load(str(tmp_path / "d.pt"))["views"] == ["v0", "v1"]
