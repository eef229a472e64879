"""The wide render without a GPU: the library's symbol and its host-side refusals, the float64 identities the GPU tests rely
on, the gradient map's quantisation rule, and the host side of the two command lines."""
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

import splat_lift_reference as lref  # noqa: E402
import splat_reference as ref  # noqa: E402
import voxproj_host  # noqa: E402
from test_splat_lift_cpu import small_scene  # noqa: E402


def test_library_exports_vp_splat_render():
    assert "vp_splat_render" in voxproj_host.EXPORTS
    L = voxproj_host.lib()
    assert hasattr(L, "vp_splat_render"), "libvoxproj.so has no vp_splat_render"
    assert L.vp_abi_version() == voxproj_host.VP_ABI_VERSION == 4       # detected by symbol: the version did not move


def test_host_side_refusals_need_no_gpu():
    L = voxproj_host.lib()
    buf = ctypes.create_string_buffer(4096 + 256)
    ws = (ctypes.addressof(buf) + 255) & ~255                 # never dereferenced: every call below is refused before a launch
    rows = out = ws
    C = 24

    def call(**over):
        a = dict(rows=rows, f16=1, C=C, row_stride=C, n=10, W=32, H=16, cap=100, sorted=0, out=out, out16=1, pix_stride=C,
                 alpha=None, status=None, ws=ws, ws_bytes=4096)
        assert set(over) <= set(a), over
        a.update(over)
        return L.vp_splat_render(*[a[k] for k in ("rows", "f16", "C", "row_stride", "n", "W", "H", "cap", "sorted", "out", "out16",
                                                  "pix_stride", "alpha", "status", "ws", "ws_bytes")], None)

    EINVAL, EWORKSPACE = -1, -2                          # VP_EINVAL, VP_EWORKSPACE of include/voxproj.h
    for rc, over in [(EINVAL, dict(rows=None)), (EINVAL, dict(out=None)), (EINVAL, dict(C=0)),
                     (EINVAL, dict(C=4097, row_stride=4097, pix_stride=4097)), (EINVAL, dict(row_stride=C - 1)),
                     (EINVAL, dict(pix_stride=C - 1)), (EINVAL, dict(sorted=2)), (EINVAL, dict(sorted=-1)),
                     (EINVAL, dict(f16=2)), (EINVAL, dict(f16=-1)), (EINVAL, dict(out16=2)), (EINVAL, dict(n=-1)),
                     (EINVAL, dict(n=2 ** 31)), (EINVAL, dict(W=0)), (EINVAL, dict(W=32769)), (EINVAL, dict(H=0)),
                     (EINVAL, dict(cap=-1)), (EINVAL, dict(cap=2 ** 31)),
                     (EWORKSPACE, dict(ws=None)), (EWORKSPACE, dict(ws=ws + 16))]:
        assert call(**over) == rc, over
        assert voxproj_host.last_error()
    assert buf.raw == bytes(len(buf)), "a refused call wrote into its buffers"


def test_python_wrappers_check_their_arguments_before_the_gpu():
    rows = torch.zeros((5, 8), dtype=torch.float16)
    ws = voxproj_host.SplatWorkspace()
    with pytest.raises(ValueError, match="sorted"):
        voxproj_host.splat_render(rows, 5, 8, 8, 10, ws, sorted=3)
    with pytest.raises(ValueError, match="CUDA"):                      # there is no CPU path
        voxproj_host.splat_render(rows, 5, 8, 8, 10, ws)
    with pytest.raises(ValueError, match="CUDA"):
        voxproj_host.splat_render_view(torch.zeros((5, 3)), torch.zeros((5, 4)), torch.zeros((5, 3)), torch.zeros(5), rows,
                                       np.eye(4), np.eye(3), 8, 8)
    import splat_autograd
    z = torch.zeros((5, 3))
    with pytest.raises(ValueError, match="rows only"):
        splat_autograd.splat_wide_features(z.clone().requires_grad_(), torch.zeros((5, 4)), z, torch.zeros(5), rows, np.eye(4),
                                           np.eye(3), 8, 8)
    with pytest.raises(ValueError, match="rows only"):
        splat_autograd.splat_wide_features(z, torch.zeros((5, 4)), z, torch.zeros(5).requires_grad_(), rows, np.eye(4),
                                           np.eye(3), 8, 8)


def test_rendering_is_linear_in_the_rows():
    """What the 512-channel GPU case relies on: the float64 render of rows[:, c] * factor[c] is the render of rows[:, c] times
    factor[c] exactly when the factors are powers of two, and the decisions (fragile, visits, alpha) do not depend on the rows."""
    s, vm, K, W, H = small_scene(seed=6)
    rng = np.random.default_rng(3)
    base = rng.normal(size=(len(s["means"]), 4)).astype(np.float32)
    factor = np.array([1.0, -4.0, 0.5, -16.0, 2.0, 8.0, -1.0, 0.25, 4.0, -2.0])
    idx = np.arange(len(factor)) % 4
    a = ref.splat64(s["means"], s["quats"], s["scales"], s["opacities"], base, vm, K, W, H)
    b = ref.splat64(s["means"], s["quats"], s["scales"], s["opacities"], base.astype(np.float64)[:, idx] * factor, vm, K, W, H)
    assert (a["visits"] > 0).sum() > 100 and np.abs(a["logits"]).max() > 0.1
    assert np.array_equal(b["logits"], a["logits"][idx] * factor[:, None, None])
    assert np.array_equal(a["fragile"], b["fragile"]) and np.array_equal(a["visits"], b["visits"])
    assert np.array_equal(a["alpha"], b["alpha"])
    # and additive, to rounding: render(x + y) = render(x) + render(y)
    x, y = base.astype(np.float64), rng.normal(size=base.shape)
    c = ref.splat64(s["means"], s["quats"], s["scales"], s["opacities"], x + y, vm, K, W, H)
    d = ref.splat64(s["means"], s["quats"], s["scales"], s["opacities"], y, vm, K, W, H)
    assert np.allclose(c["logits"], a["logits"] + d["logits"], rtol=0, atol=1e-12)


def test_render_is_the_adjoint_of_the_lift_in_float64():
    s, vm, K, W, H = small_scene(seed=7)
    rng = np.random.default_rng(4)
    C = 6
    G = rng.normal(size=(H, W, C)).astype(np.float16)
    F = rng.normal(size=(len(s["means"]), C))
    o = ref.splat64(s["means"], s["quats"], s["scales"], s["opacities"], F, vm, K, W, H)
    r = lref.lift64(s["means"], s["quats"], s["scales"], s["opacities"], G, vm, K, W, H)
    lhs = (o["logits"].transpose(1, 2, 0) * G.astype(np.float64)).sum()
    assert abs(lhs) > 1.0 and lhs == pytest.approx((F * r["sum"]).sum(), rel=1e-11)


def quantize64(G):
    """The documented rule in NumPy: s = 2^(14 - ceil(log2 max|G|)), Gq = f16(G s)."""
    m = float(np.abs(G).max())
    if m == 0.0:
        return np.zeros(G.shape, np.float16), 1.0
    mant, ex = np.frexp(m)                                # m = mant 2^ex, mant in [0.5, 1): ceil(log2 m) = ex, or ex - 1 at 0.5
    s = 2.0 ** min(14 - (ex - 1 if mant == 0.5 else ex), 126)
    return (G.astype(np.float64) * s).astype(np.float16), s


@pytest.mark.parametrize("scale", [1.0, 1e-9, 3.1e-7, 2.0 ** -20, 6e4, 1e30])
def test_gradient_quantisation_rule(scale):
    import splat_autograd
    rng = np.random.default_rng(5)
    G = (rng.normal(size=(7, 5, 3)) * scale).astype(np.float32)
    if scale == 2.0 ** -20:
        G = np.clip(G, -scale, scale)
        G[0, 0, 0] = scale                                # the largest element an exact power of two: it lands on 2^14
    Gq, k = splat_autograd.quantize_gradient_map(torch.from_numpy(G))
    want, s = quantize64(G)
    assert Gq.dtype == torch.float16 and k.dtype == torch.int32 and 2.0 ** int(k) == s
    assert Gq.numpy().tobytes() == want.tobytes()
    top = np.abs(want.astype(np.float64)).max()
    assert 2.0 ** 13 < top <= 2.0 ** 14, "the largest element lands in (2^13, 2^14]"
    # nothing but the one rounding to binary16: every element within 2^-11 of itself or 2^-25 s^-1 (a subnormal), and
    # elements down to 2^-27 of the largest are still nonzero
    back = want.astype(np.float64) / s
    assert (np.abs(back - G) <= np.maximum(2.0 ** -11 * np.abs(G), 2.0 ** -25 / s)).all()
    assert (back[np.abs(G) > 2.0 ** -27 * np.abs(G).max()] != 0).all()


def test_gradient_quantisation_of_an_all_zero_map_and_of_tiny_values():
    import splat_autograd
    Gq, k = splat_autograd.quantize_gradient_map(torch.zeros((4, 3, 2)))
    assert int(k) == 0 and Gq.dtype == torch.float16 and not Gq.any()
    G = torch.full((2, 2, 1), 1e-9)
    G[0, 0, 0] = -2.5e-10
    Gq, k = splat_autograd.quantize_gradient_map(G)
    assert int(k) == 43                                   # 2^-30 < 1e-9 <= 2^-29: s = 2^(14 + 29)
    assert torch.equal(Gq.double() * 2.0 ** -43, (G.double() * 2.0 ** 43).half().double() * 2.0 ** -43)
    assert abs(float(Gq[1, 1, 0]) * 2.0 ** -43 - 1e-9) <= 2.0 ** -11 * 1e-9 and Gq.float().abs().min() > 2000
    with pytest.raises(ValueError):
        splat_autograd.quantize_gradient_map(torch.zeros((2, 2, 1), dtype=torch.float16))
    Gq, k = splat_autograd.quantize_gradient_map(torch.full((1, 1, 1), 1e-40))
    assert int(k) == 126 and float(Gq) > 0               # the exponent's cap


def test_render_cli_parser_and_scene_loading(tmp_path, monkeypatch):
    import lift_gaussian_features as lgf
    import render_gaussian_features as rgf
    base = ["--gaussians_ply", "p.ply", "--gauss_feats", "l.pt", "--cam_params", "c.json", "--out_dir", "o"]
    a = rgf.build_parser().parse_args(base)
    assert (a.views, a.max_images, a.downsample_factor, a.principal_point, a.images_dir, a.save_alpha) == \
        (None, None, None, "center", "", False)
    a = rgf.build_parser().parse_args(base + ["--views", "v0", "v1", "--save_alpha"])
    assert a.views == ["v0", "v1"] and a.save_alpha
    for drop in range(0, 8, 2):
        with pytest.raises(SystemExit):
            rgf.build_parser().parse_args(base[:drop] + base[drop + 2:])
    # the rows must match the point cloud
    geo = dict(means=np.zeros((5, 3), np.float32), quats=np.ones((5, 4), np.float32), scales=np.ones((5, 3), np.float32),
               opacities=np.ones(5, np.float32))
    monkeypatch.setattr(rgf.gaussian_ply, "read_gaussian_ply", lambda path: geo)
    feats = torch.arange(20, dtype=torch.float32).reshape(5, 4).to(torch.float16)
    lgf.save_lifted(str(tmp_path / "l.pt"), torch.zeros((5, 3)), feats, torch.ones(5), ["v"])
    args = rgf.build_parser().parse_args(base[:2] + ["--gauss_feats", str(tmp_path / "l.pt")] + base[4:])
    g, rows = rgf.load_scene(args, torch.device("cpu"))
    assert set(g) == set(geo) and rows.dtype == torch.float16 and torch.equal(rows, feats) and rows.is_contiguous()
    lgf.save_lifted(str(tmp_path / "short.pt"), torch.zeros((4, 3)), feats[:4], torch.ones(4), ["v"])
    args = rgf.build_parser().parse_args(base[:2] + ["--gauss_feats", str(tmp_path / "short.pt")] + base[4:])
    with pytest.raises(ValueError, match="4 rows"):
        rgf.load_scene(args, torch.device("cpu"))


def test_query_cli_gaussian_views_parser_and_label_rule(tmp_path, capsys):
    import query_voxel_features as qvf
    np.save(tmp_path / "t.npy", np.eye(3, 4, dtype=np.float32))
    base = ["gaussian_views", "--text_emb", str(tmp_path / "t.npy"), "--prompt", "a", "b", "c", "--gaussians_ply", "p.ply",
            "--gauss_feats", "l.pt", "--cam_params", "c.json", "--out_dir", "o"]
    a = qvf.build_parser().parse_args(base)
    assert (a.cmd, a.logit_scale, a.save_logits, a.views, a.downsample_factor, a.principal_point) == \
        ("gaussian_views", 1.0, False, None, None, "center")
    assert qvf.build_parser().parse_args(base + ["--save_logits", "--logit_scale", "14.5"]).save_logits
    with pytest.raises(SystemExit):
        qvf.build_parser().parse_args(base[:-2])                       # --out_dir is required
    with pytest.raises(SystemExit):
        qvf.main(base[:4] + ["a", "b"] + base[7:])                     # two prompts for three embedding rows
    assert "2 prompts for 3" in capsys.readouterr().err
    # the sub-command's view arguments are render_gaussian_features.py's, option for option and default for default
    import render_gaussian_features as rgf
    view_base = base[7:]
    mine, theirs = vars(qvf.build_parser().parse_args(base)), vars(rgf.build_parser().parse_args(view_base))
    shared = set(theirs) - {"save_alpha"}
    assert shared == set(mine) - {"cmd", "text_emb", "prompt", "logit_scale", "save_logits"}
    assert all(mine[k] == theirs[k] for k in shared)
    # the existing sub-commands parse as before
    v = qvf.build_parser().parse_args(["views", "--text_emb", "t", "--prompt", "a", "--features_pt", "f.pt"])
    assert v.cmd == "views" and v.out_dir == "semantic_views" and not hasattr(v, "gauss_feats")
    # label -1, confidence 0 and zero logits where alpha is 0 or the rendered row is all zeros
    H, W, C, P = 2, 3, 4, 3
    img = torch.zeros((H, W, C), dtype=torch.float16)
    img[0, 0, 1] = 2.0
    img[0, 1, 2] = 1.0                                                 # alpha 0 below
    img[1, 2, 0] = -3.0
    alpha = torch.tensor([[0.5, 0.0, 0.7], [0.2, 0.9, 1.0]])           # (0, 2), (1, 0), (1, 1): alpha > 0 but a row of zeros
    labels = torch.tensor([1, 2, 0, 0, 0, -1], dtype=torch.int32)      # the last row: non-finite in the query (label -1)
    margin = torch.full((H * W,), 0.25)
    logits = torch.arange(H * W * P, dtype=torch.float32).reshape(H * W, P) + 1.0
    lab, conf, lg = qvf.rendered_labels(img, alpha, labels, margin, logits)
    assert lab.dtype == torch.int32 and lab.tolist() == [[1, -1, -1], [-1, -1, -1]]
    assert conf.tolist() == [[0.25, 0, 0], [0, 0, 0]] and lg.shape == (H, W, P)
    assert lg[0, 0].tolist() == [1.0, 2.0, 3.0] and not lg.reshape(-1, P)[1:].any()
    lab2, conf2, none = qvf.rendered_labels(img, torch.ones((H, W)), torch.zeros(H * W, dtype=torch.int32), margin)
    assert none is None and lab2.tolist() == [[0, 0, -1], [-1, -1, 0]] and conf2[1, 2] == 0.25
