"""The photometric loss without a GPU: (a) the float64 statement of tests/photo_loss_reference.py against recorded results of
the reference's own l1_loss / ssim and their autograd gradient, (b) the derived fp32 bounds against an fp32 torch composite
of the same formula on every input the GPU test runs, (c) the library's three symbols, its workspace formula and its
host-side refusals.  Everything that touches the library fails on a tree without vp_photo_loss."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import photo_loss_reference as pref  # noqa: E402
import voxproj_host  # noqa: E402

SYMBOLS = ("vp_photo_loss_workspace_bytes", "vp_photo_loss", "vp_photo_loss_gradient")
EINVAL, EWORKSPACE = -1, -2                              # VP_EINVAL, VP_EWORKSPACE of include/voxproj.h
NAN, INF = float("nan"), float("inf")
GOLDEN = os.path.join(HERE, "golden", "photo_loss_golden.npz")


# ---------------------------------------------------------------- (a) the statement against the reference's recorded results
def test_row_is_the_reference_gaussian_and_the_header_lists_it():
    import math
    g = np.array([math.exp(-(i - 5) ** 2 / 4.5) for i in range(11)]).astype(np.float32)
    row = pref.ROW.astype(np.float32)
    assert (row.astype(np.float64) == pref.ROW).all()                    # fp32 numbers
    # the fp32 sum's last bit depends on the order of the additions: every order lands within 2 ulp of the recorded row
    assert np.abs(row - g / g.sum(dtype=np.float32)).max() <= 2 * 2.0 ** -24 * row.max()
    assert abs(pref.ROW.sum() - 1) < 1e-6 and (row == row[::-1]).all()
    hdr = open(os.path.join(ROOT, "include", "voxproj.h")).read()
    import re
    listed = [float.fromhex(h) for h in re.findall(r"g\[\d+\](?: = g\[\d+\])?\s*= (0x1\.[0-9a-f]+p-\d+)", hdr)]
    assert listed == [float(v) for v in row[:6]], listed


def test_statement_matches_the_recorded_reference_results():
    gold = np.load(GOLDEN)
    lam = float(gold["lambda_dssim"])
    w2 = gold["window2d"]
    assert w2.dtype == np.float32 and w2.shape == (11, 11)
    # the reference's window is the row's outer product rounded to fp32: one more rounding per weight, nothing else
    assert np.array_equal(w2, np.outer(pref.ROW.astype(np.float32), pref.ROW.astype(np.float32)))
    assert np.abs(w2 - np.outer(pref.ROW, pref.ROW)).max() <= 2.0 ** -24 * w2.max()
    cases = [c.split(",") for c in gold["cases"]]
    assert len(cases) >= 5
    for i, (kind, C, W, H, seed) in enumerate(cases):
        x, y = gold[f"x{i}"], gold[f"y{i}"]
        mx, my = pref.make_inputs(kind, int(C), int(W), int(H), int(seed))
        assert np.array_equal(x, mx) and np.array_equal(y, my), "the seeded inputs moved"
        ref = pref.statement64(x, y, lambda_dssim=lam, window2d=w2)
        n = x.size
        assert abs(ref["stats"][0] / n - gold[f"l1_{i}"]) <= 1e-12 * max(abs(gold[f"l1_{i}"]), 1e-300) or kind == "equal"
        assert abs(ref["stats"][2] / n - gold[f"ssim_{i}"]) <= 1e-12 * abs(gold[f"ssim_{i}"])
        assert abs(ref["loss"] - gold[f"loss_{i}"]) <= 1e-12 * abs(gold[f"loss_{i}"])
        g = gold[f"grad_{i}"]
        # at x = y the gradient is analytically 0 (m is at its maximum, sgn(0) = 0): both sides are float64 noise there, and
        # the scale of the comparison is the L1 part's size, (1 - lambda) / n, instead of the noise's own
        scale = (1 - lam) / n if kind == "equal" else np.abs(g).max()
        assert np.abs(ref["grad"] - g).max() <= 1e-12 * scale, (kind, np.abs(ref["grad"] - g).max(), scale)
        if kind == "equal":
            assert ref["stats"][0] == 0 and gold[f"l1_{i}"] == 0 and abs(ref["stats"][2] / n - 1) < 1e-12
        # the contract's window (exact products) against the reference's (rounded products): inside the fp32 bounds by far
        own = pref.statement64(x, y, lambda_dssim=lam)
        bnd = pref.bounds(x, y, lambda_dssim=lam)
        assert (np.abs(own["m"] - ref["m"]) <= 0.1 * bnd["m"]).all()
        assert (np.abs(own["grad"] - ref["grad"]) <= 0.1 * bnd["grad"]).all()


# ---------------------------------------------------------------- (b) the bounds against an fp32 composite
def _composite32(x, y, lam):
    """The formula in fp32 torch on the CPU, the window as two 11-tap passes, the gradient by autograd."""
    row = torch.from_numpy(pref.ROW.astype(np.float32))
    C = x.shape[0]
    wh, wv = row.view(1, 1, 1, 11).repeat(C, 1, 1, 1), row.view(1, 1, 11, 1).repeat(C, 1, 1, 1)

    def ws(a):
        return F.conv2d(F.conv2d(a[None], wh, padding=(0, 5), groups=C), wv, padding=(5, 0), groups=C)[0]

    xt = torch.from_numpy(x).clone().requires_grad_(True)
    yt = torch.from_numpy(y)
    mu1, mu2 = ws(xt), ws(yt)
    s1, s2, s12 = ws(xt * xt) - mu1 * mu1, ws(yt * yt) - mu2 * mu2, ws(xt * yt) - mu1 * mu2
    m = ((2 * mu1 * mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1 * mu1 + mu2 * mu2 + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    loss = (1 - lam) * (xt - yt).abs().mean() + lam * (1 - m.mean())
    loss.backward()
    return m.detach().numpy(), xt.grad.numpy()


def test_bounds_hold_for_an_fp32_composite_and_are_not_vacuous():
    lam = 0.2
    worst_m = worst_g = 0.0
    largest = 0.0
    for kind, C, W, H, seed in pref.gpu_cases():
        x, y = pref.make_inputs(kind, C, W, H, seed)
        ref = pref.statement64(x, y, lambda_dssim=lam)
        bnd = pref.bounds(x, y, lambda_dssim=lam)
        m32, g32 = _composite32(x, y, lam)
        em, eg = np.abs(m32 - ref["m"]), np.abs(g32 - ref["grad"])
        assert (bnd["m"] > 0).all() and (bnd["grad"] >= 0).all()        # 0: an element whose every term is an exact zero
        assert bnd["m"].max() <= 1.0, (kind, C, W, H, bnd["m"].max())   # m lies in [-1, 1]: half the range
        largest = max(largest, float(bnd["m"].max()))
        assert (eg[bnd["grad"] == 0] == 0).all()
        rm, rg = float((em / bnd["m"]).max()), float((eg / np.where(bnd["grad"] > 0, bnd["grad"], 1.0)).max())
        worst_m, worst_g = max(worst_m, rm), max(worst_g, rg)
        assert rm <= 1.0, (kind, C, W, H, rm)
        assert rg <= 1.0, (kind, C, W, H, rg)
        print(f"{kind:7s} C={C} {W}x{H}: m {rm:.3f} of bound max {bnd['m'].max():.2e}; gradient {rg:.3f}, bound max "
              f"{bnd['grad'].max() * x.size:.2e} / n beside |grad| max {np.abs(ref['grad']).max() * x.size:.2e} / n")
    print(f"fp32 composite: worst error / bound {worst_m:.3f} (m), {worst_g:.3f} (gradient); largest bound on m {largest:.3e}")
    assert worst_m > 1e-4 and worst_g > 1e-4                             # the bound is within four decades of a real error


def test_smooth_images_need_the_derived_bound():
    """The cancellation the bound exists for: on a smooth image the fp32 map is off by far more than on noise."""
    xs, ys = pref.make_inputs("smooth", 3, 130, 67, 1)
    xn, yn = pref.make_inputs("noise", 3, 130, 67, 1)
    bs, bn = pref.bounds(xs, ys)["m"].max(), pref.bounds(xn, yn)["m"].max()
    assert bs > 20 * bn


# ---------------------------------------------------------------- (c) the library on the host
def test_library_exports_the_three_symbols():
    L = voxproj_host.lib()
    hdr = open(os.path.join(ROOT, "include", "voxproj.h")).read()
    for name in SYMBOLS:
        assert name in voxproj_host.EXPORTS and f" {name}(" in hdr
        assert hasattr(L, name), f"libvoxproj.so has no {name}"
    assert L.vp_abi_version() == voxproj_host.VP_ABI_VERSION == 4       # detected by symbol: the version did not move


def test_workspace_size_function():
    size = voxproj_host.photo_loss_workspace_bytes
    for C, W, H in [(0, 5, 5), (65, 5, 5), (-1, 5, 5), (3, 0, 5), (3, 5, 0), (3, -1, 5), (3, 32769, 1), (3, 1, 32769)]:
        assert size(C, W, H) == 0

    def a256(v):
        return (v + 255) // 256 * 256
    T = pref.TILE
    for C in (1, 3, 4, 64):
        for W, H in [(1, 1), (5, 7), (T, T), (T + 1, T), (T, T + 1), (37, 21), (130, 67), (1600, 1067), (32768, 32768)]:
            tiles = C * ((W + T - 1) // T) * ((H + T - 1) // T)
            assert size(C, W, H) == a256(12 * C * W * H) + a256(24 * tiles)          # the header's formula


def _fake_buffers(nbytes):
    buf = ctypes.create_string_buffer(nbytes + 256)
    ws = (ctypes.addressof(buf) + 255) & ~255            # never dereferenced: every call below is refused before a launch
    return buf, ws


def test_loss_call_host_side_refusals_need_no_gpu():
    L = voxproj_host.lib()
    need = voxproj_host.photo_loss_workspace_bytes(3, 8, 4)
    buf, ws = _fake_buffers(need)
    order = ("image", "target", "C", "W", "H", "stats", "ssim_map", "ws", "ws_bytes")

    def call(**over):
        a = dict(image=ws, target=ws, C=3, W=8, H=4, stats=ws, ssim_map=None, ws=ws, ws_bytes=need)
        assert set(over) <= set(a), over
        a.update(over)
        return L.vp_photo_loss(*[a[k] for k in order], None)

    for rc, over in [(EINVAL, dict(image=None)), (EINVAL, dict(target=None)), (EINVAL, dict(stats=None)), (EINVAL, dict(C=0)),
                     (EINVAL, dict(C=65)), (EINVAL, dict(W=0)), (EINVAL, dict(W=32769)), (EINVAL, dict(H=0)),
                     (EINVAL, dict(H=32769)), (EWORKSPACE, dict(ws=ws + 16)), (EWORKSPACE, dict(ws_bytes=need - 1)),
                     (EWORKSPACE, dict(ws_bytes=0))]:
        assert call(**over) == rc, over
        assert voxproj_host.last_error()
    assert buf.raw == bytes(len(buf)), "a refused call wrote into its buffers"


def test_gradient_call_host_side_refusals_need_no_gpu():
    L = voxproj_host.lib()
    need = voxproj_host.photo_loss_workspace_bytes(3, 8, 4)
    buf, ws = _fake_buffers(need)
    order = ("image", "target", "C", "W", "H", "lam", "grad_loss", "grad", "ws", "ws_bytes")

    def call(**over):
        a = dict(image=ws, target=ws, C=3, W=8, H=4, lam=0.2, grad_loss=None, grad=ws, ws=ws, ws_bytes=need)
        assert set(over) <= set(a), over
        a.update(over)
        return L.vp_photo_loss_gradient(*[a[k] for k in order], None)

    for rc, over in [(EINVAL, dict(image=None)), (EINVAL, dict(target=None)), (EINVAL, dict(grad=None)), (EINVAL, dict(C=0)),
                     (EINVAL, dict(C=65)), (EINVAL, dict(W=0)), (EINVAL, dict(W=32769)), (EINVAL, dict(H=0)),
                     (EINVAL, dict(H=32769)), (EINVAL, dict(lam=NAN)), (EINVAL, dict(lam=INF)), (EINVAL, dict(lam=-0.01)),
                     (EINVAL, dict(lam=1.01)), (EWORKSPACE, dict(ws=None)), (EWORKSPACE, dict(ws=ws + 16)),
                     (EWORKSPACE, dict(ws_bytes=need - 1))]:
        assert call(**over) == rc, over
        assert voxproj_host.last_error()
    assert buf.raw == bytes(len(buf)), "a refused call wrote into its buffers"


def test_python_wrappers_check_their_arguments_before_the_gpu():
    img = torch.zeros((3, 4, 5), dtype=torch.float32)
    with pytest.raises(ValueError):
        voxproj_host.photo_loss(img.double(), img)
    with pytest.raises(ValueError):
        voxproj_host.photo_loss(img, img.double())
    with pytest.raises(ValueError):
        voxproj_host.photo_loss(img, img[:, :3])
    with pytest.raises(ValueError):
        voxproj_host.photo_loss(torch.zeros((65, 4, 5)), torch.zeros((65, 4, 5)))
    with pytest.raises(ValueError):
        voxproj_host.photo_loss_gradient(img, img, None, lambda_dssim=0.2)


def test_image_metrics_arithmetic():
    m = voxproj_host.image_metrics([30.0, 3.0, 150.0], 300)
    assert m["l1"] == 0.1 and m["ssim"] == 0.5 and abs(m["psnr"] - 20.0) < 1e-12
    assert voxproj_host.image_metrics(torch.tensor([0.0, 0.0, 12.0], dtype=torch.float64), 12)["psnr"] == float("inf")
