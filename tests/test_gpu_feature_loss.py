"""vp_feature_loss and vp_feature_loss_gradient on the GPU against the float64 statement of tests/feature_loss_reference.py,
on random images: no Gaussians are involved.  The bounds are derived in that file's docstring; every pixel and every
element is checked, because these inputs contain no fragile decision.

Shapes.  C in {1, 7, 8, 72, 512, 520, 4096}: the element path (1, 7), exactly one 16-byte load in one lane (8), a lane tail
(72: 9 of 64 lanes), every lane loaded once (512), a second chunk with one lane (520), the register limit (4096: 8 chunks).
W x H in {1x1, 37x19, 130x67}: one pixel, three workgroups with a tail, and 35 workgroups (the halving tree and the ordered
sum over workgroups).  C = 4096 is run at 1x1 and 37x19 only: the kernel's path depends on C alone, and the float64 reference
of 130 x 67 x 4096 elements would take the test from seconds to a minute.  Both image dtypes and both kinds are crossed with
these; SUM / MEAN with and without grad_loss, pixel strides of C and C + 24 and a base offset by one element (which forces
the element path) are drawn per case with a seeded generator, and test_layout_and_reduction_variants crosses them in full
at C = 72 and C = 8.  257 x 256 at C = 8 has 257 workgroups: one more than k_feature_loss_sum stages at a time.

The one ill-posed comparison: with C = 1 the cosine of two scalars is +-1 and its gradient is identically zero, so the
float64 maximum is rounding noise (or 0) and fixes no exponent.  There the device's k is checked against the device's own
largest element only; every other check runs as everywhere else.

Every test here fails on a library without the three vp_feature_loss symbols."""
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

import feature_loss_reference as fref  # noqa: E402
import voxproj_host  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CANARY16 = 0x5A5A
KIND = {"cosine": 0, "l2": 1}
REDUCTION = {"sum": 0, "mean": 1}
NEAR_POWER_EXITS = []                                     # the cases that took the +-1 exit of the exponent check


def strided(values, pad=0, offset=0, canary=float("nan")):
    """values [H,W,C] (numpy) as a device view with pixel stride C + pad, `offset` elements into a flat buffer whose every
    other element is `canary`: (view, flat)."""
    H, W, C = values.shape
    stride = C + pad
    t = torch.from_numpy(values)
    flat = torch.full((offset + H * W * stride + 8,), canary, dtype=t.dtype, device=DEV)
    view = torch.as_strided(flat, (H, W, C), (W * stride, stride, 1), offset)
    view.copy_(t.to(DEV))
    return view, flat


def run(image, target, weight=None, alpha=None, min_alpha=0.0, kind="cosine", reduction="mean", grad_loss=None, gpad=0, goff=0):
    """Both calls through the C ABI on buffers with canaries round every output.  image / target: device views [H,W,C].
    Returns a dict of numpy results; asserts the canaries."""
    L = voxproj_host.lib()
    H, W, C = (int(v) for v in image.shape)
    n = H * W
    ws = voxproj_host.SplatWorkspace()
    ptr = ws.ensure(voxproj_host.feature_loss_workspace_bytes(W, H), DEV)
    stats = torch.full((4,), -7.25, dtype=torch.float64, device=DEV)
    pl = torch.full((n + 2,), -7.25, dtype=torch.float32, device=DEV)
    gstride = C + gpad
    gflat = torch.full((goff + n * gstride + 8,), CANARY16, dtype=torch.int16, device=DEV)
    kbuf = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    w = torch.from_numpy(weight).to(DEV) if weight is not None else None
    a = torch.from_numpy(alpha).to(DEV) if alpha is not None else None
    g = torch.tensor([grad_loss], dtype=torch.float32, device=DEV) if grad_loss is not None else None
    stream = torch.cuda.current_stream(DEV).cuda_stream
    f16 = int(image.dtype == torch.float16)
    esz = gflat.element_size()
    rc = L.vp_feature_loss(image.data_ptr(), f16, int(image.stride(1)), target.data_ptr(), int(target.stride(1)), C, W, H,
                           voxproj_host._ptr(w), voxproj_host._ptr(a), float(min_alpha), KIND[kind], stats.data_ptr() + 8,
                           pl.data_ptr() + 4, ptr, ws.capacity(), stream)
    assert rc == 0, voxproj_host.last_error()
    rc = L.vp_feature_loss_gradient(image.data_ptr(), f16, int(image.stride(1)), target.data_ptr(), int(target.stride(1)), C, W, H,
                                    stats.data_ptr() + 8, REDUCTION[reduction], voxproj_host._ptr(g),
                                    gflat.data_ptr() + goff * esz, gstride, kbuf.data_ptr() + 4, ptr, ws.capacity(), stream)
    assert rc == 0, voxproj_host.last_error()
    torch.cuda.synchronize()
    stats_h, pl_h, k_h, g_h = stats.cpu().numpy(), pl.cpu().numpy(), kbuf.cpu().numpy(), gflat.cpu().numpy()
    assert stats_h[0] == -7.25 and stats_h[3] == -7.25, "loss_stats' neighbours were written"
    assert pl_h[0] == -7.25 and pl_h[-1] == -7.25, "pixel_loss' neighbours were written"
    assert k_h[0] == 0x5A5A5A5A and k_h[2] == 0x5A5A5A5A, "grad_exponent's neighbours were written"
    assert (g_h[:goff] == CANARY16).all() and (g_h[goff + n * gstride:] == CANARY16).all(), "the gradient image's ends were written"
    body = g_h[goff:goff + n * gstride].reshape(n, gstride)
    assert (body[:, C:] == CANARY16).all(), "padding elements of the gradient image were written"
    grad = np.ascontiguousarray(body[:, :C]).view(np.float16).reshape(H, W, C)
    return dict(stats=stats_h[1:3].copy(), pixel_loss=pl_h[1:-1].reshape(H, W).copy(), k=int(k_h[1]), grad=grad)


def check(out, image_np, target_np, weight=None, alpha=None, min_alpha=0.0, kind="cosine", reduction="mean", grad_loss=None):
    """Every check of the contract on one result of run()."""
    r = fref.feature_loss64(image_np, target_np, weight, alpha, min_alpha, kind)
    C = r["C"]
    # per-pixel loss: m l within m bound + one rounding of the product; exactly 0 at invalid pixels
    bound = r["m"] * (fref.loss_bound(r) + fref.U * r["l"])
    err = np.abs(out["pixel_loss"].astype(np.float64) - r["pixel_loss"])
    worst = float((err / np.maximum(bound, 1e-300)).max()) if r["valid"].any() else 0.0
    print(f"per-pixel loss: worst {worst:.3f} of the bound ({kind}, C = {C})")
    assert (err <= bound).all(), f"per-pixel loss off by {worst:.3f} of the bound"
    assert not out["pixel_loss"][~r["valid"]].any() and np.isfinite(out["pixel_loss"]).all()
    # statistics
    e0 = abs(out["stats"][0] - r["stats"][0])
    print(f"loss_stats: {out['stats']} against {r['stats']}, error {e0:.3e} of {fref.stats_bound(r):.3e}")
    assert e0 <= fref.stats_bound(r)
    assert abs(out["stats"][1] - r["stats"][1]) <= 1e-12 * r["stats"][1]
    # the scalar, the exponent, the image
    s = fref.scalar(r, reduction, 1.0 if grad_loss is None else grad_loss)
    x64 = abs(s) * r["vmax"]
    k, grad = out["k"], out["grad"]
    top = float(np.abs(grad.astype(np.float64)).max())
    degenerate = kind == "cosine" and C == 1                    # the gradient is identically zero: see the module docstring
    if x64 == 0.0 and not degenerate:
        assert top == 0.0 and k == 0
    elif not degenerate:
        want = fref.exponent(x64)
        if k != want:
            assert fref.near_power_of_two(x64) and abs(k - want) == 1, f"exponent {k}, reference {want} for a maximum of {x64!r}"
            NEAR_POWER_EXITS.append((kind, C, x64))
            assert len(NEAR_POWER_EXITS) <= 1, NEAR_POWER_EXITS
    if top > 0.0:
        assert 2.0 ** 12 < top <= 2.0 ** 14, f"the largest element is {top}"
    else:
        assert k == 0
    G = fref.gradient64(r, s)
    gb = fref.gradient_bound(r, s, k)
    gerr = np.abs(fref.dequantised(grad, k) - G)
    gw = float((gerr / gb).max())
    print(f"gradient: worst {gw:.3f} of the bound, k = {k}, largest element {top}")
    assert (gerr <= gb).all(), f"gradient off by {gw:.3f} of the bound"
    assert not grad[~r["valid"]].view(np.uint16).any(), "an invalid pixel's gradient row is not all zero bytes"
    return r


def maps(C, W, H, f16, seed):
    rng = np.random.default_rng(seed)
    image = rng.normal(size=(H, W, C)).astype(np.float16 if f16 else np.float32)
    target = rng.normal(size=(H, W, C)).astype(np.float16)
    weight = rng.uniform(0.25, 4.0, size=(H, W)).astype(np.float32)
    alpha = rng.uniform(0.0, 1.0, size=(H, W)).astype(np.float32)
    return image, target, weight, alpha


SIZES = [(1, 1), (37, 19), (130, 67)]
CHANNELS = [1, 7, 8, 72, 512, 520, 4096]
SWEEP = [(C, W, H) for C in CHANNELS for (W, H) in SIZES if not (C == 4096 and (W, H) == (130, 67))]


@pytest.mark.parametrize("kind", fref.KINDS)
@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("C,W,H", SWEEP)
def test_against_float64(C, W, H, f16, kind):
    seed = C * 1000 + W * 10 + int(f16) * 2 + KIND[kind]
    rng = np.random.default_rng(seed + 77)
    reduction = ("mean", "sum")[int(rng.integers(2))]
    grad_loss = (None, 0.37, -2.5)[int(rng.integers(3))]
    pad, gpad = 24 * int(rng.integers(2)), 24 * int(rng.integers(2))
    off = int(rng.integers(3)) == 0
    use_weight, use_alpha = bool(rng.integers(2)), bool(rng.integers(2))
    image, target, weight, alpha = maps(C, W, H, f16, seed)
    kw = dict(weight=weight if use_weight else None, alpha=alpha if use_alpha else None, min_alpha=0.2, kind=kind,
              reduction=reduction, grad_loss=grad_loss)
    print(f"variant: {reduction}, grad_loss {grad_loss}, strides C + {pad} / C + {gpad}, offset {int(off)}, weight {use_weight}, alpha {use_alpha}")
    iv, _ = strided(image, pad, int(off))
    tv, _ = strided(target, pad, int(off))
    out = run(iv, tv, gpad=gpad, goff=int(off), **kw)
    check(out, image, target, **kw)


@pytest.mark.parametrize("kind", fref.KINDS)
@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
def test_more_workgroups_than_one_staging_of_the_sum(f16, kind):
    """k_feature_loss_sum stages FLOSS_THREADS = 256 workgroup pairs at a time and a workgroup of the loss kernel holds 256
    pixels: a second staging iff W H > 256 * 256 = 65 536.  257 x 256 pixels are 257 workgroups: the second staging holds the
    pair of workgroup 256 alone, the pixels 65 536.. (the last image row from x = 1 on), which are all valid here and carry
    the largest weights of the image: without them both statistics leave their bounds by orders of magnitude."""
    C, W, H = 8, 257, 256
    assert (W * H + 255) // 256 == 257
    image, target, weight, alpha = maps(C, W, H, f16, seed=257 + int(f16) * 2 + KIND[kind])
    weight.reshape(-1)[65536:] = np.float32(6.0)
    alpha.reshape(-1)[65536:] = np.float32(0.9)
    kw = dict(weight=weight, alpha=alpha, min_alpha=0.2, kind=kind, reduction="mean", grad_loss=0.37)
    out = run(strided(image)[0], strided(target)[0], **kw)
    r = check(out, image, target, **kw)
    last = r["valid"].reshape(-1)[65536:]
    assert last.all() and r["m"].reshape(-1)[65536:].sum() > 1e3 * fref.stats_bound(r)


@pytest.mark.parametrize("goff", [0, 1])
@pytest.mark.parametrize("pad", [0, 24])
@pytest.mark.parametrize("grad_loss", [None, 0.37])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("C", [8, 72])
def test_layout_and_reduction_variants(C, f16, reduction, grad_loss, pad, goff):
    W, H = 37, 19
    image, target, weight, alpha = maps(C, W, H, f16, seed=C + 5)
    kw = dict(weight=weight, alpha=alpha, min_alpha=0.2, kind="cosine", reduction=reduction, grad_loss=grad_loss)
    iv, _ = strided(image, pad, goff)
    tv, _ = strided(target, pad, goff)
    out = run(iv, tv, gpad=pad, goff=goff, **kw)
    check(out, image, target, **kw)
    # the layout does not change a bit: the contiguous, aligned call gives the same results
    base = run(*(strided(x)[0] for x in (image, target)), **kw)
    assert base["stats"].tobytes() == out["stats"].tobytes() and base["k"] == out["k"]
    assert base["pixel_loss"].tobytes() == out["pixel_loss"].tobytes() and base["grad"].tobytes() == out["grad"].tobytes()


@pytest.mark.parametrize("kind", fref.KINDS)
@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
def test_invalid_pixels(f16, kind):
    C, W, H = 72, 37, 19
    image, target, weight, alpha = maps(C, W, H, f16, seed=11)
    alpha = np.maximum(alpha, np.float32(0.5))
    weight[0, 0], weight[3, 5], weight[18, 36] = 0.0, -1.5, -0.0         # 0, negative, -0: read as 0
    alpha[7, 7] = 0.25                                                  # below min_alpha = 0.4
    image[9, 1] = 0.0                                                   # a pixel nothing reaches
    target[10, 2] = 0.0                                                 # a map with an empty row
    alpha[12, 12] = np.nan                                              # not >= min_alpha
    weight[13, 13] = np.nan                                             # not > 0
    bad = [(0, 0), (3, 5), (18, 36), (7, 7), (12, 12), (13, 13)]
    image[0, 0, 3], image[3, 5, 70], image[18, 36, 0] = np.nan, np.inf, -np.inf
    target[7, 7, 1], target[12, 12, 71], target[13, 13, 8] = np.nan, np.inf, np.nan
    kw = dict(weight=weight, alpha=alpha, min_alpha=0.4, kind=kind, reduction="mean", grad_loss=None)
    out = run(strided(image)[0], strided(target)[0], **kw)
    r = check(out, image, target, **kw)
    for y, x in bad:
        assert not r["valid"][y, x] and out["pixel_loss"][y, x] == 0 and not out["grad"][y, x].view(np.uint16).any()
    assert r["valid"][9, 1] == r["valid"][10, 2] == (kind == "l2")      # the cosine needs both rows; the L2 does not
    assert r["valid"].sum() == W * H - len(bad) - (2 if kind == "cosine" else 0)
    # the neighbours are unaffected: the same maps with the invalid pixels' rows cleaned give the same bits elsewhere
    image2, target2 = image.copy(), target.copy()
    for y, x in bad:
        image2[y, x], target2[y, x] = 1.0, 1.0
    out2 = run(strided(image2)[0], strided(target2)[0], **kw)
    assert out2["stats"].tobytes() == out["stats"].tobytes() and out2["k"] == out["k"]
    assert out2["grad"].tobytes() == out["grad"].tobytes() and out2["pixel_loss"].tobytes() == out["pixel_loss"].tobytes()


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("kind", fref.KINDS)
def test_all_pixels_invalid(kind, reduction):
    C, W, H = 72, 37, 19
    image, target, weight, _ = maps(C, W, H, True, seed=12)
    image[2, 2, 2] = np.nan
    out = run(strided(image)[0], strided(target)[0], weight=np.zeros_like(weight), kind=kind, reduction=reduction)
    assert out["stats"].tobytes() == np.zeros(2).tobytes() and out["k"] == 0
    assert not out["grad"].view(np.uint16).any() and not out["pixel_loss"].view(np.uint32).any()
    # and a zero upstream gradient: zeros and k = 0 whatever the maps hold
    out = run(strided(image)[0], strided(target)[0], weight=weight, kind=kind, reduction=reduction, grad_loss=0.0)
    assert out["k"] == 0 and not out["grad"].view(np.uint16).any()


def test_two_runs_give_the_same_bytes():
    C, W, H = 520, 130, 67
    image, target, weight, alpha = maps(C, W, H, True, seed=13)
    iv, tv = strided(image)[0], strided(target)[0]
    kw = dict(weight=weight, alpha=alpha, min_alpha=0.1, kind="cosine", reduction="mean", grad_loss=0.37)
    a, b = run(iv, tv, **kw), run(iv, tv, **kw)
    assert a["stats"].tobytes() == b["stats"].tobytes() and a["k"] == b["k"]
    assert a["pixel_loss"].tobytes() == b["pixel_loss"].tobytes() and a["grad"].tobytes() == b["grad"].tobytes()


def test_python_wrappers_give_the_c_calls_bits():
    C, W, H = 72, 37, 19
    image, target, weight, alpha = maps(C, W, H, False, seed=14)
    iv, tv = strided(image, 24, 1)[0], strided(target, 24, 1)[0]
    kw = dict(weight=weight, alpha=alpha, min_alpha=0.3, kind="l2", reduction="sum", grad_loss=1.5)
    want = run(iv, tv, **kw)
    wt, at = torch.from_numpy(weight).to(DEV), torch.from_numpy(alpha).to(DEV)
    stats, pl, ws = voxproj_host.feature_loss(iv, tv, wt, at, kind="l2", min_alpha=0.3, want_pixel_loss=True)
    Gq, k = voxproj_host.feature_loss_gradient(iv, tv, stats, ws, reduction="sum",
                                               grad_loss=torch.tensor([1.5], device=DEV))
    assert stats.cpu().numpy().tobytes() == want["stats"].tobytes() and int(k) == want["k"] and k.dtype == torch.int32
    assert pl.cpu().numpy().tobytes() == want["pixel_loss"].tobytes() and Gq.cpu().numpy().tobytes() == want["grad"].tobytes()
    with pytest.raises(ValueError, match="workspace"):
        voxproj_host.feature_loss_gradient(iv, tv, stats, voxproj_host.SplatWorkspace())


def test_refused_calls_leave_every_output_untouched():
    L = voxproj_host.lib()
    C, W, H = 8, 5, 3
    image, target, _, _ = maps(C, W, H, True, seed=15)
    iv, tv = strided(image)[0], strided(target)[0]
    ws = voxproj_host.SplatWorkspace()
    ptr = ws.ensure(voxproj_host.feature_loss_workspace_bytes(W, H), DEV)
    outs = [torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device=DEV) for _ in range(4)]       # stats, pixel_loss, grad, k
    wsbuf = ws.buf.clone()
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def loss(**over):
        a = dict(image=iv.data_ptr(), f16=1, ps=C, target=tv.data_ptr(), ts=C, C=C, W=W, H=H, w=None, a=None, ma=0.0, kind=0,
                 stats=outs[0].data_ptr(), pl=outs[1].data_ptr(), ws=ptr, wb=ws.capacity())
        a.update(over)
        return L.vp_feature_loss(*a.values(), stream)

    def gradient(**over):
        a = dict(image=iv.data_ptr(), f16=1, ps=C, target=tv.data_ptr(), ts=C, C=C, W=W, H=H, stats=outs[0].data_ptr(), red=1,
                 g=None, grad=outs[2].data_ptr(), gs=C, k=outs[3].data_ptr(), ws=ptr, wb=ws.capacity())
        a.update(over)
        return L.vp_feature_loss_gradient(*a.values(), stream)

    for over in (dict(kind=5), dict(f16=3), dict(C=0), dict(ps=C - 1), dict(ts=C - 1), dict(W=0), dict(H=40000), dict(image=None),
                 dict(target=None), dict(stats=None)):
        assert loss(**over) == -1, over
    for over in (dict(ws=None), dict(ws=ptr + 16), dict(wb=255)):
        assert loss(**over) == -2, over
    for over in (dict(red=7), dict(gs=C - 1), dict(grad=None), dict(k=None), dict(f16=-1), dict(C=5000), dict(stats=None)):
        assert gradient(**over) == -1, over
    for over in (dict(ws=None), dict(ws=ptr + 128), dict(wb=255)):
        assert gradient(**over) == -2, over
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == 0x5A5A5A5A).all()), "a refused call wrote an output"
    assert torch.equal(ws.buf, wsbuf), "a refused call wrote the workspace"


def test_offsets_beyond_2_31_elements():
    """2100 pixels of 8 channels at a pixel stride of 2^20 elements: the last pixel starts 2^31.03 elements in.  Only the C
    elements of every pixel are initialised; the rest of the three 4.4 GB buffers is whatever torch.empty returned."""
    n, C, stride = 2100, 8, 1 << 20
    try:
        bufs = [torch.empty(n * stride, dtype=torch.float16, device=DEV) for _ in range(3)]
    except RuntimeError as e:                                          # pragma: no cover
        pytest.skip(f"three buffers of {n * stride * 2 / 2 ** 30:.1f} GiB do not fit on this GPU: {e}")
    image, target, weight, _ = maps(C, n, 1, True, seed=16)
    views = [torch.as_strided(b, (1, n, C), (n * stride, stride, 1)) for b in bufs]
    views[0].copy_(torch.from_numpy(image).to(DEV))
    views[1].copy_(torch.from_numpy(target).to(DEV))
    views[2].fill_(7.0)
    wt = torch.from_numpy(weight).to(DEV)
    stats, pl, ws = voxproj_host.feature_loss(views[0], views[1], wt, kind="cosine", want_pixel_loss=True)
    Gq, k = voxproj_host.feature_loss_gradient(views[0], views[1], stats, ws, reduction="mean", out=views[2])
    assert Gq.data_ptr() == bufs[2].data_ptr()
    out = dict(stats=stats.cpu().numpy(), pixel_loss=pl.cpu().numpy(), k=int(k), grad=Gq.cpu().numpy())
    r = check(out, image, target, weight=weight, kind="cosine", reduction="mean")
    assert r["valid"].all() and np.abs(out["grad"][0, -1].astype(np.float64)).max() > 0      # the last pixel was reached
