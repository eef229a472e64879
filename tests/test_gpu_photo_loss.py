"""vp_photo_loss and vp_photo_loss_gradient on the GPU, through the C ABI with canaries round every output, against the float64
statement of tests/photo_loss_reference.py.  Every element of m, of the three workspace maps and of the gradient image lies
inside its derived bound, the three statistics inside the summed bounds.

Shapes (photo_loss_reference.gpu_cases): W x H in {1x1, 5x7 (smaller than the window), 11x11, 32x32 and 33x32 (the kernel's
tile and one column more), 37x21, 130x67 (5 x 3 tiles per channel: the ordered combine)}, all at C = 3 with the five input
kinds; C = 1 and 4 at four of the sizes; 530x490 at C = 4 (1088 tile triples, more than the sum stages at a time).  Every test here fails on a library without the three vp_photo_loss symbols."""
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

import photo_loss_reference as pref  # noqa: E402
import voxproj_host  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CANARY = -7.25
LAMBDA = 0.2
WORST = {"m": 0.0, "P": 0.0, "Q": 0.0, "R": 0.0, "grad": 0.0}          # device error / bound, largest so far


def run(x, y, *, lam=LAMBDA, grad_loss=None, ssim_map=True, workspace=True, gradient=True):
    """Both calls through the C ABI on buffers with canaries round every output.  Returns a dict of numpy results."""
    L = voxproj_host.lib()
    C, H, W = x.shape
    n = x.size
    need = voxproj_host.photo_loss_workspace_bytes(C, W, H)
    assert need > 0
    wsbuf = torch.full((need // 4 + 128,), CANARY, dtype=torch.float32, device=DEV)      # 256 spare bytes on either side
    ptr = (wsbuf.data_ptr() + 256 + 255) & ~255
    lead = (ptr - wsbuf.data_ptr()) // 4
    img, tgt = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    stats = torch.full((5,), CANARY, dtype=torch.float64, device=DEV)
    mp = torch.full((n + 2,), CANARY, dtype=torch.float32, device=DEV)
    grad = torch.full((n + 2,), CANARY, dtype=torch.float32, device=DEV)
    g = torch.tensor([grad_loss], dtype=torch.float32, device=DEV) if grad_loss is not None else None
    stream = torch.cuda.current_stream(DEV).cuda_stream
    rc = L.vp_photo_loss(img.data_ptr(), tgt.data_ptr(), C, W, H, stats.data_ptr() + 8, mp.data_ptr() + 4 if ssim_map else None,
                         ptr if workspace else None, need if workspace else 0, stream)
    assert rc == 0, voxproj_host.last_error()
    if gradient:
        assert workspace
        rc = L.vp_photo_loss_gradient(img.data_ptr(), tgt.data_ptr(), C, W, H, lam, voxproj_host._ptr(g), grad.data_ptr() + 4,
                                      ptr, need, stream)
        assert rc == 0, voxproj_host.last_error()
    torch.cuda.synchronize()
    stats_h, m_h, g_h, ws_h = stats.cpu().numpy(), mp.cpu().numpy(), grad.cpu().numpy(), wsbuf.cpu().numpy()
    assert stats_h[0] == CANARY and stats_h[4] == CANARY, "stats' neighbours were written"
    assert m_h[0] == CANARY and m_h[-1] == CANARY, "ssim_map's neighbours were written"
    assert g_h[0] == CANARY and g_h[-1] == CANARY, "the gradient image's neighbours were written"
    assert (ws_h[:lead] == CANARY).all() and (ws_h[lead + need // 4:] == CANARY).all(), "the workspace's neighbours were written"
    if not ssim_map:
        assert (m_h == CANARY).all()
    if not workspace:
        assert (ws_h == CANARY).all()
    if not gradient:
        assert (g_h == CANARY).all()
    maps = ws_h[lead:lead + 3 * n].reshape(3, C, H, W).copy()
    return dict(stats=stats_h[1:4].copy(), m=m_h[1:-1].reshape(C, H, W).copy(), P=maps[0], Q=maps[1], R=maps[2],
                grad=g_h[1:-1].reshape(C, H, W).copy())


_REF = {}


def reference(case, lam=LAMBDA):
    """The inputs, the float64 statement and the bounds of a case, computed once and shared."""
    key = (case, lam)
    if key not in _REF:
        x, y = pref.make_inputs(*case)
        _REF[key] = (x, y, pref.statement64(x, y, lambda_dssim=lam), pref.bounds(x, y, lambda_dssim=lam))
    return _REF[key]


def inside(name, got, want, bound, what):
    err = np.abs(got.astype(np.float64) - want)
    assert np.isfinite(got).all()
    ratio = float((err / np.where(bound > 0, bound, 1.0)).max())
    WORST[name] = max(WORST[name], ratio)
    print(f"{what} {name}: worst error / bound {ratio:.3f} (largest bound {bound.max():.3e}, so far {WORST[name]:.3f})")
    assert (err <= bound).all(), f"{what} {name}: {int((err > bound).sum())} elements outside their bound, worst {ratio:.3f}"


def every_element(case):
    x, y, ref, bnd = reference(case)
    out = run(x, y)
    what = "%s C=%d %dx%d" % case[:4]
    for name in ("m", "P", "Q", "R", "grad"):
        inside(name, out[name], ref[name], bnd[name], what)
    for k in range(3):
        e = abs(out["stats"][k] - ref["stats"][k])
        print(f"{what} stats[{k}]: {out['stats'][k]!r} against {ref['stats'][k]!r}, error {e:.3e} of {bnd['stats'][k]:.3e}")
        assert e <= bnd["stats"][k]
    if case[0] == "binary" and x.size > 100:
        assert out["m"].min() < 0                                       # the kind exists for negative m
    if case[0] == "equal":
        assert out["stats"][0] == 0 and out["stats"][1] == 0
        zero = run(x, y, lam=0.0)["grad"]
        assert not zero.any(), "x = y: the L1 part of the gradient is exactly 0 everywhere"
    return x, y, ref, bnd, out


@pytest.mark.parametrize("case", pref.gpu_cases(), ids=lambda c: "%s-C%d-%dx%d" % c[:4])
def test_every_element_inside_its_bound(case):
    every_element(case)


def test_more_tiles_than_one_staging_of_the_sum():
    """k_photo_loss_sum stages PHOTO_THREADS = 1024 tile triples at a time; there is one triple per 32 x 32 tile and channel:
    a second staging iff C ceil(W / 32) ceil(H / 32) > 1024.  C = 4 at 530 x 490 has 4 x 17 x 16 = 1088 triples (both edges
    ragged: 530 = 16 x 32 + 18, 490 = 15 x 32 + 10); the second staging holds the last 64: channel 3 from tile 4 of tile row
    12 on.  On noise the tile rows 13..15 of that channel alone carry more than ten times the bound of each of the three sums."""
    case = ("noise", 4, 530, 490, 1088)
    assert case[1] * ((case[2] + 31) // 32) * ((case[3] + 31) // 32) == 1088
    x, y, ref, bnd, out = every_element(case)
    d = x[3, 13 * 32:].astype(np.float64) - y[3, 13 * 32:]
    share = np.array([np.abs(d).sum(), np.square(d).sum(), abs(ref["m"][3, 13 * 32:].sum())])
    assert (share > 10 * np.asarray(bnd["stats"])).all(), (share, bnd["stats"])
    del _REF[(case, LAMBDA)]                                            # a million float64 elements per map: not kept
    pref._SUMS.clear()


BIG = ("noise", 3, 130, 67, 160)
ODD = ("smooth", 4, 37, 21, 581)


@pytest.mark.parametrize("case", [BIG, ODD], ids=["130x67", "37x21"])
def test_second_run_and_null_outputs_give_the_same_bits(case):
    x, y, _, _ = reference(case)
    a, b = run(x, y), run(x, y)
    for k in ("stats", "m", "P", "Q", "R", "grad"):
        assert a[k].tobytes() == b[k].tobytes(), f"{k} differs between two runs"
    c = run(x, y, ssim_map=False)                                       # the map's canaries are checked in run()
    assert c["stats"].tobytes() == a["stats"].tobytes() and c["grad"].tobytes() == a["grad"].tobytes()
    d = run(x, y, workspace=False, gradient=False)                      # the workspace's canaries are checked in run()
    assert d["stats"].tobytes() == a["stats"].tobytes(), (d["stats"], a["stats"])
    assert d["m"].tobytes() == a["m"].tobytes()
    e = run(x, y, ssim_map=False, workspace=False, gradient=False)
    assert e["stats"].tobytes() == a["stats"].tobytes()


def test_grad_loss_scales_exactly():
    x, y, _, _ = reference(ODD)
    one, two, zero = run(x, y, grad_loss=1.0)["grad"], run(x, y, grad_loss=2.0)["grad"], run(x, y, grad_loss=0.0)["grad"]
    assert one.tobytes() == run(x, y)["grad"].tobytes()                 # NULL reads as 1
    assert two.tobytes() == (2.0 * one).astype(np.float32).tobytes() and np.abs(one).max() > 0
    assert not zero.any()


@pytest.mark.parametrize("s", [None, -3.0])
def test_lambda_zero_is_the_sign_image(s):
    x, y, _, _ = reference(BIG)
    out = run(x, y, lam=0.0, grad_loss=s)["grad"]
    a = np.float32(1.0 / x.size)                                        # fp32((1 - 0) / n) from float64
    want = (np.float32(1.0 if s is None else s) * (a * np.sign(x - y).astype(np.float32))).astype(np.float32)
    assert np.array_equal(out, want)


def test_lambda_one_has_no_l1_part():
    x, y, ref, _ = reference(BIG)
    out = run(x, y, lam=1.0)["grad"]
    bnd = pref.bounds(x, y, lambda_dssim=1.0)["grad"]                   # a = 0: the bound holds no L1 term either
    want = -(1.0 / x.size) * ref["dm"]
    assert (np.abs(out - want) <= bnd).all()
    assert (bnd < 1e-3 * np.abs(want).max()).all()                      # far below the L1 part's 1 / n: it would show


def test_wrapper_layer_matches_the_abi():
    x, y, _, _ = reference(ODD)
    raw = run(x, y)
    img, tgt = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    stats, mp, ws = voxproj_host.photo_loss(img, tgt, want_ssim_map=True)
    grad = voxproj_host.photo_loss_gradient(img, tgt, ws, lambda_dssim=LAMBDA)
    ev, none_map, none_ws = voxproj_host.photo_loss(img, tgt, evaluate_only=True)
    assert none_map is None and none_ws is None
    assert stats.cpu().numpy().tobytes() == raw["stats"].tobytes() == ev.cpu().numpy().tobytes()
    assert mp.cpu().numpy().tobytes() == raw["m"].tobytes() and grad.cpu().numpy().tobytes() == raw["grad"].tobytes()
    met = voxproj_host.image_metrics(stats, x.size)
    assert abs(met["ssim"] - raw["stats"][2] / x.size) < 1e-15 and met["psnr"] > 0
