"""The prototype-contrastive loss without a GPU: the library's three symbols and their host-side refusals, the workspace size
function, the Python wrappers' argument checks, the float64 reference's closed form against its own autograd, and the
reference against a transcription of the loss's formula on drawn samples.  Everything that touches the library fails on a
tree without vp_proto_contrast."""
import ctypes
import math
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

import proto_loss_reference as pref  # noqa: E402
import voxproj_host  # noqa: E402

SYMBOLS = ("vp_proto_contrast_workspace_bytes", "vp_proto_contrast", "vp_proto_contrast_gradient")
EINVAL, EWORKSPACE = -1, -2                              # VP_EINVAL, VP_EWORKSPACE of include/voxproj.h
NAN, INF = float("nan"), float("inf")


def test_library_exports_the_three_symbols():
    L = voxproj_host.lib()
    hdr = open(os.path.join(ROOT, "include", "voxproj.h")).read()
    for name in SYMBOLS:
        assert name in voxproj_host.EXPORTS and f" {name}(" in hdr
        assert hasattr(L, name), f"libvoxproj.so has no {name}"
    assert L.vp_abi_version() == voxproj_host.VP_ABI_VERSION == 4       # detected by symbol: the version did not move
    assert "#define VP_PROTO_MAX_IDS 256" in hdr and voxproj_host.VP_PROTO_MAX_IDS == pref.MAX_IDS == 256


def test_workspace_size_function():
    size = voxproj_host.proto_contrast_workspace_bytes
    for D, W, H in [(0, 5, 5), (65, 5, 5), (-1, 5, 5), (16, 0, 5), (16, 5, 0), (16, -1, 5), (16, 32769, 1), (16, 1, 32769)]:
        assert size(D, W, H) == 0
    for D in (1, 3, 16, 17, 64):
        last = 0
        for W, H in [(1, 1), (16, 16), (37, 19), (130, 67), (1600, 1067), (32768, 32768)]:
            b = size(D, W, H)
            assert b > 0 and b % 256 == 0 and b >= last
            groups = min((W * H + 255) // 256, 768)
            assert b >= 3 * 256 * D * 4 + groups * 256 * D * 4          # the three tables and the workgroups' partial sums
            last = b
        assert size(D, 1600, 1067) == size(D, 32768, 32768)             # the workgroups are capped: the size stops growing
        assert size(D, 32768, 32768) <= 18 * 1024 + 3 * 1024 * D + 768 * (3 * 1024 + 1024 * D)   # the header's statement
    assert size(64, 130, 67) > size(16, 130, 67)


def _fake_buffers(nbytes):
    buf = ctypes.create_string_buffer(nbytes + 256)
    ws = (ctypes.addressof(buf) + 255) & ~255            # never dereferenced: every call below is refused before a launch
    return buf, ws


def test_loss_call_host_side_refusals_need_no_gpu():
    L = voxproj_host.lib()
    need = voxproj_host.proto_contrast_workspace_bytes(16, 8, 4)
    buf, ws = _fake_buffers(need)
    order = ("image", "D", "W", "H", "ids", "count", "ignore_id", "min_count", "phi_scale", "phi_min", "phi_max", "stats",
             "pixel_loss", "own_prob", "ws", "ws_bytes")

    def call(**over):
        a = dict(image=ws, D=16, W=8, H=4, ids=ws, count=None, ignore_id=-1, min_count=20, phi_scale=10.0, phi_min=0.5,
                 phi_max=1.0, stats=ws, pixel_loss=None, own_prob=None, ws=ws, ws_bytes=need)
        assert set(over) <= set(a), over
        a.update(over)
        return L.vp_proto_contrast(*[a[k] for k in order], None)

    for rc, over in [(EINVAL, dict(image=None)), (EINVAL, dict(ids=None)), (EINVAL, dict(stats=None)), (EINVAL, dict(D=0)),
                     (EINVAL, dict(D=65)), (EINVAL, dict(W=0)), (EINVAL, dict(W=32769)), (EINVAL, dict(H=0)),
                     (EINVAL, dict(H=32769)), (EINVAL, dict(min_count=-1)), (EINVAL, dict(phi_scale=NAN)),
                     (EINVAL, dict(phi_scale=INF)), (EINVAL, dict(phi_min=NAN)), (EINVAL, dict(phi_min=0.0)),
                     (EINVAL, dict(phi_min=-0.5)), (EINVAL, dict(phi_max=NAN)), (EINVAL, dict(phi_max=INF)),
                     (EINVAL, dict(phi_max=0.25)), (EWORKSPACE, dict(ws=None)), (EWORKSPACE, dict(ws=ws + 16)),
                     (EWORKSPACE, dict(ws_bytes=need - 1))]:
        assert call(**over) == rc, over
        assert voxproj_host.last_error()
    assert buf.raw == bytes(len(buf)), "a refused call wrote into its buffers"


def test_gradient_call_host_side_refusals_need_no_gpu():
    L = voxproj_host.lib()
    need = voxproj_host.proto_contrast_workspace_bytes(16, 8, 4)
    buf, ws = _fake_buffers(need)
    order = ("image", "D", "W", "H", "ids", "count", "wc", "wn", "grad_loss", "grad", "ws", "ws_bytes")

    def call(**over):
        a = dict(image=ws, D=16, W=8, H=4, ids=ws, count=None, wc=1.0, wn=1.0, grad_loss=None, grad=ws, ws=ws, ws_bytes=need)
        assert set(over) <= set(a), over
        a.update(over)
        return L.vp_proto_contrast_gradient(*[a[k] for k in order], None)

    for rc, over in [(EINVAL, dict(image=None)), (EINVAL, dict(ids=None)), (EINVAL, dict(grad=None)), (EINVAL, dict(D=0)),
                     (EINVAL, dict(D=65)), (EINVAL, dict(W=0)), (EINVAL, dict(W=32769)), (EINVAL, dict(H=0)),
                     (EINVAL, dict(H=32769)), (EINVAL, dict(wc=NAN)), (EINVAL, dict(wc=INF)), (EINVAL, dict(wn=NAN)),
                     (EINVAL, dict(wn=-INF)), (EWORKSPACE, dict(ws=None)), (EWORKSPACE, dict(ws=ws + 16)),
                     (EWORKSPACE, dict(ws_bytes=need - 1))]:
        assert call(**over) == rc, over
        assert voxproj_host.last_error()
    assert buf.raw == bytes(len(buf)), "a refused call wrote into its buffers"


def test_python_wrappers_check_their_arguments_before_the_gpu():
    img = torch.zeros((4, 3, 5), dtype=torch.float32)
    ids = torch.zeros((3, 5), dtype=torch.int32)
    with pytest.raises(ValueError):
        voxproj_host.proto_contrast(img.double(), ids)
    with pytest.raises(ValueError):
        voxproj_host.proto_contrast(img, ids.long())
    with pytest.raises(ValueError):
        voxproj_host.proto_contrast(img, ids[:2])
    with pytest.raises(ValueError):
        voxproj_host.proto_contrast(torch.zeros((65, 3, 5)), ids)
    with pytest.raises(ValueError):
        voxproj_host.proto_contrast(img, ids, torch.zeros((3, 5)))          # count must be int32
    with pytest.raises(ValueError):
        voxproj_host.proto_contrast_gradient(img, ids, None, None)


def _case(seed, D=5, H=20, W=20, n_ids=7, small=4):
    """400 pixels, 7 ids of which the last has `small` drawn pixels, multiplicities 0-3, ids -1 and 256 sprinkled in."""
    g = np.random.default_rng(seed)
    n = H * W
    ids = g.integers(0, n_ids - 1, n)
    ids[g.choice(n, 12, replace=False)] = np.array([-1, 256] * 6)
    count = g.integers(0, 4, n)
    rare = g.choice(n, small, replace=False)
    ids[rare], count[rare] = n_ids - 1, 1
    protos = g.normal(size=(n_ids + 2, D))
    f = protos[np.clip(ids, -1, n_ids)] * g.uniform(0.5, 1.5, (n, 1)) + 0.6 * g.normal(size=(n, D))
    return (f.T.reshape(D, H, W).astype(np.float32), ids.reshape(H, W).astype(np.int32), count.reshape(H, W).astype(np.int32))


@pytest.mark.parametrize("params", [dict(pref.LOSS_PARAMS, min_count=5), pref.CONFIDENCE_PARAMS], ids=["loss", "confidence"])
@pytest.mark.parametrize("with_count", [True, False])
def test_closed_form_equals_autograd_in_float64(params, with_count):
    image, ids, count = _case(3)
    count = count if with_count else None
    ref = pref.statement64(image, ids, count, ignore_id=2, weight_contrast=0.7, weight_norm=1.3, want_grad=True, **params)
    cf = pref.closed_form(image, ids, count, ignore_id=2, weight_contrast=0.7, weight_norm=1.3, **params)
    assert ref["K"] == cf["K"] and (ref["K"] == 5 if params["min_count"] else ref["K"] == 6)   # id 2 ignored, id 6 by count
    assert np.abs(ref["grad"]).max() > 1e-3
    assert np.abs(ref["grad"] - cf["grad"]).max() <= 1e-13 * np.abs(ref["grad"]).max()
    assert np.abs(ref["l"] - cf["l"]).max() <= 1e-13 and np.abs(ref["own_prob"] - cf["own_prob"]).max() <= 1e-13
    assert np.allclose(ref["stats"], cf["stats"], rtol=1e-13, atol=0)
    # what is not a valid sample: exact zeros
    inval = ~ref["valid"]
    assert inval.any() and not ref["pixel_loss"][inval].any() and not ref["own_prob"][inval].any()
    assert ref["stats"][3] == ref["m"].sum()


def _formula(samples, labels, min_pixnum, scale, lo, hi):
    """The loss's formula on drawn samples [B,D] with labels [B]: clusters with more than min_pixnum samples, their means
    and concentrations, the softmax of every sample of a cluster against every cluster, summed and divided by the number
    of clusters; and the regulariser is not part of it."""
    x = samples / (np.linalg.norm(samples, axis=-1, keepdims=True) + 1e-6)
    cids, cnums = np.unique(labels, return_counts=True)
    cids, cnums = cids[cnums > min_pixnum], cnums[cnums > min_pixnum]
    means, phis = [], []
    for cid, cn in zip(cids, cnums):
        cl = x[labels == cid]
        mu = cl.mean(0)
        means.append(mu)
        phis.append(np.linalg.norm(cl - mu, axis=1).sum() / (cn * math.log(cn + 10)))
    phis = np.clip(np.array(phis) * scale, lo, hi)
    total = 0.0
    for i, cid in enumerate(cids):
        cl = x[labels == cid]
        logits = np.stack([(cl * mu).sum(1) / ph for mu, ph in zip(means, phis)], 1)
        total += (-np.log(np.exp(logits[:, i]) / (np.exp(logits).sum(1) + 1e-6))).sum()
    return total / len(cids), len(cids)


def test_reference_equals_the_formula_on_drawn_samples():
    """Pixels drawn with replacement: the multiplicity map against the samples written out one by one.  The formula has
    -log(e^z_c / (sum + 1e-6)), the contract log(sum + 1e-6) - z_c: the same number."""
    image, ids, _ = _case(11, n_ids=6, small=3)
    D, H, W = image.shape
    g = np.random.default_rng(5)
    ids = np.clip(ids, 0, 255)                                           # the formula knows no excluded ids
    draw = g.integers(0, H * W, 900)
    count = np.bincount(draw, minlength=H * W).reshape(H, W).astype(np.int32)
    samples = image.reshape(D, -1).T.astype(np.float64)[draw]
    labels = ids.reshape(-1)[draw]
    for params in (dict(pref.LOSS_PARAMS, min_count=8), pref.CONFIDENCE_PARAMS):
        want, K = _formula(samples, labels, params["min_count"], params["phi_scale"], params["phi_min"], params["phi_max"])
        ref = pref.statement64(image, ids, count, **params)
        assert ref["K"] == K and K >= 5
        assert abs(ref["stats"][0] / K - want) <= 1e-12 * abs(want)
        assert ref["stats"][3] == sum(int((labels == k).sum()) for k in ref["active"])


def test_float32_yardstick_is_small_and_positive():
    image, ids, count = _case(3)
    params = dict(pref.LOSS_PARAMS, min_count=5)
    b = pref.bounds(image, ids, count, params)
    assert 0 < b["E_z"] < 1e-4 and 0 < b["E_s"] < 1e-4
    assert b["dLds"] == 8 * b["E_s"]                                     # a non-zero yardstick is not raised by any floor
    ref = pref.statement64(image, ids, count, want_grad=True, **params)
    assert pref.norm_bound(ref) < 1e-3 * ref["stats"][2]
    assert pref.gradient_bound(ref, b).shape == image.shape
    assert (b["pixel_loss"][ref["valid"]] > 0).all() and (b["pixel_loss"] < 1e-3).all() and (b["own_prob"] < 1e-4).all()
