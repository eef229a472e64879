"""vp_proto_contrast and vp_proto_contrast_gradient on the GPU against the float64 statement of
tests/proto_loss_reference.py, on random images: no Gaussians are involved.  The bounds are that file's; every pixel and every
element is checked, because these inputs contain no fragile decision.

Shapes.  D in {1, 3, 16, 17, 64}: one channel, a partly filled block of 16, a full one, one channel into a second block (the
32-register variant), the limit.  W x H in {1x1, 37x19, 130x67}: one pixel, three workgroups with a tail, 35 workgroups (the
ordered combine).  One more size, 1024x200 at D = 3 with three ids, has 800 tiles for the 768 workgroups: the only size at
which a workgroup walks more than one tile.

Id layouts: one id (K = 1, loss about 0), two, 37, all 256 (130x67 only: elsewhere there are not enough pixels), and "edge":
ids -1, 256 and the ignored id, an id with exactly min_count drawn pixels (dropped) and one with min_count + 1 (kept), one id
confined to the first tile and one with a pixel in every tile.  Count maps: NULL, all zero (K = 0), mixed 0-3.  One pixel with
f = 0 (not at 1x1, whose only pixel has a non-zero row).  Both of the reference's parameter sets.

Every test here fails on a library without the three vp_proto_contrast symbols."""
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

import proto_loss_reference as pref  # noqa: E402
import voxproj_host  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CANARY = -7.25
IGNORE = 7
PARAMS = {"loss": pref.LOSS_PARAMS, "confidence": pref.CONFIDENCE_PARAMS}
WORST = {"pixel_loss": 0.0, "own_prob": 0.0, "gradient": 0.0}      # device error / bound, largest so far


def make_case(D, W, H, layout, count_kind, min_count, seed):
    """(image f32 [D,H,W], ids i32 [H,W], count i32 [H,W] or None): rows scattered round one direction per id."""
    g = np.random.default_rng(seed)
    n = W * H
    tiles = (n + 255) // 256
    if layout == "one":
        ids = np.full(n, 5)
    elif layout == "two":
        ids = (np.arange(n) * 2 // max(n, 1)) * 200                    # ids 0 and 200
    elif layout == "37":
        ids = 3 + 6 * g.integers(0, 37, n)
    elif layout == "256":
        ids = g.permutation(np.arange(n) % 256)
    else:
        assert layout == "edge"
        ids = 10 + g.integers(0, 5, n)
    count = None if count_kind == "null" else np.zeros(n, np.int64) if count_kind == "zero" else g.integers(0, 4, n)
    if layout == "edge" and n >= 256:
        perm = g.permutation(n)
        every = np.array([perm[perm // 256 == t][0] for t in range(tiles)], np.int64)     # one pixel in every tile
        rest = perm[~np.isin(perm, every)]
        first = rest[rest < 256][:30]                                   # confined to the first tile
        rest = list(rest[~np.isin(rest, first)])

        def take(k):
            return np.array([rest.pop() for _ in range(k)], np.int64)
        ids[take(9)] = np.array([-1, 256, IGNORE] * 3)
        ids[take(3)] = np.array([-2 ** 31, 2 ** 31 - 1, 300])
        for the_id, k in ((40, min_count), (41, min_count + 1)):       # dropped by one, kept by one
            sel = take(k)
            ids[sel] = the_id
            if count is not None and count_kind != "zero":
                count[sel] = 1
        ids[first] = 42
        ids[every] = 43
        if count is not None and count_kind != "zero":
            count[first] = 2
            count[every] = 3 + 7 * (tiles < 8)                          # more than min_count drawn in all, few tiles or many
    dirs = g.normal(size=(258, D))
    f = dirs[np.clip(ids, -1, 256) + 1] * g.uniform(0.5, 1.6, (n, 1)) + 0.5 * g.normal(size=(n, D))
    if n > 1:
        f[n // 2] = 0.0                                                 # the pixel with f = 0
    image = np.ascontiguousarray(f.T.reshape(D, H, W)).astype(np.float32)
    return image, ids.reshape(H, W).astype(np.int32), None if count is None else count.reshape(H, W).astype(np.int32)


def run(image, ids, count, params, ignore_id=IGNORE, weights=(1.0, 1.0), grad_loss=None, outputs=True):
    """Both calls through the C ABI on buffers with canaries round every output.  Returns a dict of numpy results."""
    L = voxproj_host.lib()
    D, H, W = image.shape
    n = H * W
    ws = voxproj_host.SplatWorkspace()
    ptr = ws.ensure(voxproj_host.proto_contrast_workspace_bytes(D, W, H), DEV)
    img = torch.from_numpy(image).to(DEV)
    idt = torch.from_numpy(ids).to(DEV)
    cnt = torch.from_numpy(count).to(DEV) if count is not None else None
    stats = torch.full((6,), CANARY, dtype=torch.float64, device=DEV)
    pl = torch.full((n + 2,), CANARY, dtype=torch.float32, device=DEV)
    op = torch.full((n + 2,), CANARY, dtype=torch.float32, device=DEV)
    grad = torch.full((D * n + 2,), CANARY, dtype=torch.float32, device=DEV)
    g = torch.tensor([grad_loss], dtype=torch.float32, device=DEV) if grad_loss is not None else None
    stream = torch.cuda.current_stream(DEV).cuda_stream
    rc = L.vp_proto_contrast(img.data_ptr(), D, W, H, idt.data_ptr(), voxproj_host._ptr(cnt), ignore_id, params["min_count"],
                             params["phi_scale"], params["phi_min"], params["phi_max"], stats.data_ptr() + 8,
                             pl.data_ptr() + 4 if outputs else None, op.data_ptr() + 4 if outputs else None, ptr, ws.capacity(),
                             stream)
    assert rc == 0, voxproj_host.last_error()
    rc = L.vp_proto_contrast_gradient(img.data_ptr(), D, W, H, idt.data_ptr(), voxproj_host._ptr(cnt), weights[0], weights[1],
                                      voxproj_host._ptr(g), grad.data_ptr() + 4, ptr, ws.capacity(), stream)
    assert rc == 0, voxproj_host.last_error()
    torch.cuda.synchronize()
    stats_h, pl_h, op_h, g_h = stats.cpu().numpy(), pl.cpu().numpy(), op.cpu().numpy(), grad.cpu().numpy()
    assert stats_h[0] == CANARY and stats_h[5] == CANARY, "stats' neighbours were written"
    assert pl_h[0] == CANARY and pl_h[-1] == CANARY, "pixel_loss' neighbours were written"
    assert op_h[0] == CANARY and op_h[-1] == CANARY, "own_prob's neighbours were written"
    assert g_h[0] == CANARY and g_h[-1] == CANARY, "the gradient image's neighbours were written"
    if not outputs:
        assert (pl_h == CANARY).all() and (op_h == CANARY).all()
    return dict(stats=stats_h[1:5].copy(), pixel_loss=pl_h[1:-1].copy(), own_prob=op_h[1:-1].copy(),
                grad=g_h[1:-1].reshape(D, H, W).copy())


def check(out, image, ids, count, params, ignore_id=IGNORE, weights=(1.0, 1.0), grad_loss=None):
    """Every check of the contract on one result of run().  Returns the float64 reference."""
    gl = 1.0 if grad_loss is None else float(np.float32(grad_loss))
    ref = pref.statement64(image, ids, count, ignore_id=ignore_id, weight_contrast=weights[0], weight_norm=weights[1],
                           want_grad=True, **params)
    bnd = pref.bounds(image, ids, count, dict(params, ignore_id=ignore_id), weights)
    valid = ref["valid"]
    # statistics: K and sum m exactly, the norm within its derived bound, the loss within the pixels' bounds
    print(f"stats {out['stats']} against {ref['stats']}")
    assert out["stats"][1] == ref["stats"][1] and out["stats"][3] == ref["stats"][3]
    e2, b2 = abs(out["stats"][2] - ref["stats"][2]), pref.norm_bound(ref)
    print(f"norm statistic: error {e2:.3e} of {b2:.3e}")
    assert e2 <= b2
    e0 = abs(out["stats"][0] - ref["stats"][0])
    print(f"loss statistic: error {e0:.3e} of {bnd['stats0']:.3e}")
    assert e0 <= bnd["stats0"]
    # per-pixel outputs: exact zeros where the pixel is not a valid sample
    assert np.isfinite(out["pixel_loss"]).all() and np.isfinite(out["own_prob"]).all()
    assert not out["pixel_loss"][~valid].any() and not out["own_prob"][~valid].any()
    el = np.abs(out["pixel_loss"].astype(np.float64) - ref["pixel_loss"])
    ep = np.abs(out["own_prob"].astype(np.float64) - ref["own_prob"])
    if valid.any():
        WORST["pixel_loss"] = max(WORST["pixel_loss"], float((el[valid] / bnd["pixel_loss"][valid]).max()))
        WORST["own_prob"] = max(WORST["own_prob"], float((ep[valid] / bnd["own_prob"][valid]).max()))
    assert (el <= bnd["pixel_loss"]).all() and (ep <= bnd["own_prob"]).all(), WORST
    # the gradient image: every element
    G = gl * ref["grad"]
    gb = pref.gradient_bound(ref, bnd, gl)
    eg = np.abs(out["grad"].astype(np.float64) - G)
    assert np.isfinite(out["grad"]).all()
    worst = float((eg / np.maximum(gb, 1e-300)).max())
    WORST["gradient"] = max(WORST["gradient"], worst)
    print(f"gradient: worst {worst:.3f} of the bound, largest |G| {np.abs(G).max():.3e}; worst so far, of the bounds: {WORST}")
    assert (eg <= gb).all(), f"gradient off by {worst:.3f} of the bound"
    return ref


@pytest.mark.parametrize("size", [(1, 1), (37, 19), (130, 67)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("D", [1, 3, 16, 17, 64])
def test_against_float64_over_shapes(D, size):
    W, H = size
    seed = D * 1000 + W
    for which, layout, count_kind in (("loss", "edge", "mixed"), ("confidence", "37", "null")):
        print(f"--- D = {D}, {W} x {H}, {which}, {layout}, count {count_kind}")
        params = PARAMS[which]
        image, ids, count = make_case(D, W, H, layout, count_kind, params["min_count"], seed)
        ref = check(run(image, ids, count, params), image, ids, count, params)
        if layout == "edge" and W * H >= 256:
            assert 40 not in ref["active"] and 41 in ref["active"] and 42 in ref["active"] and 43 in ref["active"]
            assert IGNORE not in ref["active"]


@pytest.mark.parametrize("which", ["loss", "confidence"])
@pytest.mark.parametrize("count_kind", ["null", "zero", "mixed"])
@pytest.mark.parametrize("layout", ["one", "two", "37", "edge"])
def test_layouts_counts_and_parameters(layout, count_kind, which):
    params = PARAMS[which]
    image, ids, count = make_case(16, 37, 19, layout, count_kind, params["min_count"], 77)
    out = run(image, ids, count, params)
    ref = check(out, image, ids, count, params)
    if count_kind == "zero":
        assert ref["K"] == 0 and out["stats"][0] == 0.0 and out["stats"][1] == 0.0 and out["stats"][3] == 0.0
        only_norm = run(image, ids, count, params, weights=(1.0, 0.0))
        assert not only_norm["grad"].any(), "K = 0: the contrastive part must be exactly 0"
    elif layout == "one":
        assert ref["K"] == 1 and abs(out["stats"][0]) <= 1e-3 * ref["stats"][3]   # log(e^z + 1e-6) - z: about 1e-6 e^-z a sample
    elif layout == "two":
        assert ref["K"] == 2 and ref["active"] == [0, 200]


@pytest.mark.parametrize("which", ["loss", "confidence"])
@pytest.mark.parametrize("count_kind", ["null", "mixed"])
def test_all_256_ids(count_kind, which):
    params = PARAMS[which]
    image, ids, count = make_case(16, 130, 67, "256", count_kind, params["min_count"], 5)
    ref = check(run(image, ids, count, params, ignore_id=-1), image, ids, count, params, ignore_id=-1)
    assert ref["K"] == 256


def test_more_tiles_than_workgroups():
    """1024 x 200 = 800 tiles on 768 workgroups: the first 32 workgroups walk two tiles each."""
    params = pref.LOSS_PARAMS
    g = np.random.default_rng(9)
    W, H, D = 1024, 200, 3
    ids = g.integers(0, 3, (H, W)).astype(np.int32) * 100
    count = g.integers(0, 3, (H, W)).astype(np.int32)
    dirs = g.normal(size=(3, D))
    image = (dirs[ids // 100] + 0.4 * g.normal(size=(H, W, D))).transpose(2, 0, 1).astype(np.float32).copy()
    ref = check(run(image, ids, count, params), image, ids, count, params)
    assert ref["K"] == 3


def test_second_run_is_bit_identical_and_outputs_are_optional():
    params = pref.LOSS_PARAMS
    image, ids, count = make_case(17, 130, 67, "edge", "mixed", params["min_count"], 21)
    a = run(image, ids, count, params, weights=(0.7, 1.3), grad_loss=-2.5)
    b = run(image, ids, count, params, weights=(0.7, 1.3), grad_loss=-2.5)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), f"{key} differs between two runs"
    c = run(image, ids, count, params, weights=(0.7, 1.3), grad_loss=-2.5, outputs=False)
    assert c["stats"].tobytes() == a["stats"].tobytes() and c["grad"].tobytes() == a["grad"].tobytes()


def test_grad_loss_and_weights_scale_as_stated():
    params = pref.LOSS_PARAMS
    image, ids, count = make_case(16, 37, 19, "37", "mixed", params["min_count"], 33)
    check(run(image, ids, count, params, weights=(0.7, 1.3), grad_loss=-2.5), image, ids, count, params, weights=(0.7, 1.3),
          grad_loss=-2.5)
    contrast = check(run(image, ids, count, params, weights=(2.0, 0.0)), image, ids, count, params, weights=(2.0, 0.0))
    norm = check(run(image, ids, count, params, weights=(0.0, 3.0)), image, ids, count, params, weights=(0.0, 3.0))
    assert np.abs(contrast["grad"]).max() > 0 and np.abs(norm["grad"]).max() > 0
    # grad_loss = 2 and weights doubled are powers of two: the same bits
    one = run(image, ids, count, params, weights=(1.0, 0.5))
    two = run(image, ids, count, params, weights=(1.0, 0.5), grad_loss=2.0)
    dbl = run(image, ids, count, params, weights=(2.0, 1.0))
    assert (2.0 * one["grad"]).tobytes() == two["grad"].tobytes() == dbl["grad"].tobytes()
    zero = run(image, ids, count, params, grad_loss=0.0)
    assert not zero["grad"].any()
