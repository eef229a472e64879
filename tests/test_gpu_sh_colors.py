"""vp_sh_colors and vp_sh_colors_backward on the GPU, through the C ABI with canaries round every output, against the float64
statement of tests/sh_reference.py.  Colours, mask and the three gradients of every case lie inside the bounds that module
derives for an fp32 evaluation; no tolerance is picked by hand.

Sizes: N in {1, 63, 64, 65, 257, 4099} (one lane, one wavefront less / exactly / more than one, three workgroups of 128
with a partial last one, 33 workgroups), every Dmax in 0 .. 3 with every active degree d <= Dmax (d == Dmax stages the
contiguous stretch, d < Dmax the row heads).  Inputs: sh_reference.make_inputs.  A channel whose |pre| is below its bound
may be clamped on one side and not on the other: those channels are left out of the mask and gradient comparison, and a
case fails when that is more than 0.1 % of them.  Every test here fails on a library without the two vp_sh symbols."""
import ctypes
import itertools
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

import sh_reference as shref  # noqa: E402
import voxproj_host  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CANARY = -7.25
SIZES = (1, 63, 64, 65, 257, 4099)
DEGREES = [(D, d) for D in range(4) for d in range(D + 1)]
WORST = {"colors": 0.0, "grad_dc": 0.0, "grad_rest": 0.0, "grad_means": 0.0}        # device error / bound, largest so far


def _guarded(n_floats, fill=CANARY):
    """A float32 buffer with four canary floats on either side of n_floats: (buffer, pointer to the payload)."""
    buf = torch.full((n_floats + 8,), CANARY, dtype=torch.float32, device=DEV)
    buf[4:4 + n_floats] = fill
    return buf, buf.data_ptr() + 16


def _payload(buf, shape):
    h = buf.cpu().numpy()
    assert (h[:4] == CANARY).all() and (h[-4:] == CANARY).all(), "an output's neighbours were written"
    return h[4:-4].reshape(shape).copy()


def run(inp, d, *, want=(True, True, True)):
    """Both calls through the C ABI; want = (grad_dc, grad_rest, grad_means).  Returns a dict of numpy results."""
    L = voxproj_host.lib()
    n, kr = inp["f_rest"].shape[:2]
    D = {0: 0, 3: 1, 8: 2, 15: 3}[kr]
    t = {k: torch.from_numpy(np.ascontiguousarray(inp[k])).to(DEV) for k in ("f_dc", "f_rest", "means", "grad_colors")}
    cam = (ctypes.c_float * 3)(*[float(v) for v in inp["campos"]])
    stream = torch.cuda.current_stream(DEV).cuda_stream
    ptr = voxproj_host._ptr
    colors, colors_p = _guarded(3 * n)
    clamped = torch.full((n + 2,), 0xA5, dtype=torch.uint8, device=DEV)
    rc = L.vp_sh_colors(ptr(t["f_dc"]), ptr(t["f_rest"]), ptr(t["means"]), cam, n, d, D, colors_p, clamped.data_ptr() + 1, stream)
    assert rc == 0, voxproj_host.last_error()
    gd, gd_p = _guarded(3 * n)
    gr, gr_p = _guarded(3 * kr * n, fill=float("nan"))
    gm, gm_p = _guarded(3 * n)
    rc = L.vp_sh_colors_backward(None, ptr(t["f_rest"]) if want[2] else None, ptr(t["means"]), cam, n, d, D, ptr(t["grad_colors"]),
                                 clamped.data_ptr() + 1, gd_p if want[0] else None, gr_p if want[1] and kr else None,
                                 gm_p if want[2] else None, stream)
    assert rc == 0, voxproj_host.last_error()
    torch.cuda.synchronize()
    ch = clamped.cpu().numpy()
    assert ch[0] == 0xA5 and ch[-1] == 0xA5, "clamped's neighbours were written"
    out = {"colors": _payload(colors, (n, 3)), "clamped": ch[1:-1].copy(), "clamped_dev": clamped}
    for name, buf, shape, on in (("grad_dc", gd, (n, 3), want[0]), ("grad_rest", gr, (n, kr, 3), want[1]), ("grad_means", gm, (n, 3), want[2])):
        got = _payload(buf, shape)
        if on:
            out[name] = got
        else:
            assert (got == CANARY).all() or np.isnan(got).all(), f"{name} was written although it was not asked for"
    return out


def check(inp, d, got):
    """Every output of ``got`` against the statement, inside the derived bounds."""
    args = (inp["f_dc"], inp["f_rest"], inp["means"], inp["campos"], d)
    f = shref.forward(*args)
    b = shref.backward(*args, inp["grad_colors"])
    bd = shref.bounds(*args, inp["grad_colors"])
    n, kr = inp["f_rest"].shape[:2]
    assert np.isfinite(got["colors"]).all()
    err = np.abs(got["colors"] - f["colors"])
    assert (err <= bd["colors"]).all(), f"colours off by {(err / bd['colors']).max():.2f} bounds"
    WORST["colors"] = max(WORST["colors"], float((err / bd["colors"]).max()))
    near = np.abs(f["pre"]) < bd["pre"]                      # the clamp may fall either way here
    assert near.mean() <= 1e-3, f"{near.sum()} of {near.size} channels lie within their bound of the kink"
    assert np.array_equal(shref.mask_bits(got["clamped"])[~near], shref.mask_bits(f["clamped"])[~near])
    assert (got["clamped"] < 8).all()
    keep_c = ~near
    keep_g = ~near.any(axis=1)
    for name, keep in (("grad_dc", keep_c), ("grad_rest", np.broadcast_to(keep_c[:, None, :], (n, kr, 3))),
                       ("grad_means", np.broadcast_to(keep_g[:, None], (n, 3)))):
        if name not in got:
            continue
        assert np.isfinite(got[name]).all(), f"{name} has a NaN (grad_rest was pre-filled with NaN) or an infinity"
        e = np.abs(got[name] - b[name])[keep]
        lim = bd[name][keep]
        assert (e <= lim).all(), f"{name} off by {(e[lim > 0] / lim[lim > 0]).max() if (lim > 0).any() else np.inf:.2f} bounds"
        if (lim > 0).any():
            WORST[name] = max(WORST[name], float((e[lim > 0] / lim[lim > 0]).max()))
    if "grad_rest" in got:
        tail = got["grad_rest"][:, shref.rest_width(d):]
        assert tail.tobytes() == np.zeros_like(tail).tobytes(), "the inactive tail of grad_rest is not exact zeros"
    if "grad_means" in got and d == 0:
        assert not got["grad_means"].any()


@pytest.mark.parametrize("D,d", DEGREES)
@pytest.mark.parametrize("n", SIZES)
def test_colours_mask_and_gradients_inside_the_derived_bounds(n, D, d):
    inp = shref.make_inputs(n, D, 1000 * n + 10 * D + d)
    got = run(inp, d)
    check(inp, d, got)
    again = run(inp, d)
    for k in ("colors", "clamped", "grad_dc", "grad_rest", "grad_means"):
        assert got[k].tobytes() == again[k].tobytes(), f"{k} differs between two runs"
    print(f"worst error / bound so far: {WORST}")


def test_clamped_share_is_what_the_inputs_promise():
    """3 to 17 % of the channels clamped (measured with the reference's own code by tests/golden/make_sh_golden.py)."""
    for D, d in DEGREES:
        inp = shref.make_inputs(4099, D, 7)
        got = run(inp, d, want=(False, False, False))
        share = shref.mask_bits(got["clamped"]).mean()
        assert 0.03 <= share <= 0.17, (D, d, share)


@pytest.mark.parametrize("D,d", [(3, 3), (3, 1), (2, 2), (0, 0)])
def test_every_null_output_combination(D, d):
    inp = shref.make_inputs(257, D, 50 + d)
    full = run(inp, d)
    for want in itertools.product((False, True), repeat=3):
        part = run(inp, d, want=want)
        for name, on in zip(("grad_dc", "grad_rest", "grad_means"), want):
            if on:
                assert part[name].tobytes() == full[name].tobytes(), (want, name)


@pytest.mark.parametrize("d", [0, 1, 3])
def test_a_mean_at_the_camera_centre_gives_finite_outputs(d):
    inp = shref.make_inputs(130, 3, 77)
    inp["means"][5] = inp["campos"]
    inp["means"][129] = inp["campos"]
    got = run(inp, d)
    check(inp, d, got)
    assert not got["grad_means"][[5, 129]].any()
    want = np.maximum(np.float32(0.5) + np.float32(shref.C0) * inp["f_dc"][5], 0)      # the constant term alone
    assert np.abs(got["colors"][5] - want).max() <= 2.0 ** -23


@pytest.mark.parametrize("D,d", [(3, 3), (3, 2), (1, 1), (2, 2)])
def test_row_offset_views_give_the_values_of_contiguous_copies(D, d):
    """f_rest[1:] starts 12 Kr bytes into its buffer, means[1:] and f_dc[1:] 12 bytes: not 16-byte aligned.  Through the host
    wrappers, outputs included (out_rest is a row-offset view too)."""
    n = 300
    inp = shref.make_inputs(n + 1, D, 9)
    big = {k: torch.from_numpy(inp[k]).to(DEV) for k in ("f_dc", "f_rest", "means", "grad_colors")}
    view = {k: v[1:] for k, v in big.items()}
    copy = {k: v[1:].clone() for k, v in big.items()}
    assert view["means"].data_ptr() % 16 != 0 and copy["f_rest"].data_ptr() % 16 == 0
    assert (view["f_rest"].data_ptr() % 16 != 0) == (D != 2)           # 12 Kr bytes in: 36, 96 (aligned), 180
    vm = torch.eye(4, dtype=torch.float64)
    vm[:3, 3] = -torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64)
    res = {}
    for tag, t in (("view", view), ("copy", copy)):
        colors, clamped = voxproj_host.sh_colors(t["f_dc"], t["f_rest"], t["means"], vm, d)
        out_rest = torch.full((n + 1,) + tuple(t["f_rest"].shape[1:]), float("nan"), device=DEV)[1:] if tag == "view" else None
        grads = voxproj_host.sh_colors_backward(t["f_dc"], t["f_rest"], t["means"], vm, d, t["grad_colors"], clamped, out_rest=out_rest)
        res[tag] = [x.cpu().numpy() for x in (colors, clamped) + grads]
    for a, b in zip(res["view"], res["copy"]):
        assert a.tobytes() == b.tobytes()
    sub = {k: inp[k][1:] for k in ("f_dc", "f_rest", "means", "grad_colors")}
    sub["campos"] = shref.camera_position(vm.numpy())
    check(sub, d, dict(zip(("colors", "clamped", "grad_dc", "grad_rest", "grad_means"), res["view"])))


def test_an_empty_cloud_is_a_valid_call():
    vm = torch.eye(4)
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    colors, clamped = voxproj_host.sh_colors(z(0, 3), z(0, 15, 3), z(0, 3), vm, 3)
    assert tuple(colors.shape) == (0, 3) and tuple(clamped.shape) == (0,)
    grads = voxproj_host.sh_colors_backward(z(0, 3), z(0, 15, 3), z(0, 3), vm, 3, z(0, 3), clamped)
    assert [tuple(g.shape) for g in grads] == [(0, 3), (0, 15, 3), (0, 3)]
    torch.cuda.synchronize()
