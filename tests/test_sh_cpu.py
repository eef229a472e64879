"""CPU-side checks of the view-dependent colour (include/voxproj_ext.h): the float64 twin of tests/sh_reference.py against
results recorded from the reference's own eval_sh, its adjoints against central differences, the ply columns, the degree
schedule of the fitting CLI, the host wrappers' refusals and the second signature table against its header.  No device call
is made here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import sh_reference as shref
from test_abi_cpu import _binding_error          # the comparison of a ctypes binding with a C prototype, written once

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sh_golden.npz")
NAMES = ("f_dc", "f_rest", "means", "campos", "grad_colors")


def _case(g, d):
    return {k: g[f"{k}_{d}"] for k in NAMES}


@pytest.mark.parametrize("d", [0, 1, 2, 3])
def test_twin_matches_the_reference_at_float64_rounding(d):
    """The recorded colours and gradients come from utils/sh_utils.eval_sh + clamp_min under autograd in float64.  Both sides
    add at most 16 products of magnitude below max |sh| * max |Y| each: 64 roundings of the largest result bound the gap."""
    g = np.load(GOLDEN)
    inp = _case(g, d)
    args = (inp["f_dc"], inp["f_rest"], inp["means"], inp["campos"], d)
    f = shref.forward(*args)
    b = shref.backward(*args, inp["grad_colors"])
    grad_sh = np.concatenate([b["grad_dc"][:, None], b["grad_rest"]], axis=1)
    for got, want in ((f["colors"], g[f"colors_{d}"]), (grad_sh, g[f"grad_sh_{d}"]), (b["grad_means"], g[f"grad_means_{d}"])):
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 64 * 2.0 ** -53 * max(1.0, np.abs(want).max())
    # the reference leaves the coefficients beyond the active degree without gradient: exact zeros here
    assert not grad_sh[:, shref.n_coeffs(d):].any() and not g[f"grad_sh_{d}"][:, shref.n_coeffs(d):].any()
    assert 0.02 < shref.mask_bits(f["clamped"]).mean() < 0.25          # the clamp is exercised


@pytest.mark.parametrize("d", [1, 2, 3])
def test_twin_adjoints_match_central_differences(d):
    """sum(colour * upstream) differentiated numerically, step 1e-6 in float64 (truncation ~ h^2 |f'''| ~ 1e-10, rounding
    ~ 1e-16 / h = 1e-10), on the Gaussians none of whose channels lies within 1e-3 of the kink."""
    inp = shref.make_inputs(24, 3, 40 + d)
    a = {k: inp[k].astype(np.float64) for k in NAMES}
    f = shref.forward(a["f_dc"], a["f_rest"], a["means"], a["campos"], d)
    away = (np.abs(f["pre"]) > 1e-3).all(axis=1)
    assert away.sum() >= 20
    b = shref.backward(a["f_dc"], a["f_rest"], a["means"], a["campos"], d, a["grad_colors"])

    def loss(**kw):
        v = dict(a, **kw)
        return (shref.forward(v["f_dc"], v["f_rest"], v["means"], v["campos"], d)["colors"] * a["grad_colors"]).sum(axis=1)

    h = 1e-6
    for name, grad in (("f_dc", b["grad_dc"]), ("f_rest", b["grad_rest"]), ("means", b["grad_means"])):
        flat = grad.reshape(grad.shape[0], -1)
        for j in range(flat.shape[1]):
            e = np.zeros_like(flat)
            e[:, j] = h
            e = e.reshape(grad.shape)
            num = (loss(**{name: a[name] + e}) - loss(**{name: a[name] - e})) / (2 * h)
            assert np.abs(num - flat[:, j])[away].max() <= 2e-8 * max(1.0, np.abs(flat).max()), (name, j)


def test_derived_bounds_are_fp32_sized_and_grow_with_the_degree():
    inp = shref.make_inputs(257, 3, 5)
    prev = 0.0
    for d in range(4):
        bd = shref.bounds(inp["f_dc"], inp["f_rest"], inp["means"], inp["campos"], d, inp["grad_colors"])
        assert set(bd) == {"pre", "colors", "grad_dc", "grad_rest", "grad_means"}
        assert 1e-8 < bd["pre"].max() < 1e-4 and bd["pre"].max() > prev
        prev = bd["pre"].max()
        assert not bd["grad_rest"][:, shref.rest_width(d):].any()       # exact zeros carry no error
        assert (bd["grad_means"] == 0).all() if d == 0 else bd["grad_means"].max() < 1e-3
    # a mean at the camera centre: direction 0 exactly, finite bounds, no gradient to the mean
    inp["means"][3] = inp["campos"]
    f = shref.forward(inp["f_dc"], inp["f_rest"], inp["means"], inp["campos"], 3)
    b = shref.backward(inp["f_dc"], inp["f_rest"], inp["means"], inp["campos"], 3, inp["grad_colors"])
    bd = shref.bounds(inp["f_dc"], inp["f_rest"], inp["means"], inp["campos"], 3, inp["grad_colors"])
    assert np.isfinite(f["colors"]).all() and not b["grad_means"][3].any() and not bd["grad_means"][3].any()
    assert np.allclose(f["pre"][3], 0.5 + shref.C0 * inp["f_dc"][3].astype(np.float64))


def _cloud(n, seed=3):
    rng = np.random.default_rng(seed)
    return dict(means=rng.normal(size=(n, 3)).astype(np.float32), opacity_logits=rng.normal(size=n).astype(np.float32),
                log_scales=rng.normal(size=(n, 3)).astype(np.float32), rots=rng.normal(size=(n, 4)).astype(np.float32),
                f_dc=rng.normal(size=(n, 3)).astype(np.float32))


@pytest.mark.parametrize("D", [1, 2, 3])
def test_ply_round_trip_with_channel_major_columns(tmp_path, D):
    import gaussian_ply
    n, kr = 7, (D + 1) ** 2 - 1
    c = _cloud(n)
    f_rest = np.random.default_rng(D).normal(size=(n, kr, 3)).astype(np.float32)
    path = str(tmp_path / "sh.ply")
    gaussian_ply.write_gaussian_ply(path, c["means"], c["opacity_logits"], c["log_scales"], c["rots"], f_dc=c["f_dc"], f_rest=f_rest)
    back = gaussian_ply.read_gaussian_ply(path, want_dc=True, want_raw=True, want_sh=True)
    assert back["f_rest"].dtype == np.float32 and back["f_rest"].tobytes() == f_rest.tobytes()
    assert back["f_dc"].tobytes() == c["f_dc"].tobytes() and back["rots"].tobytes() == c["rots"].tobytes()
    # the file itself: f_rest_* between f_dc_* and opacity, column i = channel i // Kr, coefficient i % Kr
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    props = re.findall(rb"property float (\S+)", head)
    assert props[6:9] == [b"f_dc_0", b"f_dc_1", b"f_dc_2"] and props[9 + 3 * kr] == b"opacity" and len(props) == 17 + 3 * kr
    assert props[9:9 + 3 * kr] == [b"f_rest_%d" % i for i in range(3 * kr)]
    rec = np.frombuffer(body, "<f4").reshape(n, len(props))
    for i in range(3 * kr):
        assert np.array_equal(rec[:, 9 + i], f_rest[:, i % kr, i // kr]), i
    # without want_sh the columns are skipped as before
    assert "f_rest" not in gaussian_ply.read_gaussian_ply(path, want_dc=True)


def test_ply_without_f_rest_is_the_17_field_file_byte_for_byte(tmp_path):
    import gaussian_ply
    n = 5
    c = _cloud(n)
    path = str(tmp_path / "plain.ply")
    gaussian_ply.write_gaussian_ply(path, c["means"], c["opacity_logits"], c["log_scales"], c["rots"], f_dc=c["f_dc"])
    fields = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2", "rot_0",
              "rot_1", "rot_2", "rot_3"]
    rows = np.concatenate([c["means"], np.zeros((n, 3), np.float32), c["f_dc"], c["opacity_logits"][:, None], c["log_scales"],
                           c["rots"]], axis=1).astype("<f4")
    want = (b"ply\nformat binary_little_endian 1.0\n" + b"element vertex %d\n" % n +
            b"".join(b"property float %s\n" % k.encode() for k in fields) + b"end_header\n" + rows.tobytes())
    assert open(path, "rb").read() == want
    back = gaussian_ply.read_gaussian_ply(path, want_sh=True)
    assert back["f_rest"].shape == (n, 0, 3) and back["f_rest"].dtype == np.float32


def test_ply_refuses_a_column_count_that_is_no_degree(tmp_path):
    import gaussian_ply
    n = 3
    c = _cloud(n)
    with pytest.raises(ValueError, match=r"f_rest must be"):
        gaussian_ply.write_gaussian_ply(str(tmp_path / "bad.ply"), c["means"], c["opacity_logits"], c["log_scales"], c["rots"],
                                        f_rest=np.zeros((n, 5, 3), np.float32))
    # a file with 12 f_rest_* columns (Kr = 4 is no (D + 1)^2 - 1), written by hand
    fields = ["x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{i}" for i in range(12)] + \
             ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    path = str(tmp_path / "twelve.ply")
    with open(path, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n)
        f.write(b"".join(b"property float %s\n" % k.encode() for k in fields) + b"end_header\n")
        f.write(np.zeros((n, len(fields)), "<f4").tobytes())
    assert gaussian_ply.read_gaussian_ply(path)["means"].shape == (n, 3)       # still readable without the coefficients
    with pytest.raises(ValueError, match=r"12 f_rest_\* columns"):
        gaussian_ply.read_gaussian_ply(path, want_sh=True)


def test_fitting_cli_has_the_sh_options_beside_the_recorded_ones():
    """build_parser() is the option set tests/golden/cli_parsers.json records (test_gaussian_views_cpu.py holds it to that);
    the command line main() parses, build_cli(), is that set and the three SH options, inert at their defaults."""
    import fit_gaussian_appearance as fga
    opts = lambda ap: {a.option_strings[0]: a for a in ap._actions if a.option_strings}  # noqa: E731
    old, new = opts(fga.build_parser()), opts(fga.build_cli())
    assert set(new) - set(old) == {"--sh_degree", "--sh_degree_interval", "--lr_sh_rest"} and set(old) <= set(new)
    assert [(new[k].default, new[k].type) for k in ("--sh_degree", "--sh_degree_interval", "--lr_sh_rest")] == \
        [(0, int), (1000, int), (None, float)]
    base = ["--gaussians_ply", "p", "--cam_params", "c", "--images_dir", "d", "--out", "o"]
    a = fga.build_cli().parse_args(base)
    assert vars(fga.build_parser().parse_args(base)).items() <= vars(a).items()
    assert (a.sh_degree, a.sh_degree_interval, a.lr_sh_rest) == (0, 1000, None)
    a = fga.build_cli().parse_args(base + ["--sh_degree", "2", "--sh_degree_interval", "5", "--lr_sh_rest", "0.001"])
    assert (a.sh_degree, a.sh_degree_interval, a.lr_sh_rest) == (2, 5, 0.001)


def test_active_sh_degree_schedule():
    from fit_gaussian_appearance import active_sh_degree
    assert [active_sh_degree(s, 3, 1000) for s in (0, 1, 999, 1000, 1999, 2000, 2999, 3000, 30000)] == [0, 0, 0, 1, 1, 2, 2, 3, 3]
    assert [active_sh_degree(s, 2, 5) for s in range(0, 16, 5)] == [0, 1, 2, 2]
    assert active_sh_degree(10 ** 9, 0, 1) == 0
    assert [active_sh_degree(s, 3, 1000, start=3) for s in (0, 5000)] == [3, 3]       # a cloud that brought its coefficients
    assert active_sh_degree(1000, 3, 1000, start=1) == 2
    for bad in ((-1, 3, 1000), (0, 3, 0), (0, -1, 5)):
        with pytest.raises(ValueError):
            active_sh_degree(*bad)
    with pytest.raises(ValueError):
        active_sh_degree(0, 2, 5, start=3)


def test_host_wrappers_refuse_cpu_tensors_and_bad_shapes_before_any_device_call(monkeypatch):
    import splat_autograd
    import voxproj_host

    def no_call(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(voxproj_host, "_call", no_call)
    n = 4
    dc, rest, means = torch.zeros(n, 3), torch.zeros(n, 15, 3), torch.zeros(n, 3)
    vm = torch.eye(4)
    for fn in (lambda *a: voxproj_host.sh_colors(*a), lambda *a: splat_autograd.sh_colors(*a),
               lambda *a: voxproj_host.sh_colors_backward(*a, torch.zeros(n, 3), torch.zeros(n, dtype=torch.uint8))):
        with pytest.raises(ValueError, match="f_dc must be a CUDA tensor: there is no CPU path"):
            fn(dc, rest, means, vm, 3)
        with pytest.raises(ValueError, match="f_rest must be torch.float32"):
            fn(dc, rest.double(), means, vm, 3)
    # shapes and degrees are judged before the device too: meta tensors claim to be CUDA-less, so fake the flag
    monkeypatch.setattr(voxproj_host, "_require_tensors", lambda *specs: None)
    cases = [((dc, torch.zeros(n, 5, 3), means, vm, 1), r"5 coefficient rows"), ((dc, rest, torch.zeros(n + 1, 3), vm, 1), r"means must be"),
             ((torch.zeros(n, 4), rest, means, vm, 1), r"f_dc must be \[N, 3\]"), ((dc, rest, means, vm, 4), r"degree = 4 outside \[0, 3\]"),
             ((dc, torch.zeros(n, 3, 3), means, vm, 2), r"degree = 2 outside \[0, 1\]"), ((dc, rest, means, vm, -1), r"degree = -1"),
             ((dc, torch.zeros(n, 15, 2), means, vm, 1), r"f_rest must be"), ((dc, rest, means, torch.zeros(3, 4), 1), r"viewmat must be")]
    for args, msg in cases:
        with pytest.raises(ValueError, match=msg):
            voxproj_host.sh_colors(*args)
    with pytest.raises(ValueError, match=r"grad_colors must be \[4, 3\]"):
        voxproj_host.sh_colors_backward(dc, rest, means, vm, 1, torch.zeros(n, 2), torch.zeros(n, dtype=torch.uint8))
    with pytest.raises(ValueError, match="viewmat requires grad"):
        splat_autograd.sh_colors(dc, rest, means, torch.eye(4, requires_grad=True), 1)


def test_camera_position_is_minus_rt_t_in_float64():
    import voxproj_host
    rng = np.random.default_rng(0)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    c = np.array([0.3, -0.2, 0.1])
    vm = np.eye(4)
    vm[:3, :3], vm[:3, 3] = q, -q @ c
    got = voxproj_host.camera_position(torch.from_numpy(vm))
    assert np.abs(np.array(got) - c).max() < 1e-15
    assert np.array_equal(shref.camera_position(vm), np.array(got, np.float32).astype(np.float64))


# ---- the second signature table against include/voxproj_ext.h ----
def _ext_prototypes():
    """{name: (return type, [parameter type, ...])} of every vp_* prototype of include/voxproj_ext.h, ``const`` and
    parameter names dropped; a pointer type ends in `` *``."""
    txt = open(os.path.join(ROOT, "include", "voxproj_ext.h")).read()
    txt = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))

    def ctype(decl, named):
        words = [w for w in decl.replace("*", " ").split() if w != "const"]
        return " ".join(words[:-1] if named else words) + (" *" if "*" in decl else "")

    return {name: (ctype(ret, False), [ctype(q, True) for q in params.split(",")])
            for ret, name, params in re.findall(r"([A-Za-z_][\w \t]*?[\s\*]+)(vp_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", txt)}


def test_ext_header_matches_the_second_signature_table():
    import voxproj_host
    voxproj_host.build()
    protos = _ext_prototypes()
    assert sorted(protos) == sorted(voxproj_host.EXPORTS_EXT) == ["vp_sh_colors", "vp_sh_colors_backward"]
    assert len(voxproj_host.EXPORTS) == 64 and not set(voxproj_host.EXPORTS) & set(voxproj_host.EXPORTS_EXT)
    assert voxproj_host.VP_ABI_VERSION == 4
    L = voxproj_host.lib()
    for name, proto in protos.items():
        fn = getattr(L, name)
        assert _binding_error(proto, fn.restype, fn.argtypes) is None, (name, _binding_error(proto, fn.restype, fn.argtypes))
    proto, good = protos["vp_sh_colors"], list(L.vp_sh_colors.argtypes)
    assert proto[1][4] == "int64_t" and proto[1][3] == "float *" and len(good) == 10
    assert good[3] is ctypes.POINTER(ctypes.c_float)
    assert "argument 4 is int64_t" in _binding_error(proto, ctypes.c_int, good[:4] + [ctypes.c_int] + good[5:])
    assert "argument 3 is float *" in _binding_error(proto, ctypes.c_int, good[:3] + [ctypes.POINTER(ctypes.c_double)] + good[4:])
    assert "takes 10 arguments, bound with 9" in _binding_error(proto, ctypes.c_int, good[:-1])
    assert "returns int" in _binding_error(proto, ctypes.c_size_t, good)


def test_a_missing_ext_symbol_is_reported_by_name(monkeypatch):
    import voxproj_host

    class Function:
        restype = argtypes = None

        def __call__(self, *args):
            return 4

    class Library:
        def __init__(self, path):
            for name in voxproj_host.EXPORTS + ["vp_sh_colors"]:
                setattr(self, name, Function())

    monkeypatch.setattr(voxproj_host.ctypes, "CDLL", Library)
    monkeypatch.setattr(voxproj_host, "LIB_PATH", os.path.abspath(__file__))
    monkeypatch.setattr(voxproj_host, "_lib", None)
    L = voxproj_host.lib()
    assert isinstance(L, Library) and L.vp_sh_colors.argtypes is not None
    with pytest.raises(voxproj_host.VoxprojError, match=r"has no vp_sh_colors_backward"):
        voxproj_host._entry("vp_sh_colors_backward")


def test_entry_points_validate_on_the_host_before_any_launch():
    """Fake device addresses that are never dereferenced: every refusal is host arithmetic, and n = 0 launches nothing."""
    import voxproj_host
    L = voxproj_host.lib()
    P = 0x7000_0000_0000
    cam = (ctypes.c_float * 3)(0.3, -0.2, 0.1)
    base = dict(f_dc=P, f_rest=P + 4096, means=P + 8192, campos=cam, n=10, d=2, D=3, colors=P + 12288, clamped=P + 16384)

    def fwd(**kw):
        a = dict(base, **kw)
        return L.vp_sh_colors(a["f_dc"], a["f_rest"], a["means"], a["campos"], a["n"], a["d"], a["D"], a["colors"], a["clamped"], None)

    nan = (ctypes.c_float * 3)(0.0, float("nan"), 0.0)
    for kw, msg in ((dict(n=-1), b"outside [0, 2^31 - 1]"), (dict(n=1 << 31), b"outside [0, 2^31 - 1]"), (dict(d=3, D=2), b"degree"),
                    (dict(d=-1), b"degree"), (dict(d=4, D=4), b"max_degree <= 3"), (dict(campos=None), b"null campos"),
                    (dict(campos=nan), b"campos[1] is not finite"), (dict(means=None), b"means"), (dict(f_dc=None), b"null pointer"),
                    (dict(colors=None), b"null pointer"), (dict(f_rest=None), b"f_rest with degree > 0"),
                    (dict(f_rest=P + 4098), b"4-byte aligned")):
        assert fwd(**kw) == -1, kw
        assert msg in L.vp_last_error(), (kw, L.vp_last_error())
    assert fwd(n=0, f_dc=None, f_rest=None, means=None, colors=None, clamped=None) == 0

    bbase = dict(base, g=P + 20480, gd=P + 24576, gr=P + 28672, gm=P + 32768)

    def bwd(**kw):
        a = dict(bbase, **kw)
        return L.vp_sh_colors_backward(a["f_dc"], a["f_rest"], a["means"], a["campos"], a["n"], a["d"], a["D"], a["g"], a["clamped"],
                                       a["gd"], a["gr"], a["gm"], None)

    for kw, msg in ((dict(n=-5), b"outside [0, 2^31 - 1]"), (dict(d=2, D=1), b"degree"), (dict(g=None), b"grad_colors or clamped"),
                    (dict(clamped=None), b"grad_colors or clamped"), (dict(f_rest=None), b"needs f_rest"),
                    (dict(gr=P + 28673), b"4-byte aligned"), (dict(campos=None), b"null campos")):
        assert bwd(**kw) == -1, kw
        assert msg in L.vp_last_error(), (kw, L.vp_last_error())
    assert bwd(n=0) == 0
    assert bwd(gd=None, gr=None, gm=None) == 0                     # nothing asked for: nothing launched
