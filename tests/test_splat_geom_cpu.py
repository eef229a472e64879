"""CPU tests of the geometry backward: the float64 reference (tests/splat_geom_reference.py) against central finite
differences of a float64 loss with unrounded records, its per-Gaussian chain against torch's float64 autograd Jacobian, the
structure of the gradients, and the host-side refusals of vp_splat_geometry_backward_workspace_bytes /
vp_splat_rasterize_backward_geometry and of the Python entry points (fake device pointers, never dereferenced)."""
import ctypes
import os

import numpy as np
import pytest

import splat_geom_reference as geo
import splat_grad_reference as gref
import splat_reference as ref
from test_splat_grad_cpu import ID, K_, args, small_scene

FAKE = 0x7000_0000_0000
WS = 0x7100_0000_0000             # 256-byte aligned
BWS = 0x7200_0000_0000
PARAMS = (("means", 3, "grad_means", "M_means"), ("quats", 4, "grad_quats", "M_quats"), ("scales", 3, "grad_scales", "M_scales"))


def test_reference_extends_the_existing_one():
    # same sweep, same records: the features' and opacities' gradients are the existing reference's, and the unrounded
    # projection rounds to splat_reference.project's records
    s, K, W, H, G, Ga = small_scene(6, 3, 0)
    a = geo.splat_geom64(*args(s), ID, K, W, H, G=G, G_alpha=Ga)
    b = gref.splat_grad64(*args(s), ID, K, W, H, G=G, G_alpha=Ga)
    for k in ("grad_f", "grad_o", "M_f", "M_o", "fragile", "visits", "added"):
        assert np.array_equal(a[k], b[k]), k
    P = geo.project64(s["means"], s["quats"], s["scales"], s["opacities"], ID, K, W, H)
    keep, _, m2, con, _, _ = ref.project(s["means"], s["quats"], s["scales"], s["opacities"], ID, K, W, H)
    assert np.array_equal(P["keep"], keep)
    assert np.array_equal(P["mean2d"].astype(np.float32), m2.astype(np.float32))
    assert np.array_equal(P["conic"].astype(np.float32), con.astype(np.float32))


def fd_setup(seed):
    """Scene with zero upstream gradient on the pixels fragile at 1e-2, and the analytic gradients on unrounded records."""
    s, K, W, H, G, Ga = small_scene(6, 3, seed)
    s = {k: v.astype(np.float64) for k, v in s.items()}
    frag = geo.splat_geom64(*args(s), ID, K, W, H, G=G, G_alpha=Ga, fragile_rel=1e-2, round_records=False)["fragile"]
    G[:, frag] = 0.0
    Ga[frag] = 0.0
    assert (~frag).sum() >= 0.5 * W * H
    r = geo.splat_geom64(*args(s), ID, K, W, H, G=G, G_alpha=Ga, round_records=False)
    return s, K, W, H, G, Ga, r


def central(s, K, W, H, G, Ga, name, g, c, h):
    """Central difference of the unrounded float64 loss; asserts that both ends added the same (pixel, Gaussian) pairs."""
    hi, lo = dict(s), dict(s)
    hi[name], lo[name] = s[name].copy(), s[name].copy()
    hi[name][g, c] += h
    lo[name][g, c] -= h
    lh, ph = geo.forward64(*args(hi), ID, K, W, H, G, Ga)
    ll, pl = geo.forward64(*args(lo), ID, K, W, H, G, Ga)
    live = (G != 0).any(0) | (Ga != 0)                      # pixels that carry an upstream gradient
    assert np.array_equal(ph[:, live], pl[:, live]), f"a decision flipped between the ends of the step on {name}[{g},{c}]"
    return (lh - ll) / (2 * h)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_geometry_gradient_finite_differences(seed):
    # h = 2^-12 as in the opacity test.  A central difference carries a truncation term c h^2 (c = f'''/6): FD(h) - FD(h/2) =
    # 3/4 c h^2, so FD(h/2) is off by (FD(h) - FD(h/2)) / 3.  The tolerance is the opacity test's 1e-5 M plus twice that
    # measured term (the factor 2 covers the h^4 term)
    s, K, W, H, G, Ga, r = fd_setup(seed)
    h = 2.0 ** -12
    worst = 0.0
    for name, n, gk, mk in PARAMS:
        for g in range(6):
            for c in range(n):
                f1 = central(s, K, W, H, G, Ga, name, g, c, h)
                f2 = central(s, K, W, H, G, Ga, name, g, c, h / 2)
                tol = 1e-5 * r[mk][g, c] + 2.0 * abs(f1 - f2) / 3.0 + 1e-12
                err = abs(f2 - r[gk][g, c])
                worst = max(worst, err / tol)
                assert err <= tol, (name, g, c, f1, f2, r[gk][g, c], tol)
        assert (np.abs(r[gk]) > 1e-3 * np.abs(r[gk]).max()).sum() >= 2 * n, name
    print(f"seed {seed}: worst err / tol {worst:.3f}")


def test_halving_the_step_quarters_the_disagreement():
    # on the entry with the largest truncation term the disagreement is c h^2: halving h must cut it about fourfold
    s, K, W, H, G, Ga, r = fd_setup(0)
    best = None
    for g in range(6):
        for c in range(3):
            f1 = central(s, K, W, H, G, Ga, "means", g, c, 2.0 ** -11)
            f2 = central(s, K, W, H, G, Ga, "means", g, c, 2.0 ** -12)
            if best is None or abs(f1 - f2) > best[0]:
                best = (abs(f1 - f2), g, c, f1, f2)
    _, g, c, f1, f2 = best
    f3 = central(s, K, W, H, G, Ga, "means", g, c, 2.0 ** -13)
    a = r["grad_means"][g, c]
    e1, e2, e3 = abs(f1 - a), abs(f2 - a), abs(f3 - a)
    assert e1 > 1e3 * 1e-12 * (1 + abs(a)), "truncation must dominate rounding here"
    assert 3.5 <= e1 / e2 <= 4.5 and 3.5 <= e2 / e3 <= 4.5, (e1, e2, e3)


def torch_project(theta, vm, K, W, H, eps2d):
    """(means 3, quats 4, scales 3) of one Gaussian -> (mean2d x, y, conic A, B, C), written independently in torch."""
    import torch
    m, q, s = theta[:3], theta[3:7], theta[7:]
    w, x, y, z = q / q.norm()
    R = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)]),
                     torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)]),
                     torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)])])
    Rw, t = vm[:3, :3], vm[:3, 3]
    Sig = Rw @ R @ torch.diag(s * s) @ R.T @ Rw.T
    p = Rw @ m + t
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    tx = p[2] * torch.clamp(p[0] / p[2], -(cx / fx + 0.15 * W / fx), (W - cx) / fx + 0.15 * W / fx)
    ty = p[2] * torch.clamp(p[1] / p[2], -(cy / fy + 0.15 * H / fy), (H - cy) / fy + 0.15 * H / fy)
    zero = torch.zeros((), dtype=torch.float64)
    J = torch.stack([torch.stack([fx / p[2], zero, -fx * tx / p[2] ** 2]), torch.stack([zero, fy / p[2], -fy * ty / p[2] ** 2])])
    S2 = J @ Sig @ J.T + eps2d * torch.eye(2, dtype=torch.float64)
    con = torch.linalg.inv(S2)
    return torch.stack([fx * p[0] / p[2] + cx, fy * p[1] / p[2] + cy, con[0, 0], con[0, 1], con[1, 1]])


def test_chain_against_torch_jacobian():
    import torch
    rng = np.random.default_rng(7)
    W, H = 20, 16
    K = K_(12.0, W, H)
    vm = np.eye(4, dtype=np.float32)
    vm[:3, :3] = np.float32([[0.995, 0.0, 0.0998], [0.01, 0.99995, -0.0997], [-0.0998, 0.01, 0.995]])   # read as given
    vm[:3, 3] = (0.02, -0.01, 0.1)
    n = 8
    means = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.4, 0.4, n), rng.uniform(1.5, 3.0, n)], 1)
    means[0] = (3.2, 0.1, 2.0)                 # p_x / z beyond the clamp: the clamped branch in x
    means[1] = (0.2, -2.9, 2.2)                # and in y
    quats = rng.normal(size=(n, 4)) * rng.uniform(0.3, 3.0, (n, 1))        # far from unit norm
    scales = 0.15 * np.exp(rng.normal(0, 0.3, (n, 3)))
    P = geo.project64(means, quats, scales, np.full(n, 0.5), vm, K, W, H)
    assert P["keep"].all() and not P["inx"][0] and not P["iny"][1] and P["inx"][2:].all() and P["iny"][2:].all()
    assert np.abs(np.linalg.norm(quats, axis=1) - 1).min() > 0.01
    jac = geo.chain_jacobian(P)
    vm_t, K_t = torch.from_numpy(vm).double(), torch.from_numpy(K).double()
    for g in range(n):
        theta = torch.from_numpy(np.concatenate([means[g], quats[g], scales[g]]))
        out = torch_project(theta, vm_t, K_t, W, H, 0.3).numpy()
        assert np.allclose(out[:2], P["mean2d"][g], rtol=1e-12) and np.allclose(out[2:], P["conic"][g], rtol=1e-12)
        jt = torch.autograd.functional.jacobian(lambda th: torch_project(th, vm_t, K_t, W, H, 0.3), theta).numpy()
        scale = np.abs(jt).max(axis=1, keepdims=True)
        assert (np.abs(jac[g] - jt) <= 1e-9 * scale).all(), (g, np.abs(jac[g] - jt).max())
        assert (np.abs(jt) > 0).sum() >= 30


def test_quaternion_gradient_is_orthogonal_to_the_quaternion():
    s, K, W, H, G, Ga = small_scene(6, 3, 1)
    s["quats"] *= np.float32([[0.5], [2.0], [1.0], [3.0], [0.7], [1.3]])
    r = geo.splat_geom64(*args(s), ID, K, W, H, G=G, G_alpha=Ga)
    dot = (r["grad_quats"] * s["quats"]).sum(1)
    assert (np.abs(dot) <= 1e-14 * (np.abs(r["grad_quats"]) * np.abs(s["quats"])).sum(1) + 1e-300).all()
    assert (np.abs(r["grad_quats"]).max(1) > 0).sum() >= 4


def test_logits_only_and_alpha_only_add_up():
    s, K, W, H, G, Ga = small_scene(6, 3, 5)
    both = geo.splat_geom64(*args(s), ID, K, W, H, G=G, G_alpha=Ga)
    lo = geo.splat_geom64(*args(s), ID, K, W, H, G=G)
    al = geo.splat_geom64(*args(s), ID, K, W, H, G_alpha=Ga)
    for k, m in (("grad_screen", "M_screen"), ("grad_means", "M_means"), ("grad_quats", "M_quats"), ("grad_scales", "M_scales")):
        assert (np.abs(lo[k] + al[k] - both[k]) <= 1e-12 * both[m] + 1e-300).all(), k
        assert (both[k] != 0).sum() >= 0.5 * both[k].size


def test_culled_and_behind_the_stop_give_zero_rows():
    # three opaque Gaussians on the axis (the third is behind the stop at the only pixel with a gradient), one behind the
    # camera, one with a zero quaternion, one too faint
    def one(m, o, q=(1, 0, 0, 0)):
        return dict(means=np.array([m], np.float32), quats=np.array([q], np.float32), scales=np.array([[0.3] * 3], np.float32),
                    opacities=np.array([o], np.float32), features=np.ones((1, 3)))
    gs = [one((0.01, 0.02, 2.0), 0.98), one((0.0, 0.01, 3.0), 0.98), one((0.02, 0.0, 4.0), 0.98), one((0, 0, -2.0), 0.9),
          one((0.1, 0, 2.5), 0.9, q=(0, 0, 0, 0)), one((0.1, 0, 2.5), 0.003)]
    s = {k: np.concatenate([g[k] for g in gs]) for k in gs[0]}
    W = H = 9
    G = np.zeros((3, H, W))
    G[:, 4, 4] = 1.0
    Ga = np.zeros((H, W))
    Ga[4, 4] = 1.0
    r = geo.splat_geom64(*args(s), ID, K_(10.0, W, H), W, H, G=G, G_alpha=Ga)
    assert r["visits"][4, 4] == 2
    for k in ("grad_screen", "grad_means", "grad_quats", "grad_scales"):
        assert (r[k][2:] == 0).all(), k
        assert (r[k][:2] != 0).any(axis=1).all() or k == "grad_quats", k      # isotropic scales: no gradient in q
    assert np.abs(r["grad_quats"]).max() <= 1e-12 * np.abs(r["grad_means"]).max()


# ------------------------------------------------------------------------------------------------ host side
@pytest.fixture(scope="module")
def lib():
    import voxproj_host
    voxproj_host.build()
    return voxproj_host.lib()


VM = (ctypes.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1).tolist())


def _geo(lib, means=FAKE, quats=FAKE, scales=FAKE, feats=FAKE, D=32, stride=32, n=10, vm=VM, fx=10.0, fy=10.0, cx=32.0,
         cy=24.0, W=64, H=48, eps2d=0.3, cap=100, gm=FAKE, ws=WS, ws_bytes=1 << 30, bws=BWS, bws_bytes=None):
    vp = ctypes.c_void_p
    if bws_bytes is None:
        bws_bytes = lib.vp_splat_geometry_backward_workspace_bytes(max(cap, 0), D) or (1 << 30)
    return lib.vp_splat_rasterize_backward_geometry(vp(means), vp(quats), vp(scales), vp(feats), D, stride, n, vm, fx, fy, cx,
                                                    cy, W, H, eps2d, cap, vp(FAKE), None, vp(gm), vp(FAKE), vp(FAKE),
                                                    vp(FAKE), vp(FAKE), vp(FAKE), None, vp(ws), ws_bytes, vp(bws), bws_bytes,
                                                    None)


def _nan_vm():
    v = np.eye(4, dtype=np.float32).reshape(-1)
    v[5] = np.nan
    return (ctypes.c_float * 16)(*v.tolist())


@pytest.mark.parametrize("kw,code,msg", [
    (dict(feats=0), -1, b"null pointer"),
    (dict(means=0), -1, b"null pointer"),
    (dict(quats=0), -1, b"null pointer"),
    (dict(scales=0), -1, b"null pointer"),
    (dict(vm=None), -1, b"null viewmat"),
    (dict(vm=_nan_vm()), -1, b"viewmat[5]"),
    (dict(fx=0.0), -1, b"fx, fy"),
    (dict(fy=float("inf")), -1, b"fx, fy"),
    (dict(eps2d=-1.0), -1, b"eps2d"),
    (dict(D=0, stride=0), -1, b"D = 0"),
    (dict(D=65, stride=65), -1, b"D = 65"),
    (dict(stride=31), -1, b"row_stride"),
    (dict(cap=-1), -1, b"capacity"),
    (dict(W=33000), -1, b"image"),
    (dict(H=0), -1, b"image"),
    (dict(n=-2), -1, b"n_gaussians"),
    (dict(n=1 << 31), -1, b"n_gaussians"),
    (dict(ws=0), -2, b"workspace is NULL"),
    (dict(ws=WS + 64), -2, b"256-byte aligned"),
    (dict(bws=0), -2, b"backward workspace is NULL"),
    (dict(bws=BWS + 16), -2, b"backward workspace must be 256-byte aligned"),
    (dict(bws_bytes=100 * 38 * 4 - 1), -2, b"backward workspace has"),
])
def test_geometry_backward_refusals(lib, kw, code, msg):
    assert _geo(lib, **kw) == code
    assert msg in lib.vp_last_error()


def test_geometry_backward_workspace_bytes(lib):
    up = lambda v: -(-v // 256) * 256  # noqa: E731
    assert lib.vp_splat_geometry_backward_workspace_bytes(1000, 13) == up(1000 * (13 + 1 + 5) * 4)
    assert lib.vp_splat_geometry_backward_workspace_bytes(2_700_000, 64) == up(2_700_000 * 70 * 4)
    assert lib.vp_splat_geometry_backward_workspace_bytes(0, 1) == 256
    for cap, D in ((-1, 8), (1 << 31, 8), (100, 0), (100, 65)):
        assert lib.vp_splat_geometry_backward_workspace_bytes(cap, D) == 0
    assert lib.vp_splat_backward_workspace_bytes(1000, 13) == up(1000 * 14 * 4)        # the existing scratch keeps its size


def test_symbols_in_exports_and_header(lib):
    import voxproj_host
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "voxproj.h")).read()
    for name in ("vp_splat_geometry_backward_workspace_bytes", "vp_splat_rasterize_backward_geometry"):
        assert name in voxproj_host.EXPORTS and f" {name}(" in hdr
        assert getattr(lib, name) is not None
    assert voxproj_host.VP_ABI_VERSION == 4 and lib.vp_abi_version() == 4


def test_python_refusals_before_device_work():
    import torch
    import splat_autograd
    import voxproj_host
    m, q, s, o, f = torch.zeros(4, 3), torch.zeros(4, 4), torch.zeros(4, 3), torch.zeros(4), torch.zeros(4, 8)
    vm, K = np.eye(4), K_(10, 16, 16)
    with pytest.raises(ValueError, match="CUDA tensor"):
        splat_autograd.splat_gaussians(m.clone().requires_grad_(), q, s, o, f, vm, K, 16, 16)
    with pytest.raises(ValueError, match="float32"):
        splat_autograd.splat_gaussians(m.double().requires_grad_(), q, s, o, f, vm, K, 16, 16)
    with pytest.raises(ValueError, match="float32"):
        splat_autograd.splat_gaussians(m, q, s.half(), o, f, vm, K, 16, 16)
    with pytest.raises(ValueError, match="CUDA tensor"):
        voxproj_host.splat_rasterize_backward_geometry(m, q, s, f, vm, K, 16, 16, 10, voxproj_host.SplatWorkspace())
    with pytest.raises(ValueError, match="float32"):
        voxproj_host.splat_rasterize_backward_geometry(m, q.double(), s, f, vm, K, 16, 16, 10, voxproj_host.SplatWorkspace())
