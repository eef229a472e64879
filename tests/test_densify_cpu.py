"""Adaptive density control without a GPU: the fused rule of vp_densify_plan against the reference's literal sequence, the
Philox / Box-Muller generator of the split, and the host logic (camera_extent, the exported symbols, the host-side refusals
and the new command-line options).  tests/densify_reference.py is the twin.

Fails without the vp_densify_* symbols, voxproj_host.camera_extent and the --densify_* options."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "3d-semantic-segmentation_amd")
for p in (HERE, ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import densify_reference as dr  # noqa: E402

NAMES = ("vp_densify_accumulate", "vp_densify_plan_workspace_bytes", "vp_densify_plan", "vp_densify_rows", "vp_densify_split")


@pytest.mark.parametrize("screen", [0.0, 20.0])
def test_fused_rule_equals_the_literal_sequence(screen):
    rng = np.random.default_rng(11)
    seen, ties = np.zeros(4, np.int64), np.zeros(3, np.int64)
    for it in range(300):
        n = int(rng.integers(0, 301)) if it else 0
        c, thr, size = dr.random_case(rng, n)
        if it % 3 == 0:
            c["max_radius"] = None
        kw = dict(grad_threshold=thr, size_threshold=size, min_opacity=0.005, max_screen_size=screen,
                  max_world_size=np.float32(0.12))
        fs, fk, fc = dr.plan_fused(**c, **kw)
        ls, lk, lc = dr.plan_literal(**c, **kw)
        assert np.array_equal(fs, ls) and np.array_equal(fk, lk) and np.array_equal(fc, lc), (it, n)
        assert fc[0] == fc[1] + fc[2] + 2 * fc[3] <= 2 * n
        seen += fc
        if n:
            with np.errstate(all="ignore"):
                gm = np.where(c["denom"] > 0, c["grad_accum"] / np.maximum(c["denom"], 1).astype(np.float32), 0)
            ties += [(c["denom"] == 0).sum(), (gm == thr).sum(), (c["scales"].max(1) == size).sum()]
    assert (seen[1:] > 0).all() and (ties > 100).all(), (seen, ties)   # denom = 0, gm at its threshold, smax at its own


def test_rule_edges():
    kw = dict(grad_threshold=0.5, size_threshold=1.0, min_opacity=0.1, max_world_size=10.0)
    one = np.ones(1, np.float32)
    sc = lambda v: np.full((1, 3), v, np.float32)  # noqa: E731
    # gm exactly at the threshold selects; smax exactly at the size threshold clones
    s, k, c = dr.plan_fused(0.5 * one, np.ones(1, np.int32), None, sc(1.0), one, **kw)
    assert k.tolist() == [0, 1] and s.tolist() == [0, 0] and c.tolist() == [2, 1, 1, 0]
    s, k, c = dr.plan_fused(0.5 * one, np.ones(1, np.int32), None, sc(1.5), one, **kw)
    assert k.tolist() == [2, 3] and c.tolist() == [2, 0, 0, 1]
    # denom 0 and a NaN statistic count as 0
    assert dr.plan_fused(9 * one, np.zeros(1, np.int32), None, sc(1.0), one, **kw)[1].tolist() == [0]
    assert dr.plan_fused(np.full(1, np.nan, np.float32), np.ones(1, np.int32), None, sc(1.0), one, **kw)[1].tolist() == [0]
    # a faint Gaussian goes, with whatever it would have emitted
    assert dr.plan_fused(one, np.ones(1, np.int32), None, sc(1.0), 0.05 * one, **kw)[2].tolist() == [0, 0, 0, 0]
    # size rules: a large split source leaves children below the world size (16 * 0.625 = 10), a larger one nothing
    on = dict(kw, max_screen_size=20.0)
    assert dr.plan_fused(one, np.ones(1, np.int32), None, sc(16.0), one, **on)[1].tolist() == [2, 3]
    assert dr.plan_fused(one, np.ones(1, np.int32), None, sc(16.5), one, **on)[2].tolist() == [0, 0, 0, 0]
    # the screen radius prunes an original but not its clone
    s, k, c = dr.plan_fused(one, np.ones(1, np.int32), 21 * one, sc(1.0), one, **on)
    assert k.tolist() == [1] and c.tolist() == [1, 0, 1, 0]


def test_philox_known_answers():
    z = dr.philox4x32_10(np.zeros((1, 4), np.uint32), [0, 0])[0]
    assert [f"{v:08x}" for v in z] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    f = dr.philox4x32_10(np.full((1, 4), 0xFFFFFFFF, np.uint32), [0xFFFFFFFF, 0xFFFFFFFF])[0]
    assert [f"{v:08x}" for v in f] == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]


def test_split_normals_are_standard_normal():
    n = 100_000 // 3 + 1
    xi = dr.split_normals(np.arange(n), np.arange(n) % 2, seed=(7 << 32) | 5).reshape(-1)[:100_000]
    assert np.isfinite(xi).all()
    m = len(xi)
    assert abs(xi.mean()) <= 5.0 / np.sqrt(m)                    # the standard error of the mean of m unit normals
    assert abs(xi.var() - 1.0) <= 5.0 * np.sqrt(2.0 / m)         # and of their variance
    other = dr.split_normals(np.arange(8), np.zeros(8), seed=6)
    assert not np.array_equal(other, dr.split_normals(np.arange(8), np.zeros(8), seed=7))
    assert not np.array_equal(other, dr.split_normals(np.arange(8), np.ones(8), seed=6))


def test_split_geometry_twin():
    rng = np.random.default_rng(2)
    n = 50
    means, quats = rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(n, 4)).astype(np.float32)
    ls = rng.normal(-3, 0.5, (n, 3)).astype(np.float32)
    src = np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2), np.arange(1, n, 2)]).astype(np.int32)
    kind = np.concatenate([np.zeros(n // 2), np.full(n // 2, 2), np.full(n // 2, 3)]).astype(np.uint8)
    om, ol, bound = dr.split_geometry(means, quats, ls, src, kind, seed=3)
    assert om[:n // 2].tobytes() == means[::2].tobytes() and ol[:n // 2].tobytes() == ls[::2].tobytes()
    assert np.allclose(np.exp(ol[n // 2:].astype(np.float64)), 0.625 * np.exp(ls[src[n // 2:]].astype(np.float64)), rtol=1e-6)
    d = (om[n // 2:].astype(np.float64) - means[src[n // 2:]]) / np.exp(ls[src[n // 2:]].astype(np.float64)).max(1, keepdims=True)
    assert np.abs(d).max() < 6.0 and np.abs(d).max() > 0.5       # within a few sigma of the source, and moved
    assert (bound[:n // 2] == 0).all() and (bound[n // 2:] > 0).all()


def test_camera_extent_on_a_hand_made_rig():
    import voxproj_host
    # four cameras at (+-2, 0, 0) and (0, +-1, 0), each rotated about z: c = -R^T t
    vms = []
    for c, ang in (((2, 0, 0), 0.3), ((-2, 0, 0), 1.0), ((0, 1, 0), -0.7), ((0, -1, 0), 2.0)):
        R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
        vm = np.eye(4)
        vm[:3, :3], vm[:3, 3] = R, -R @ np.array(c, float)
        vms.append(vm)
    assert abs(voxproj_host.camera_extent(vms) - 2.2) < 1e-12
    assert abs(dr.camera_extent(vms) - 2.2) < 1e-12
    shifted = [vm.copy() for vm in vms]
    for vm in shifted:
        vm[:3, 3] -= vm[:3, :3] @ np.array([5.0, -3.0, 1.0])      # the same rig somewhere else
    assert abs(voxproj_host.camera_extent(shifted) - 2.2) < 1e-12


def test_symbols_are_exported_and_declared():
    import voxproj_host
    voxproj_host.build()
    lib = ctypes.CDLL(voxproj_host.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "voxproj.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in voxproj_host.EXPORTS and f" {name}(" in hdr
    assert voxproj_host.lib().vp_abi_version() == 4


def test_host_side_refusals_need_no_gpu():
    import voxproj_host
    L = voxproj_host.lib()
    P, vp = 0x7000_0000_0000, ctypes.c_void_p                # "device" addresses, never dereferenced
    err = lambda: L.vp_last_error()  # noqa: E731
    # accumulate
    acc = lambda **kw: L.vp_densify_accumulate(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("gs", P), ("n", 10), ("W", 40), ("H", 24), ("scale", 1.0), ("means", None), ("quats", None), ("scales", None),
        ("vm", None), ("fx", 0.0), ("fy", 0.0), ("cx", 0.0), ("cy", 0.0), ("eps", 0.3), ("ga", P + 4096), ("dn", P + 8192),
        ("rad", None), ("ws", P + (1 << 20)), ("wsb", 0), ("stream", None))])
    assert acc(gs=None) == -1 and b"null pointer" in err()
    assert acc(n=-1) == -1 and acc(W=0) == -1 and acc(scale=float("inf")) == -1
    assert acc(rad=P + 12288) == -1 and b"needed by max_radius" in err()
    assert acc(ws=None) == -2 and acc(ws=P + 16) == -2 and b"256-byte aligned" in err()
    # the size check needs rocprim's scratch size, which asks the device: only where there is one
    # plan
    assert L.vp_densify_plan_workspace_bytes(-1) == 0 and L.vp_densify_plan_workspace_bytes((1 << 30) + 1) == 0
    plan = lambda **kw: L.vp_densify_plan(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("ga", P), ("dn", P + 4096), ("rad", None), ("sc", P + 8192), ("op", P + 12288), ("n", 10), ("thr", 0.0002),
        ("size", 0.05), ("lo", 0.005), ("scr", 0.0), ("world", 0.5), ("src", P + 16384), ("kind", P + 20480),
        ("counts", P + 24576), ("ws", P + (1 << 20)), ("wsb", 0), ("stream", None))])
    assert plan(n=(1 << 30) + 1) == -1 and b"2^30" in err()
    assert plan(counts=None) == -1 and plan(src=None) == -1 and b"null pointer" in err()
    assert plan(thr=0.0) == -1 and plan(thr=float("nan")) == -1 and b"grad_threshold" in err()
    assert plan(world=float("nan")) == -1
    assert plan(ws=None) == -2
    # rows
    A = voxproj_host._DensifyArray
    rows = lambda a, n=1, n_src=10, n_out=12, counts=P: L.vp_densify_rows(  # noqa: E731
        (A * len(a))(*a) if a else None, n, vp(P + 4096), vp(P + 8192), vp(counts), n_src, n_out, None, None)
    good = A(P + 65536, P + 131072, 3, 0, 3, 3)
    assert rows(None) == -1 and rows([good], n=0) == -1 and rows([good] * 17, n=17) == -1
    assert rows([good], n_out=21) == -1 and b"n_out" in err()
    assert rows([good], counts=None) == -1
    assert rows([A(P + 65536, P + 131072, 0, 0, 3, 3)]) == -1 and rows([A(P + 65536, P + 131072, 4097, 0, 4097, 4097)]) == -1
    assert rows([A(P + 65536, P + 131072, 3, 0, 2, 3)]) == -1 and b"stride" in err()
    assert rows([A(P + 65536, P + 131072, 3, 2, 3, 3)]) == -1 and b"fill" in err()
    assert rows([A(P + 65536, None, 3, 0, 3, 3)]) == -1 and rows([A(P + 65538, P + 131072, 3, 0, 3, 3)]) == -1
    # split
    split = lambda **kw: L.vp_densify_split(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("m", P), ("q", P + 4096), ("ls", P + 8192), ("n_src", 10), ("src", P + 12288), ("kind", P + 16384), ("counts", P + 20480),
        ("n_out", 12), ("seed", 1), ("om", P + 24576), ("ol", P + 28672), ("status", None), ("stream", None))])
    assert split(q=None) == -1 and split(om=None) == -1 and split(n_out=-1) == -1 and split(counts=None) == -1


def test_cli_refuses_bad_densification_options(capsys):
    import fit_gaussian_appearance as fga
    base = ["--gaussians_ply", "x.ply", "--cam_params", "x.json", "--images_dir", "x", "--out", "y.ply"]
    bad = (["--densify_interval", "-1"], ["--opacity_reset_interval", "-5"],
           ["--densify_from", "100", "--densify_until", "100"], ["--densify_from", "200", "--densify_until", "100"],
           ["--densify_grad_threshold", "0"], ["--densify_grad_threshold", "-0.1"], ["--percent_dense", "0"],
           ["--min_opacity", "0"], ["--max_screen_size", "-1"], ["--scene_extent", "0"])
    for extra in bad:
        ap = fga.build_parser()
        with pytest.raises(SystemExit) as e:
            fga.check_densify_args(ap, ap.parse_args(base + extra))
        assert e.value.code == 2, extra
    capsys.readouterr()
    a = fga.build_parser().parse_args(base)
    fga.check_densify_args(fga.build_parser(), a)                # the defaults pass
    assert (a.densify_interval, a.densify_from, a.densify_until, a.opacity_reset_interval) == (0, 500, 15000, 0)
    assert (a.densify_grad_threshold, a.percent_dense, a.min_opacity, a.max_screen_size, a.scene_extent) == \
        (0.0002, 0.01, 0.005, 0.0, None)
