"""vp_densify_plan on the GPU against the NumPy twin (tests/densify_reference.py): src, kind and counts bit for bit, for every
size that crosses a workgroup or a scan block, every mix of decisions, with and without the screen radius and the size
rules; rows beyond the total stay as they were.

Fails on a library without vp_densify_plan."""
import ctypes
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

import densify_reference as dr  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 64, 65, 255, 256, 257, 1025, 70_000)
MIXES = ("kept", "pruned", "cloned", "split", "random", "ties")
F32 = np.float32


def make_case(mix, n, seed):
    rng = np.random.default_rng(seed)
    c, thr, size = dr.random_case(rng, n, ties=mix == "ties")
    if mix == "kept":
        c["grad_accum"] = np.full(n, 1e-6, F32)
        c["opacities"] = rng.uniform(0.5, 1.0, n).astype(F32)
        c["scales"] = np.full((n, 3), 0.01, F32)
        c["max_radius"] = np.full(n, 5.0, F32)
    elif mix == "pruned":
        c["opacities"] = rng.uniform(0.0, 0.004, n).astype(F32)
    elif mix in ("cloned", "split"):
        c["grad_accum"], c["denom"] = np.full(n, 1.0, F32), np.ones(n, np.int32)
        c["opacities"] = rng.uniform(0.5, 1.0, n).astype(F32)
        c["scales"] = np.full((n, 3), 0.01 if mix == "cloned" else 0.08, F32)
        c["max_radius"] = np.full(n, 5.0, F32)
    return c, thr, size


def run_plan(c, dev, **kw):
    """The raw entry point on buffers of the test's own, filled with canaries: (src [2N], kind [2N], counts [4]) as NumPy."""
    import voxproj_host
    L = voxproj_host._densify_lib()
    n = len(c["opacities"])
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in c.items() if v is not None}
    src = torch.full((2 * n + 8,), -7, dtype=torch.int32, device=dev)
    kind = torch.full((2 * n + 8,), 0xEE, dtype=torch.uint8, device=dev)
    counts = torch.full((6,), -1, dtype=torch.int64, device=dev)
    ws = voxproj_host.SplatWorkspace()
    ptr = ws.ensure(int(L.vp_densify_plan_workspace_bytes(n)), dev)
    p = voxproj_host._ptr
    rc = L.vp_densify_plan(p(t["grad_accum"]), p(t["denom"]), p(t.get("max_radius")), p(t["scales"]), p(t["opacities"]), n,
                           kw["grad_threshold"], kw["size_threshold"], kw["min_opacity"], kw["max_screen_size"],
                           kw["max_world_size"], src.data_ptr(), kind.data_ptr(), counts.data_ptr(), ptr, ws.capacity(),
                           torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, voxproj_host.last_error()
    return src.cpu().numpy(), kind.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize("n", SIZES)
def test_plan_matches_the_twin(n):
    dev = torch.device("cuda:0")
    totals = set()
    for mi, mix in enumerate(MIXES):
        c, thr, size = make_case(mix, n, 100 * mi + n % 97)
        for with_radius in (True, False):
            for screen in (0.0, 20.0):
                cc = dict(c, max_radius=c["max_radius"] if with_radius else None)
                kw = dict(grad_threshold=float(thr), size_threshold=float(size), min_opacity=0.005, max_screen_size=screen,
                          max_world_size=float(F32(0.12)))
                es, ek, ec = dr.plan_fused(**cc, **kw)
                src, kind, counts = run_plan(cc, dev, **kw)
                tag = (mix, n, with_radius, screen)
                assert counts[:4].tolist() == ec.tolist(), tag
                assert counts[4:].tolist() == [-1, -1], tag
                tot = int(ec[0])
                assert src[:tot].tobytes() == es.tobytes() and kind[:tot].tobytes() == ek.tobytes(), tag
                assert (src[tot:] == -7).all() and (kind[tot:] == 0xEE).all(), tag      # beyond the total: untouched
                totals.add((mix, tot))
        if n and mix == "kept":
            assert tot == n
        if n and mix == "pruned":
            assert tot == 0
        if n and mix in ("cloned", "split"):
            assert tot == 2 * n


def test_wrapper_and_determinism():
    import voxproj_host
    dev = torch.device("cuda:0")
    n = 5000
    c, thr, size = make_case("random", n, 5)
    stats = voxproj_host.DensifyStats(n, dev, want_radius=True)
    stats.grad_accum.copy_(torch.from_numpy(c["grad_accum"]))
    stats.denom.copy_(torch.from_numpy(c["denom"]))
    stats.max_radius.copy_(torch.from_numpy(c["max_radius"]))
    sc, op = torch.from_numpy(c["scales"]).to(dev), torch.from_numpy(c["opacities"]).to(dev)
    kw = dict(grad_threshold=float(thr), size_threshold=float(size), min_opacity=0.005, max_screen_size=20.0,
              max_world_size=float(F32(0.12)))
    a = voxproj_host.densify_plan(stats, sc, op, **kw)
    b = voxproj_host.densify_plan(stats, sc, op, **kw)
    es, ek, ec = dr.plan_fused(**c, **kw)
    assert [a.n_out, a.kept, a.clones, a.split] == ec.tolist() and a.n == n
    assert a.src[:a.n_out].cpu().numpy().tobytes() == es.tobytes() == b.src[:b.n_out].cpu().numpy().tobytes()
    assert a.kind[:a.n_out].cpu().numpy().tobytes() == ek.tobytes() == b.kind[:b.n_out].cpu().numpy().tobytes()
    with pytest.raises(ValueError):
        voxproj_host.densify_plan(stats, sc, op, **dict(kw, grad_threshold=0.0))
    with pytest.raises(ValueError):
        voxproj_host.densify_plan(stats, sc[:10], op, **kw)
