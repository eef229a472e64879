"""vp_densify_rows and vp_densify_split on the GPU, and the Adam resampling built on them: the row gather against NumPy
indexing bit for bit (every lane layout the widths pick, strides above the width, padding and canaries untouched), the status
word on a wrong n_out, resample_adam, and the split children against the NumPy twin (tests/densify_reference.py).

Fails on a library without vp_densify_rows."""
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

WIDTHS = (1, 3, 4, 16, 40, 64, 65, 512)
F32 = np.float32


@pytest.fixture(scope="module")
def plan():
    """One plan with every kind of row, shared and left unchanged: (DensifyPlan, src, kind as NumPy)."""
    import voxproj_host
    dev = torch.device("cuda:0")
    n = 1500
    c, thr, size = dr.random_case(np.random.default_rng(21), n)
    stats = voxproj_host.DensifyStats(n, dev)
    stats.grad_accum.copy_(torch.from_numpy(c["grad_accum"]))
    stats.denom.copy_(torch.from_numpy(c["denom"]))
    pl = voxproj_host.densify_plan(stats, torch.from_numpy(c["scales"]).to(dev), torch.from_numpy(c["opacities"]).to(dev),
                                   grad_threshold=float(thr), size_threshold=float(size), min_opacity=0.005,
                                   max_world_size=0.12)
    src, kind = pl.src[:pl.n_out].cpu().numpy(), pl.kind[:pl.n_out].cpu().numpy()
    assert pl.kept > 100 and pl.clones > 100 and pl.split > 100 and pl.n_out > n
    return pl, src, kind


def make_array(rng, n, width, stride, dtype):
    """A [n, stride] host array of distinct bit patterns (no NaN games needed: rows move as 32-bit words)."""
    a = rng.integers(-2 ** 31, 2 ** 31 - 1, (n, stride), dtype=np.int64).astype(np.int32)
    return a.view(np.float32) if dtype == torch.float32 else a


def expected(a, src, kind, fill, width):
    e = a[src, :width].copy()
    if fill == "zero":
        e.view(np.int32)[kind != 0] = 0
    return e


@pytest.mark.parametrize("width", WIDTHS)
def test_rows_match_numpy_indexing(plan, width):
    import voxproj_host
    pl, src, kind = plan
    dev = pl.src.device
    rng = np.random.default_rng(width)
    for dtype in (torch.float32, torch.int32):
        for fill in ("copy", "zero"):
            for pad_src, pad_dst in ((0, 0), (3, 5), (4, 8)):
                a = make_array(rng, pl.n, width, width + pad_src, dtype)
                canary = make_array(rng, pl.n_out + 2, width, width + pad_dst, dtype)
                ta, td = torch.from_numpy(a).to(dev), torch.from_numpy(canary).to(dev)
                voxproj_host.densify_rows([(ta[:, :width], td[1:-1, :width], fill)], pl.src, pl.kind, pl.counts, pl.n, pl.n_out,
                                          pl.status)
                got = td.cpu().numpy()
                tag = (width, dtype, fill, pad_src, pad_dst)
                assert got[1:-1, :width].tobytes() == expected(a, src, kind, fill, width).tobytes(), tag
                assert got[1:-1, width:].tobytes() == canary[1:-1, width:].tobytes(), tag      # the padding
                assert got[0].tobytes() == canary[0].tobytes() and got[-1].tobytes() == canary[-1].tobytes(), tag
    assert int(pl.status.item()) == 0


@pytest.mark.parametrize("count", (1, 2, 16, 17))
def test_many_arrays_in_one_call(plan, count):
    pl, src, kind = plan
    dev = pl.src.device
    rng = np.random.default_rng(count)
    host, arrays = {}, {}
    for i in range(count):
        width = WIDTHS[i % len(WIDTHS)] if i % 5 else 7
        dtype = torch.int32 if i % 3 == 0 else torch.float32
        fill = "zero" if i % 2 else "copy"
        shape_tail = (width,) if i % 4 else ((width,) if width % 2 else (width // 2, 2))
        a = make_array(rng, pl.n, width, width, dtype)
        host[f"a{i}"] = (a, fill, width)
        arrays[f"a{i}"] = (torch.from_numpy(a).to(dev).reshape((pl.n,) + shape_tail), fill)
    out = pl.resample(arrays)
    assert list(out) == list(arrays)
    for name, (a, fill, width) in host.items():
        t = out[name]
        assert t.shape[0] == pl.n_out and tuple(t.shape[1:]) == tuple(arrays[name][0].shape[1:]) and t.dtype == arrays[name][0].dtype
        assert t.cpu().numpy().reshape(pl.n_out, width).tobytes() == expected(a, src, kind, fill, width).tobytes(), name
    one_d = torch.arange(pl.n, dtype=torch.float32, device=dev)
    assert pl.resample({"x": (one_d, "copy")})["x"].cpu().numpy().tobytes() == src.astype(F32).tobytes()
    assert int(pl.status.item()) == 0


def test_rows_beyond_the_capped_grid():
    """vp_densify_rows gives an array min(ceil(n_out / rows per round), DENSIFY_MAX_BLOCKS = 65 536) workgroups, and a
    workgroup moves (256 / lanes per row) * DENSIFY_ROWS_IN_FLIGHT = 4 rows per round.  A row of 45 words is not a multiple of
    four words, so it moves word by word with 64 lanes: 4 * 4 = 16 rows per round, and a second round iff
    n_out > 65 536 * 16 = 1 048 576.  n_out = 1 048 576 + 16 + 3: workgroup 0 has a full second round, workgroup 1 three rows
    of one.  The 3-word array of the same launch (4 lanes, 256 rows per round, 4097 workgroups) stays below its cap.  The rows
    of the second round name sources that no other row names; everything is built and compared on the device."""
    import voxproj_host
    dev = torch.device("cuda:0")
    lap = 65536 * 16
    n_src, n_out, wide, narrow = 600000, lap + 16 + 3, 45, 3          # the library takes n_out <= 2 n_src
    gen = torch.Generator(device=dev).manual_seed(45)
    src = torch.randint(0, n_src - 19, (n_out,), generator=gen, device=dev, dtype=torch.int32)
    src[lap:] = torch.arange(n_src - 19, n_src, dtype=torch.int32, device=dev).flip(0)
    kind = torch.randint(0, 4, (n_out,), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
    kind[lap:] = torch.arange(19, device=dev).to(torch.uint8) % 4
    counts = torch.tensor([n_out] + [int((kind == v).sum()) for v in (0, 1, 2)], dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    a_copy = torch.randint(-2 ** 31, 2 ** 31 - 1, (n_src, wide), generator=gen, device=dev, dtype=torch.int64).to(torch.int32)
    a_zero = torch.randn((n_src, wide), generator=gen, device=dev)
    a_thin = torch.randint(-2 ** 31, 2 ** 31 - 1, (n_src, narrow), generator=gen, device=dev, dtype=torch.int64).to(torch.int32)
    d_copy = torch.full((n_out, wide), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_zero = torch.full((n_out, wide), -7.25, device=dev)
    d_thin = torch.full((n_out, narrow), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    voxproj_host.densify_rows([(a_copy, d_copy, "copy"), (a_zero, d_zero, "zero"), (a_thin, d_thin, "zero")], src, kind, counts,
                              n_src, n_out, status)
    idx, fresh = src.long(), (kind != 0)[:, None]
    assert int(status.item()) == 0
    assert torch.equal(d_copy, a_copy.index_select(0, idx))
    assert torch.equal(d_thin, torch.where(fresh, torch.zeros_like(d_thin), a_thin.index_select(0, idx)))
    want = torch.where(fresh, torch.zeros_like(d_zero), a_zero.index_select(0, idx))
    assert torch.equal(d_zero.view(torch.int32), want.view(torch.int32))
    assert bool(fresh[lap:].any()) and not bool(fresh[lap:].all()) and int(src[:lap].max()) < n_src - 19
    del d_copy, d_zero, d_thin, a_copy, a_zero, a_thin, want, idx, src, kind
    torch.cuda.empty_cache()


def test_wrong_n_out_raises_the_status_and_writes_nothing(plan):
    import voxproj_host
    pl, src, kind = plan
    dev = pl.src.device
    a = torch.randn(pl.n, 16, device=dev)
    for wrong in (pl.n_out - 1, pl.n_out + 1):
        dst = torch.full((wrong, 16), 123.0, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        voxproj_host.densify_rows([(a, dst, "copy")], pl.src, pl.kind, pl.counts, pl.n, wrong, status)
        assert int(status.item()) == 1 and bool((dst == 123.0).all())
        om = torch.full((wrong, 3), 123.0, device=dev)
        ol = torch.full((wrong, 3), 123.0, device=dev)
        status.zero_()
        L = voxproj_host._densify_lib()
        g = torch.randn(pl.n, 4, device=dev)
        rc = L.vp_densify_split(g.data_ptr(), g.data_ptr(), g.data_ptr(), pl.n, pl.src.data_ptr(), pl.kind.data_ptr(),
                                pl.counts.data_ptr(), wrong, 1, om.data_ptr(), ol.data_ptr(), status.data_ptr(),
                                torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0 and int(status.item()) == 1 and bool((om == 123.0).all()) and bool((ol == 123.0).all())
    with pytest.raises(ValueError):
        voxproj_host.densify_rows([(a, torch.empty(pl.n_out, 8, device=dev), "copy")], pl.src, pl.kind, pl.counts, pl.n,
                                  pl.n_out)
    with pytest.raises(ValueError):
        pl.resample({"x": (a[:10], "copy")})
    with pytest.raises(ValueError):
        pl.resample({"x": (a.double(), "copy")})


def test_resample_adam(plan):
    import voxproj_host
    pl, src, kind = plan
    dev = pl.src.device
    gen = torch.Generator(device="cpu").manual_seed(3)
    p = {"a": torch.nn.Parameter(torch.randn(pl.n, 3, generator=gen).to(dev)),
         "b": torch.nn.Parameter(torch.randn(pl.n, generator=gen).to(dev))}
    other = torch.nn.Parameter(torch.randn(5, generator=gen).to(dev))
    opt = torch.optim.Adam([dict(params=[p["a"]], lr=0.01), dict(params=[p["b"], other], lr=0.02)])
    for _ in range(3):
        opt.zero_grad()
        (p["a"].square().sum() + p["b"].sin().sum() + other.sum()).backward()
        opt.step()
    before = {k: (v.detach().cpu().numpy().copy(), opt.state[v]["exp_avg"].cpu().numpy().copy(),
                  opt.state[v]["exp_avg_sq"].cpu().numpy().copy(), float(opt.state[v]["step"])) for k, v in p.items()}
    moved = pl.resample({k: (v, "copy") for k, v in p.items()})
    new = {k: torch.nn.Parameter(v) for k, v in moved.items()}
    voxproj_host.resample_adam(opt, p, new, pl)
    assert opt.param_groups[0]["params"][0] is new["a"] and opt.param_groups[1]["params"][0] is new["b"]
    assert opt.param_groups[1]["params"][1] is other and other in opt.state and len(opt.state) == 3
    fresh = kind != 0
    for k, (val, m1, m2, step) in before.items():
        st = opt.state[new[k]]
        assert float(st["step"]) == step == 3.0
        assert new[k].detach().cpu().numpy().tobytes() == val[src].tobytes()
        g1, g2 = st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy()
        assert g1[~fresh].tobytes() == m1[src][~fresh].tobytes() and g2[~fresh].tobytes() == m2[src][~fresh].tobytes()
        assert not g1[fresh].any() and not g2[fresh].any() and fresh.any()
        assert p[k] not in opt.state
    opt.zero_grad()
    (new["a"].square().sum() + new["b"].sin().sum() + other.sum()).backward()
    opt.step()
    assert all(float(opt.state[v]["step"]) == 4.0 and torch.isfinite(v).all() for v in new.values())
    assert new["a"].detach().cpu().numpy().tobytes() != before["a"][0][src].tobytes()


def test_split_geometry(plan):
    pl, src, kind = plan
    dev = pl.src.device
    rng = np.random.default_rng(8)
    means = rng.normal(0, 2.0, (pl.n, 3)).astype(F32)
    quats = rng.normal(size=(pl.n, 4)).astype(F32)
    quats[::7] *= 5.0                                            # any norm: the split normalises
    ls = rng.normal(-3.0, 0.7, (pl.n, 3)).astype(F32)
    t = [torch.from_numpy(v).to(dev) for v in (means, quats, ls)]
    seed = (9 << 32) | 4
    om, ol = (v.cpu().numpy() for v in pl.split_geometry(*t, seed))
    em, el, bound = dr.split_geometry(means, quats, ls, src, kind, seed)
    copy, child = kind < 2, kind >= 2
    assert om[copy].tobytes() == em[copy].tobytes() and ol[copy].tobytes() == el[copy].tobytes()
    assert ol[child].tobytes() == el[child].tobytes()           # one fp32 addition: exact
    err = np.abs(om[child].astype(np.float64) - em[child].astype(np.float64))
    tol = 2.0 ** -22 * bound[child]
    print(f"split means: max error / bound = {(err / bound[child]).max():.3e} (allowed {2.0 ** -22:.3e})", flush=True)
    assert (err <= tol).all()
    assert (om[child] != means[src[child]]).any(axis=1).all()   # every child moved
    again, again_l = (v.cpu().numpy() for v in pl.split_geometry(*t, (4, 9)))     # the same seed as (low, high) words
    assert again.tobytes() == om.tobytes() and again_l.tobytes() == ol.tobytes()
    other = pl.split_geometry(*t, seed + 1)[0].cpu().numpy()
    assert other[copy].tobytes() == om[copy].tobytes() and (other[child] != om[child]).any(axis=1).all()
    two = kind == 2
    assert (om[two] != om[kind == 3]).any(axis=1).all()          # the two children of a source differ
