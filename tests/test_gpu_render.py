"""GPU tests of the projector's transpose: vp_first_hit_ids (the march alone) against the oracle's first-hit image and against
what a forward call leaves; vp_render_features (dst[p] = rows[hit[p]]) bit for bit, fp32 and fp16, any C, beyond 2^31
elements, with out-of-range IDs; the autograd Function's gradients and the adjoint identity; render_voxel_features.py end to
end on files."""
import json

import numpy as np
import pytest
import torch

from synthetic_scene import make_scene

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _oracle_hits(oracle_mod, occ_b, vmi, intr_b, opts, origin, vs, B, V, H, W, n_rows):
    count = np.zeros(n_rows, np.int32)
    out = np.zeros((n_rows, 1), np.float32)
    r = oracle_mod.project_features(np.zeros((B, V, H, W, 1), np.float32), occ_b, vmi.reshape(-1), intr_b, opts, origin, vs,
                                    count, out)
    return r["hits"]


def _scene_args(s, views, B=1):
    """occ int64 [B,Z,Y,X] (the scene's grid in every batch), vmi [B*V*16] (batch b takes the views rolled by b), intr [B,4]."""
    V = len(views)
    occ = np.repeat(s.occ.astype(np.int64)[None], B, axis=0)
    vmi = np.concatenate([s.c2w[np.roll(np.asarray(views), b)].reshape(-1) for b in range(B)]).astype(np.float32)
    intr = np.repeat(s.intr[None].astype(np.float32), B, axis=0)
    return occ, vmi, intr, V


@pytest.mark.parametrize("case", ["room_b1", "room_b2", "one_view", "trajectory_close_up", "trajectory_one_view"])
@pytest.mark.parametrize("exact", [False, True])
def test_first_hit_ids_equal_the_oracle_and_the_forward_calls_hit_image(oracle_mod, case, exact):
    import voxproj_host as vh
    # "one_view" cases: B*V == 1, the one-view plan of plan_split (vp_plan.h) -- the path render_voxel_features.py takes for every view
    if case.startswith("trajectory"):
        s = make_scene(6000, 40, 80, 60, seed=4, trajectory=True)
        views, B = ([0] if case == "trajectory_one_view" else [0, 1, 2]), 1    # the first frames of the path: its first close-up dwell
    else:
        s = make_scene(2500, 5, 64, 48, seed=11, room=(5.0, 4.0, 2.4))
        views, B = ([3] if case == "one_view" else [0, 2, 3, 4]), (2 if case == "room_b2" else 1)
    occ, vmi, intr, V = _scene_args(s, views, B)
    H, W, n_rows = s.height, s.width, s.n_vox + 1
    want = _oracle_hits(oracle_mod, occ, vmi, intr, s.opts(), s.grid_origin, s.voxel_size, B, V, H, W, n_rows)
    occ_t, vmi_t, intr_t = (torch.from_numpy(a).to(DEV) for a in (occ, vmi, intr))
    ws = vh.Workspace()
    ids = vh.first_hit_ids(occ_t, vmi_t, intr_t, s.opts(), s.grid_origin, s.voxel_size, H, W, n_rows, workspace=ws, exact_march=exact)
    assert ids.dtype == torch.int32 and tuple(ids.shape) == (B, V, H, W)
    assert np.array_equal(ids.cpu().numpy(), want)
    assert (want > 0).mean() > 0.3
    # again with the tables the first call built (VP_FLAG_REUSE_ACCEL: same occ tensor)
    builds = vh.table_builds(ws)
    again = vh.first_hit_ids(occ_t, vmi_t, intr_t, s.opts(), s.grid_origin, s.voxel_size, H, W, n_rows, workspace=ws, exact_march=exact)
    assert vh.table_builds(ws) == builds and torch.equal(again, ids)
    # a forward call with the same arguments leaves the same image
    C = 8
    feats = torch.randn(B, V, H, W, C, device=DEV)
    count, out = torch.zeros(n_rows, dtype=torch.int32, device=DEV), torch.zeros(n_rows, C, device=DEV)
    vh.project_features_raw(feats, occ_t, vmi_t, intr_t, s.opts(), count, out, s.grid_origin, s.voxel_size, workspace=ws,
                            exact_march=exact)
    assert torch.equal(vh.hit_image(ws, DEV), ids)
    # vp_first_hit_ids counts as a call: nothing is left for a gather-only call or vp_copy_hit_image
    vh.first_hit_ids(occ_t, vmi_t, intr_t, s.opts(), s.grid_origin, s.voxel_size, H, W, n_rows, workspace=ws, exact_march=exact)
    ws.set_row_range(n_rows // 2, None)
    try:
        with pytest.raises(vh.VoxprojError, match="error -1"):
            vh.project_features_raw(feats, occ_t, vmi_t, intr_t, s.opts(), count, out, s.grid_origin, s.voxel_size, workspace=ws,
                                    gather_only=True)
    finally:
        ws.set_row_range()
    with pytest.raises(vh.VoxprojError, match="error -1"):
        vh.hit_image(ws, DEV)
    ws.release()


def _special_rows(n_rows, C, seed):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n_rows, C)).astype(np.float32)
    flat = rows.reshape(-1)
    k = max(1, flat.size // 50)
    pick = rng.choice(flat.size, size=min(flat.size, 6 * k), replace=False)
    specials = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, 3e-6, 7e4, -1e-45], np.float32)   # f32 denormals, f16 subnormal / overflow
    flat[pick] = specials[np.arange(pick.size) % specials.size]
    return rows


def _same_f16(a, b):
    """Bit-equal float16 arrays, any NaN matching any NaN."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint16)[~na], b.view(np.uint16)[~nb])


@pytest.fixture(scope="module")
def scene_hits(oracle_mod):
    s = make_scene(3000, 4, 72, 40, seed=7, room=(5.0, 4.0, 2.4))
    occ, vmi, intr, V = _scene_args(s, [0, 1, 2])
    hits = _oracle_hits(oracle_mod, occ, vmi, intr, s.opts(), s.grid_origin, s.voxel_size, 1, V, s.height, s.width, s.n_vox + 1)
    return hits, s.n_vox + 1


@pytest.mark.parametrize("C", [1, 3, 4, 8, 12, 16, 64, 67, 512])
def test_render_features_copies_the_hit_rows_bit_for_bit(scene_hits, C):
    import voxproj_host as vh
    hits, n_rows = scene_hits
    rows = _special_rows(n_rows, C, seed=C)
    want = np.where((hits > 0)[..., None], rows[hits], np.float32(0))
    ids_t, rows_t = torch.from_numpy(hits).to(DEV), torch.from_numpy(rows).to(DEV)
    got = vh.render_features(ids_t, rows_t)
    assert got.dtype == torch.float32 and tuple(got.shape) == hits.shape + (C,)
    assert got.cpu().numpy().tobytes() == want.tobytes()
    got16 = vh.render_features(ids_t, rows_t, dtype=torch.float16).cpu().numpy()
    with np.errstate(over="ignore"):                     # 7e4 rounds to inf in float16, as it should
        assert _same_f16(got16, want.astype(np.float16))
    # a destination that is not 16-byte aligned takes the scalar path, to the same bits
    buf = torch.empty(hits.size * C + 1, dtype=torch.float32, device=DEV)
    out = buf[1:].view(hits.shape + (C,))
    vh.render_features(ids_t, rows_t, out=out)
    assert out.cpu().numpy().tobytes() == want.tobytes()
    # a pixel count that is not a multiple of 64 (the last tile is partial)
    n = hits.size - 37
    part = vh.render_features(ids_t.reshape(-1)[:n], rows_t)
    assert part.cpu().numpy().tobytes() == want.reshape(-1, C)[:n].tobytes()


def test_render_features_beyond_2_31_elements_equals_a_chunked_torch_gather():
    # 8 views of 968x548 pixels x 512 channels: 2.17e9 elements (8.7 GB) in one call, 64-bit offsets throughout
    import voxproj_host as vh
    n_pix, C, n_rows = 8 * 968 * 548, 512, 200001
    assert n_pix * C > 2 ** 31
    g = torch.Generator(device=DEV).manual_seed(3)
    runs = torch.randint(0, n_rows, (n_pix // 12 + 1,), device=DEV, dtype=torch.int32, generator=g)
    ids = runs.repeat_interleave(12)[:n_pix].contiguous()            # runs of one voxel, as along an image row
    ids[torch.randint(0, n_pix, (n_pix // 10,), device=DEV, generator=g)] = 0
    rows = torch.randn(n_rows, C, device=DEV, generator=g)
    dst = vh.render_features(ids.view(8, 548, 968), rows)
    flat = dst.view(n_pix, C)
    step = 1 << 20
    for p0 in range(0, n_pix, step):
        i = ids[p0:p0 + step].long()
        ref = torch.where((i > 0)[:, None], rows[i], torch.zeros((), device=DEV))
        assert torch.equal(flat[p0:p0 + step].view(torch.int32), ref.view(torch.int32)), p0
    del dst, flat


def test_out_of_range_ids_render_zeros_and_are_counted():
    import ctypes

    import voxproj_host as vh
    n_rows, C = 50, 64
    ids = torch.randint(1, n_rows, (3, 100), dtype=torch.int32, device=DEV)
    ids[0, 5] = -1
    ids[1, 7] = n_rows
    ids[2, 99] = -(2 ** 31)
    ids[2, 0] = 0
    rows = torch.randn(n_rows, C, device=DEV)
    for f16 in (0, 1):
        dst = torch.full((3, 100, C), 7.0, dtype=torch.float16 if f16 else torch.float32, device=DEV)
        bad = torch.zeros(1, dtype=torch.int32, device=DEV)
        vh.check(vh.lib().vp_render_features(ids.data_ptr(), ids.numel(), rows.data_ptr(), n_rows, C, dst.data_ptr(), f16,
                                             bad.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
        torch.cuda.synchronize()
        assert int(bad.item()) == 3
        zero = (ids < 1) | (ids >= n_rows)
        assert bool((dst[zero] == 0).all())
        ok = ~zero
        assert torch.equal(dst[ok].float(), rows[ids[ok].long()].to(dst.dtype).float())
    with pytest.raises(vh.VoxprojError, match="3 pixel"):
        vh.render_features(ids, rows, check=True)
    assert vh.render_features(ids, rows, check=False).shape == (3, 100, C)


def _autograd_scene():
    s = make_scene(2000, 4, 48, 32, seed=21, room=(5.0, 4.0, 2.4))
    occ, vmi, intr, V = _scene_args(s, [0, 1, 2, 3])
    return s, torch.from_numpy(occ).to(DEV), torch.from_numpy(vmi).to(DEV), torch.from_numpy(intr).to(DEV), V


@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_autograd_gradient_is_the_render_of_the_upstream_gradient(reduce, dtype):
    import project_features_autograd as pfa
    import voxproj_host as vh
    s, occ, vmi, intr, V = _autograd_scene()
    C, n_rows = 16, s.n_vox + 1
    feats = torch.randn(1, V, s.height, s.width, C, device=DEV).to(dtype).requires_grad_(True)
    out, count = pfa.project_features(feats, occ, vmi, intr, s.opts(), s.grid_origin, s.voxel_size, n_rows, reduce=reduce)
    assert out.dtype == torch.float32 and count.dtype == torch.int32 and not count.requires_grad and out.requires_grad
    # forward = the library's forward call
    c_ref, o_ref = torch.zeros(n_rows, dtype=torch.int32, device=DEV), torch.zeros(n_rows, C, device=DEV)
    vh.project_features_raw(feats.detach().contiguous(), occ, vmi, intr, s.opts(), c_ref, o_ref, s.grid_origin, s.voxel_size,
                            workspace=vh.Workspace())
    if reduce == "mean":
        o_ref = o_ref / c_ref.clamp(min=1)[:, None].float()
    assert torch.equal(count, c_ref) and torch.equal(out, o_ref)
    g = torch.randn(n_rows, C, device=DEV)
    (grad,) = torch.autograd.grad(out, feats, g, retain_graph=True)
    assert grad.dtype == dtype and grad.shape == feats.shape
    ids = vh.first_hit_ids(occ, vmi, intr, s.opts(), s.grid_origin, s.voxel_size, s.height, s.width, n_rows, workspace=vh.Workspace())
    gs = g / count.clamp(min=1)[:, None].float() if reduce == "mean" else g
    want = vh.render_features(ids, gs, dtype=dtype)
    assert torch.equal(grad.view(torch.int16 if dtype == torch.float16 else torch.int32),
                       want.view(torch.int16 if dtype == torch.float16 else torch.int32))
    # a loss through the output reaches the maps
    feats.grad = None
    (out * g).sum().backward()
    assert torch.equal(feats.grad, grad)


def test_adjoint_identity_in_float64():
    # <P f, g> = <f, P^T g> for a multi-view call on the default (split-voxel) path
    import project_features_autograd as pfa
    import voxproj_host as vh
    s = make_scene(2000, 6, 96, 64, seed=5, room=(5.0, 4.0, 2.4))
    occ, vmi, intr, V = _scene_args(s, [0, 1, 2, 3, 4, 5])
    occ, vmi, intr = (torch.from_numpy(a).to(DEV) for a in (occ, vmi, intr))
    C, n_rows = 32, s.n_vox + 1
    gen = torch.Generator(device=DEV).manual_seed(9)
    f = torch.rand(1, V, s.height, s.width, C, device=DEV, generator=gen) + 0.5
    g = torch.rand(n_rows, C, device=DEV, generator=gen) + 0.5
    out, count = pfa.project_features(f, occ, vmi, intr, s.opts(), s.grid_origin, s.voxel_size, n_rows)
    assert int(count.sum()) > 0.3 * V * s.height * s.width
    ids = vh.first_hit_ids(occ, vmi, intr, s.opts(), s.grid_origin, s.voxel_size, s.height, s.width, n_rows)
    lhs = (out.double() * g.double()).sum().item()
    rhs = (f.double() * vh.render_features(ids, g).double()).sum().item()
    assert abs(lhs - rhs) <= 1e-6 * abs(rhs)


def _write_files(tmp_path, n_views=4, C=16):
    """A voxel-grid PLY with the header comments the aggregator reads, a camera JSON and fp16 LSeg-layout maps [C,h,w]."""
    s = make_scene(1500, n_views, 48, 32, seed=33, room=(5.0, 4.0, 2.4))
    ply = tmp_path / f"grid_{s.n_vox}vox.ply"
    with open(ply, "w") as f:
        f.write("ply\nformat ascii 1.0\n")
        f.write(f"comment voxel_size {s.voxel_size!r}\ncomment grid_origin {float(s.grid_origin[0])!r} "
                f"{float(s.grid_origin[1])!r} {float(s.grid_origin[2])!r}\n")
        f.write(f"element vertex {s.n_vox}\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
        for q in s.points:
            f.write(f"{float(q[0])!r} {float(q[1])!r} {float(q[2])!r}\n")
    lseg = tmp_path / "lseg"
    lseg.mkdir()
    rng = np.random.default_rng(33)
    images = {}
    for v in range(n_views):
        name = f"IMG{v:04d}"
        np.save(lseg / f"{name}.npy", rng.standard_normal((C, 32, 48)).astype(np.float16))
        c2w = s.c2w[v].astype(np.float64)
        R = c2w[:3, :3].T                       # the camera file holds world->camera [R|t]
        images[str(v)] = {"name": name, "camera_id": 1, "R": R.tolist(), "tvec": (-R @ c2w[:3, 3]).tolist()}
    # the scripts scale the intrinsics by --downsample_factor 0.5: the file holds the double-resolution camera
    cams = {"1": {"params": [float(x) * 2 for x in s.intr], "width": 96, "height": 64}}
    cam_json = tmp_path / "cams.json"
    cam_json.write_text(json.dumps({"images": images, "cameras": cams}))
    return s, ply, lseg, cam_json


def test_render_script_end_to_end_on_an_aggregation_result(tmp_path):
    import aggregate_voxel_features_onthefly as agg
    import build_sparse_occupancy as bso
    import prepare_tensor_data as ptd
    import render_voxel_features
    import voxproj_host as vh
    s, ply, lseg, cam_json = _write_files(tmp_path)
    agg.main(["--mode", "fast", "--lseg_dir", str(lseg), "--cam_params", str(cam_json), "--voxel_ply", str(ply),
              "--checkpoint_dir", str(tmp_path / "agg")])
    pt = tmp_path / "agg" / f"ALL_nonzero_voxel_features_4_vox{s.n_vox}.pt"
    out_dir = tmp_path / "views"
    render_voxel_features.main(["--features_pt", str(pt), "--voxel_ply", str(ply), "--cam_params", str(cam_json),
                                "--views", "IMG0001", "IMG0003", "--out_dir", str(out_dir), "--save_ids"])
    d = torch.load(pt)
    vs, origin, _, _ = bso.extract_voxel_params(str(ply))
    occ3 = bso.build_occupancy(bso.read_voxel_ply(str(ply)), origin, vs, device=DEV)
    n_rows = int(occ3.max()) + 1
    zyx = d["voxel_coords"].long().to(DEV)
    table = torch.zeros(n_rows, d["avg_feats"].shape[1], device=DEV)
    table[occ3[zyx[:, 0], zyx[:, 1], zyx[:, 2]].long()] = d["avg_feats"].float().to(DEV)
    by_name, cams = ptd.load_camera_params(str(cam_json))
    for name in ("IMG0001", "IMG0003"):
        intr, c2w = ptd.camera_for(by_name[name], cams, 0.5)
        ids = vh.first_hit_ids(occ3[None].long().contiguous(), c2w.reshape(-1).to(DEV), intr.reshape(1, 4).to(DEV),
                               agg.ray_opts(48, 32, vs), origin, vs, 32, 48, n_rows)[0, 0]
        assert np.array_equal(np.load(out_dir / f"{name}_ids.npy"), ids.cpu().numpy())
        img = np.load(out_dir / f"{name}_fused.npy")
        want = torch.where((ids > 0)[..., None], table[ids.long()], torch.zeros((), device=DEV)).half().permute(2, 0, 1)
        assert img.dtype == np.float16 and img.shape == (16, 32, 48)
        assert img.tobytes() == want.contiguous().cpu().numpy().tobytes()
        assert (ids > 0).float().mean() > 0.3 and np.abs(img.astype(np.float32)).sum() > 0
