"""GPU parity tests proper: the HIP path (through project_features_cuda -> C-ABI) against the CPU
oracle on the same seeded inputs.  Bar: first-hit voxel IDs and hit counts bit-exact; feature sums
within 1e-4 relative (they are in fact bit-identical while a voxel's pixels are summed by one
wavefront in (view, y, x) order, which these tests also assert)."""
import numpy as np
import pytest
import torch

from synthetic_scene import make_features_np, make_scene

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _no_heavy_path_by_default(heavy_threshold):
    # the bit-identical-sums assertions hold for voxels summed by ONE wavefront; keep the split-voxel path
    # (different, fixed summation tree) out of those tests.  test_heavy_voxels_* lowers it again.
    heavy_threshold(100000000)


FRONT = {"name": "compiled"}


@pytest.fixture(autouse=True, params=["compiled", "python"])
def _front(request):
    # every test runs through both fronts of the drop-in module: the compiled pybind11 wrapper
    # (csrc/project_features_ext.cpp) and the ctypes one; both end in the same C-ABI call
    if request.param == "compiled":
        import project_features_cuda as m      # ModuleNotFoundError = not built: run __graft_entry__.build()
        assert m.__file__.endswith(".so")
    FRONT["name"] = request.param
    yield request.param


def _drop_in():
    if FRONT["name"] == "compiled":
        import project_features_cuda as m
        return m.project_features_cuda
    import project_features_front
    return project_features_front.project_features_cuda_py


def _last_ws():
    import project_features_front
    return project_features_front.last_workspace(torch.device(DEV), front=FRONT["name"])


def _gpu_call(feats, occ, c2w, intr, opts, origin, vs, count_t, out_t):
    B = feats.shape[0]
    _drop_in()(
        torch.from_numpy(feats).to(DEV).contiguous(),
        torch.from_numpy(occ.astype(np.int64)).to(DEV).contiguous(),
        torch.from_numpy(np.ascontiguousarray(c2w, np.float32)).reshape(-1).to(DEV),
        torch.from_numpy(np.ascontiguousarray(intr, np.float32)).reshape(B, 4).to(DEV),
        torch.from_numpy(np.asarray(opts, np.float32)), count_t, out_t,
        torch.tensor([False]), torch.from_numpy(np.asarray(origin, np.float32)), float(vs))


def _compare(oracle_mod, feats, occ, c2w, intr, opts, origin, vs, n_rows, expect_boxmiss=False, bitwise=True):
    import voxproj_host
    B, V, H, W, C = feats.shape
    count = np.zeros(n_rows, np.int32)
    out = np.zeros((n_rows, C), np.float32)
    r = oracle_mod.project_features(feats, occ.astype(np.int64), np.asarray(c2w, np.float32).reshape(-1),
                                    np.asarray(intr, np.float32).reshape(B, 4), opts, origin, vs, count, out,
                                    want_f64=True)
    assert r["rc"] == 0
    count_t = torch.zeros(n_rows, dtype=torch.int32, device=DEV)
    out_t = torch.zeros(n_rows, C, dtype=torch.float32, device=DEV)
    _gpu_call(feats, occ, c2w, intr, opts, origin, vs, count_t, out_t)
    ws = _last_ws()
    hits = voxproj_host.hit_image(ws, torch.device(DEV)).cpu().numpy()
    ctr = voxproj_host.counters(ws, torch.device(DEV))
    assert np.array_equal(hits, r["hits"]), f"first-hit IDs differ at {(hits != r['hits']).sum()} pixels"
    assert np.array_equal(count_t.cpu().numpy(), count)
    got = out_t.cpu().numpy()
    scale = np.abs(r["out64"]).max(axis=1, keepdims=True) + 1e-30
    assert (np.abs(got - r["out64"]) / scale).max() <= 1e-4        # tolerance of north_star: 1e-4 relative, of each ROW's magnitude
    if bitwise:
        assert got.tobytes() == out.tobytes()
    assert ctr["bad_id"] == 0
    if expect_boxmiss is not None:
        assert (ctr["box_miss"] > 0) == expect_boxmiss, ctr
    return r, got, count


def _scene_case(oracle_mod, n_vox, V, W, H, C, seed, room=(5.0, 4.0, 2.4)):
    s = make_scene(n_vox, V, W, H, seed=seed, room=room)
    feats = make_features_np(V, H, W, C, seed=seed)[None]
    r, got, count = _compare(oracle_mod, feats, s.occ[None], s.c2w, s.intr, s.opts(), s.grid_origin,
                             s.voxel_size, s.n_vox + 1)
    assert (r["hits"] > 0).mean() > 0.9
    return s, r, got, count


def test_s1_fixture_shape(oracle_mod):           # 8 views x 2k voxels x 48x32x16
    _scene_case(oracle_mod, 2000, 8, 48, 32, 16, seed=11)


def test_s0_plumbing_shape(oracle_mod):          # BASELINE config 1: 8 cams x 10k voxels x 64x64x32
    _scene_case(oracle_mod, 10000, 8, 64, 64, 32, seed=12, room=(10.0, 8.0, 3.2))


def test_c512_rows(oracle_mod):                  # the production row width (two 1-KiB loads per row)
    _scene_case(oracle_mod, 5000, 3, 96, 64, 512, seed=13)


@pytest.mark.parametrize("C", [1, 3, 7, 20, 260, 1000])
def test_ragged_channel_counts(oracle_mod, C):
    _scene_case(oracle_mod, 2000, 2, 40, 24, C, seed=14 + C)


def test_many_views_per_call(oracle_mod):        # V > 64 (more than one lane-batch of views), V > 16
    _scene_case(oracle_mod, 2000, 70, 24, 16, 8, seed=15)


def test_batch_of_two_grids(oracle_mod):
    s = make_scene(2000, 4, 40, 24, seed=16, room=(5.0, 4.0, 2.4))
    s2 = make_scene(2000, 4, 40, 24, seed=17, room=(5.0, 4.0, 2.4))
    assert s.occ.shape == s2.occ.shape
    feats = make_features_np(4, 24, 40, 12, seed=16).reshape(2, 2, 24, 40, 12)
    occ = np.stack([s.occ, s2.occ])
    intr = np.stack([s.intr, s.intr * np.float32(1.1)])
    _compare(oracle_mod, feats, occ, s.c2w, intr, s.opts(), s.grid_origin, s.voxel_size, s.n_vox + 1)
    # three batches whose per-batch tables need padding (block count not a multiple of 16) and whose later
    # batches are sparse: a distance field attached to the wrong batch offset would leap over isolated voxels
    rng = np.random.default_rng(18)
    sparse = []
    for k in range(2):
        o = np.zeros_like(s.occ)
        idx = rng.choice(o.size, 60, replace=False)
        o.reshape(-1)[idx] = rng.integers(1, s.n_vox, 60)
        sparse.append(o)
    occ3 = np.stack([s.occ, sparse[0], sparse[1]])
    feats3 = make_features_np(6, 24, 40, 4, seed=19).reshape(3, 2, 24, 40, 4)
    c2w3 = np.concatenate([s.c2w[:2], s.c2w[:2], s.c2w[2:4]])
    intr3 = np.stack([s.intr, s.intr, s.intr])
    r, _, _ = _compare(oracle_mod, feats3, occ3, c2w3, intr3, s.opts(), s.grid_origin, s.voxel_size, s.n_vox + 1,
                       expect_boxmiss=None)
    assert (r["hits"][1:] > 0).sum() > 20


def test_sparse_grid_with_misses(oracle_mod):
    rng = np.random.default_rng(5)
    occ = np.zeros((12, 20, 24), np.int32)
    idx = rng.choice(occ.size, 300, replace=False)
    occ.reshape(-1)[idx] = np.arange(1, 301)
    s = make_scene(2000, 3, 40, 24, seed=6, room=(5.0, 4.0, 2.4))
    feats = make_features_np(3, 24, 40, 16, seed=7)[None]
    opts = np.array([40, 24, 0.01, 10.0, 0.11], np.float32)
    r, _, _ = _compare(oracle_mod, feats, occ[None], s.c2w, s.intr, opts, np.array([-2.1, -1.7, 0.05], np.float32),
                       0.2, 301)
    assert 0.02 < (r["hits"] > 0).mean() < 0.98


def test_kat_walls_on_gpu(oracle_mod):
    Z, Y, X = 8, 17, 17
    occ = np.zeros((1, Z, Y, X), np.int64)
    occ[0, 3] = 1 + (np.arange(Y)[:, None]) * X + np.arange(X)[None, :]
    occ[0, 6] = 1 + (Y + np.arange(Y)[:, None]) * X + np.arange(X)[None, :]
    feats = np.random.default_rng(3).standard_normal((1, 1, 8, 8, 4)).astype(np.float32)
    opts = np.array([8, 8, 0.01, 10.0, 0.25], np.float32)
    r, got, count = _compare(oracle_mod, feats, occ, np.eye(4, dtype=np.float32)[None], np.array([4, 4, 4, 4], np.float32),
                             opts, np.array([-8, -8, 0], np.float32), 1.0, 2 * Y * X + 1)
    assert r["hits"][0, 0, 4, 4] == 1 + 8 * 17 + 8          # K2: only the first wall is hit
    assert count[Y * X + 1:].sum() == 0


def test_accumulates_across_calls_like_the_reference(oracle_mod):
    # Q13: outputs are += ; AGG calls once per view.  8 single-view calls == the oracle called the same way.
    s = make_scene(2000, 8, 48, 32, seed=21, room=(5.0, 4.0, 2.4))
    C = 16
    feats = make_features_np(8, 32, 48, C, seed=21)
    n_rows = s.n_vox + 1
    count = np.zeros(n_rows, np.int32)
    out = np.zeros((n_rows, C), np.float32)
    count_t = torch.zeros(n_rows, dtype=torch.int32, device=DEV)
    out_t = torch.zeros(n_rows, C, device=DEV)
    for v in range(8):
        oracle_mod.project_features(feats[None, v:v + 1], s.occ[None].astype(np.int64), s.c2w[v].reshape(-1),
                                    s.intr[None], s.opts(), s.grid_origin, s.voxel_size, count, out)
        _gpu_call(feats[None, v:v + 1], s.occ[None], s.c2w[v:v + 1], s.intr, s.opts(), s.grid_origin,
                  s.voxel_size, count_t, out_t)
    assert np.array_equal(count_t.cpu().numpy(), count)
    assert out_t.cpu().numpy().tobytes() == out.tobytes()
    # and a miss leaves nonzero outputs untouched (K3)
    before = out_t.clone()
    empty = np.zeros_like(s.occ)[None]
    _gpu_call(feats[None, :1], empty, s.c2w[:1], s.intr, s.opts(), s.grid_origin, s.voxel_size, count_t, out_t)
    assert torch.equal(before, out_t)


def test_id_labelling_several_cells_falls_back_to_full_scan(oracle_mod):
    # generic grids may reuse an ID for many cells; the search boxes then miss pixels and the voxel is
    # rescanned over whole images -- results must still be exact.
    s = make_scene(2000, 2, 40, 24, seed=22, room=(5.0, 4.0, 2.4))
    occ = np.where(s.occ > 0, (s.occ % 7) + 1, 0).astype(np.int32)
    feats = make_features_np(2, 24, 40, 8, seed=22)[None]
    _compare(oracle_mod, feats, occ[None], s.c2w, s.intr, s.opts(), s.grid_origin, s.voxel_size, 9,
             expect_boxmiss=True)


def test_heavy_voxels_use_the_workgroup_path(oracle_mod, heavy_threshold):
    # voxels that collect more than VP_OPT_HEAVY_THRESHOLD pixels in a call are summed by a whole workgroup with a
    # fixed summation tree: IDs/counts stay exact, sums within 1e-4 (not bit-identical to the serial order),
    # and two runs agree bit for bit.
    import voxproj_host
    heavy_threshold(6)
    s = make_scene(2000, 5, 48, 32, seed=31, room=(5.0, 4.0, 2.4))
    for C in (16, 512, 7):
        feats = make_features_np(5, 32, 48, C, seed=31)[None]
        r, got, _ = _compare(oracle_mod, feats, s.occ[None], s.c2w, s.intr, s.opts(), s.grid_origin, s.voxel_size,
                             s.n_vox + 1, bitwise=False)
        assert voxproj_host.counters(_last_ws(), torch.device(DEV))["n_heavy"] > 50
        _, got2, _ = _compare(oracle_mod, feats, s.occ[None], s.c2w, s.intr, s.opts(), s.grid_origin, s.voxel_size,
                              s.n_vox + 1, bitwise=False)
        assert got.tobytes() == got2.tobytes()
    # an ID labelling several cells AND heavy: the parts come up short, k_combine_parts redoes the voxel over whole images
    occ = np.where(s.occ > 0, (s.occ % 5) + 1, 0).astype(np.int32)
    feats = make_features_np(5, 32, 48, 8, seed=32)[None]
    _compare(oracle_mod, feats, occ[None], s.c2w, s.intr, s.opts(), s.grid_origin, s.voxel_size, 7,
             expect_boxmiss=True, bitwise=False)


def test_pipelined_calls_of_varying_size(oracle_mod):
    # VP_FLAG_PIPELINE: phase 1 of a call overlaps the previous call's gather on a side stream, two buffer
    # sets alternate; calls of different V on one workspace must not disturb each other.
    import voxproj_host
    s = make_scene(2000, 11, 48, 32, seed=41, room=(5.0, 4.0, 2.4))
    C = 16
    feats = make_features_np(11, 32, 48, C, seed=41)
    n_rows = s.n_vox + 1
    count = np.zeros(n_rows, np.int32)
    out = np.zeros((n_rows, C), np.float32)
    dev = torch.device(DEV)
    feats_t = torch.from_numpy(feats[None]).to(dev)
    occ_t = torch.from_numpy(s.occ[None].astype(np.int64)).to(dev)
    c2w_t = torch.from_numpy(s.c2w).to(dev)
    intr_t = torch.from_numpy(s.intr[None]).to(dev)
    count_t = torch.zeros(n_rows, dtype=torch.int32, device=dev)
    out_t = torch.zeros(n_rows, C, device=dev)
    ws = voxproj_host.Workspace()
    opts = [float(v) for v in s.opts()]
    origin = [float(v) for v in s.grid_origin]
    splits = [(0, 4), (4, 8), (8, 9), (9, 11), (0, 3), (3, 11)]
    vmis = [c2w_t[a:b].reshape(-1).contiguous() for a, b in splits]
    for rep in range(2):
        for (a, b), vmi in zip(splits, vmis):
            oracle_mod.project_features(feats[None, a:b], s.occ[None].astype(np.int64), s.c2w[a:b].reshape(-1),
                                        s.intr[None], s.opts(), s.grid_origin, s.voxel_size, count, out)
            voxproj_host.project_features_raw(feats_t[:, a:b], occ_t, vmi, intr_t, opts, count_t, out_t, origin,
                                              s.voxel_size, workspace=ws, sync=False, pipeline=True)
    voxproj_host.workspace_status(ws, dev)
    assert voxproj_host.counters(ws, dev)["box_miss"] == 0
    assert np.array_equal(count_t.cpu().numpy(), count)
    assert out_t.cpu().numpy().tobytes() == out.tobytes()
    # a plain call on the same workspace after pipelined ones
    voxproj_host.project_features_raw(feats_t[:, 0:2], occ_t, vmis[0][:32].contiguous(), intr_t, opts, count_t, out_t,
                                      origin, s.voxel_size, workspace=ws, sync=True)
    oracle_mod.project_features(feats[None, 0:2], s.occ[None].astype(np.int64), s.c2w[0:2].reshape(-1),
                                s.intr[None], s.opts(), s.grid_origin, s.voxel_size, count, out)
    assert np.array_equal(count_t.cpu().numpy(), count)
    assert out_t.cpu().numpy().tobytes() == out.tobytes()


def test_occupancy_tables_follow_the_tensor_not_its_address(oracle_mod):
    # the drop-in keeps the occupancy-derived tables between calls only for the very same, unmodified tensor:
    # an in-place edit (version counter) and a new tensor at a recycled address must both rebuild them
    import voxproj_host
    s = make_scene(2000, 2, 40, 24, seed=61, room=(5.0, 4.0, 2.4))
    feats = make_features_np(2, 24, 40, 8, seed=61)[None]
    n_rows = s.n_vox + 1
    dev = torch.device(DEV)
    fixed = (torch.from_numpy(s.c2w).reshape(-1).to(dev), torch.from_numpy(s.intr[None]).to(dev),
             torch.from_numpy(s.opts()))
    tail = (torch.tensor([False]), torch.from_numpy(s.grid_origin), s.voxel_size)
    feats_t = torch.from_numpy(feats).to(dev)

    def check(occ_t, occ_np):
        count_t = torch.zeros(n_rows, dtype=torch.int32, device=dev)
        out_t = torch.zeros(n_rows, 8, device=dev)
        _drop_in()(feats_t, occ_t, *fixed, count_t, out_t, *tail)
        ref = oracle_mod.first_hit(occ_np[None].astype(np.int64), s.c2w.reshape(-1), s.intr[None], s.opts(),
                                   s.grid_origin, s.voxel_size, 1, 2)
        assert np.array_equal(voxproj_host.hit_image(_last_ws(), dev).cpu().numpy(), ref)
        assert int(count_t.sum()) == int((ref > 0).sum())

    occ_np = s.occ.copy()
    occ_t = torch.from_numpy(occ_np[None].astype(np.int64)).to(dev)
    check(occ_t, occ_np)
    builds = voxproj_host.table_builds(_last_ws())
    check(occ_t, occ_np)                                  # same tensor again: tables reused
    check(occ_t.clone(), occ_np)                          # a new tensor with equal contents (DPF:143): verified, reused
    check(torch.from_numpy(occ_np[None].astype(np.int64)).to(dev), occ_np)
    assert voxproj_host.table_builds(_last_ws()) == builds
    one = occ_t.clone()
    cell = tuple(int(v) for v in np.argwhere(occ_np == 0)[7])
    one[0][cell] = 5                                      # a new tensor that differs in ONE cell: rebuilt
    occ_one = occ_np.copy()
    occ_one[cell] = 5
    check(one, occ_one)
    assert voxproj_host.table_builds(_last_ws()) == builds + 1
    check(occ_t, occ_np)                                  # and back
    assert voxproj_host.table_builds(_last_ws()) == builds + 2
    zs = occ_np.shape[0]
    occ_np[: zs // 2] = 0                                 # in-place edit of the same tensor
    occ_t[:, : zs // 2] = 0
    check(occ_t, occ_np)
    del occ_t                                             # a different grid, most likely at the recycled address
    occ_np2 = np.where(s.occ > 0, s.occ, 0).copy()
    occ_np2[:, : occ_np2.shape[1] // 2] = 0
    occ_t2 = torch.from_numpy(occ_np2[None].astype(np.int64)).to(dev)
    check(occ_t2, occ_np2)


def test_out_of_range_id_raises(oracle_mod):
    s = make_scene(2000, 1, 40, 24, seed=23, room=(5.0, 4.0, 2.4))
    feats = make_features_np(1, 24, 40, 8, seed=23)[None]
    count_t = torch.zeros(100, dtype=torch.int32, device=DEV)       # far too small for IDs up to 2000
    out_t = torch.zeros(100, 8, device=DEV)
    with pytest.raises(RuntimeError, match="outside"):
        _gpu_call(feats, s.occ[None], s.c2w, s.intr, s.opts(), s.grid_origin, s.voxel_size, count_t, out_t)


def test_wrapper_checks_on_gpu():
    fn = _drop_in()
    B, V, H, W, C = 1, 1, 4, 4, 8
    a = [torch.zeros(B, V, H, W, C, device=DEV), torch.zeros(B, 2, 2, 2, dtype=torch.int64, device=DEV),
         torch.eye(4, device=DEV).reshape(-1), torch.ones(B, 4, device=DEV), torch.tensor([W, H, 0.01, 10.0, 0.5]),
         torch.zeros(3, dtype=torch.int32, device=DEV), torch.zeros(3, C, device=DEV), torch.tensor([False]),
         torch.zeros(3), 1.0]
    assert fn(*a) is None
    for i, msg in [(1, "occupancy_3D must be int64"), (5, "mapping2dto3d_num must be int32")]:
        b = list(a)
        b[i] = b[i].float()
        with pytest.raises(RuntimeError, match=msg):
            fn(*b)
    b = list(a)
    b[0] = a[0].permute(0, 1, 2, 4, 3)
    with pytest.raises(RuntimeError, match="encoded_2d_features must be contiguous"):
        fn(*b)
    b = list(a)
    b[2] = a[2].reshape(4, 4)
    with pytest.raises(RuntimeError, match="viewMatrixInv must be 1D flattened"):
        fn(*b)
    b = list(a)
    b[7] = torch.tensor([True])
    with pytest.raises(RuntimeError, match="pred_mode_t"):
        fn(*b)


def test_full_resolution_view_properties(oracle_mod):
    # BASELINE config 3 shape, one view: 200k voxels, 968x548x512.  IDs/counts against the oracle's march
    # (seconds on the host cores); sums through size-independent properties (linearity / checksums).
    import voxproj_host
    from synthetic_scene import make_features_torch
    s = make_scene(200000, 2, 968, 548, seed=0)
    V, H, W, C = 1, 548, 968, 512
    feats = make_features_torch(V, H, W, C, DEV, seed=0)[None]
    n_rows = s.n_vox + 1
    count_t = torch.zeros(n_rows, dtype=torch.int32, device=DEV)
    out_t = torch.zeros(n_rows, C, device=DEV)
    fn = _drop_in()
    occ_t = torch.from_numpy(s.occ[None].astype(np.int64)).to(DEV)
    args = (feats, occ_t, torch.from_numpy(s.c2w[:1]).reshape(-1).to(DEV), torch.from_numpy(s.intr[None]).to(DEV),
            torch.from_numpy(s.opts()), count_t, out_t, torch.tensor([False]), torch.from_numpy(s.grid_origin),
            s.voxel_size)
    fn(*args)
    ws = _last_ws()
    hits = voxproj_host.hit_image(ws, torch.device(DEV))
    ref = oracle_mod.first_hit(s.occ[None].astype(np.int64), s.c2w[:1].reshape(-1), s.intr[None], s.opts(),
                               s.grid_origin, s.voxel_size, 1, 1)
    assert np.array_equal(hits.cpu().numpy(), ref)
    ctr = voxproj_host.counters(ws, torch.device(DEV))
    assert ctr["bad_id"] == 0 and ctr["box_miss"] == 0
    flat = hits.reshape(-1).long()
    assert torch.equal(count_t.long(), torch.bincount(flat, minlength=n_rows) * (torch.arange(n_rows, device=DEV) > 0))
    # checksum of checksums: total over voxels == total over hit pixels (float64)
    mask = (flat > 0)
    tot_px = feats.reshape(-1, C)[mask].double().sum(0)
    tot_abs = feats.reshape(-1, C)[mask].double().abs().sum(0)
    tot_vx = out_t.double().sum(0)
    assert ((tot_px - tot_vx).abs() <= 1e-6 * tot_abs).all()      # fp32 row sums: ~1e-7 relative each
    # exact per-voxel sums for a sample of voxels, in raster order
    ids = torch.unique(flat[mask])[:: 997][:40]
    f2 = feats.reshape(-1, C)
    for i in ids.tolist():
        px = torch.nonzero(flat == i).reshape(-1)
        acc = torch.zeros(C, device=DEV)
        for j in px.tolist():
            acc = acc + f2[j]
        assert torch.equal(acc, out_t[i]), i
    # idempotence of the accumulate contract: a second call doubles counts and (to rounding) sums
    fn(*args)
    assert torch.equal(count_t.long(), 2 * torch.bincount(flat, minlength=n_rows) * (torch.arange(n_rows, device=DEV) > 0))
    assert ((out_t.double().sum(0) - 2 * tot_px).abs() <= 2e-6 * tot_abs).all()


def test_grid_with_more_cells_than_one_round_of_the_table_build(oracle_mod):
    """k_build_cells runs min(ceil(cells / 256), 16 384) workgroups of 256 threads and strides by gridDim * 256: a thread reads
    a second cell iff the grid has more than 16 384 * 256 = 4 194 304 cells (the 200k-voxel scene above has 3.96 M).  210 000
    voxels in the default room are 81 x 204 x 255 = 4 213 620 cells; the 19 316 cells past the first round hold voxels of the
    top layers, and a few hundred pixels of the two small views must hit them.
    k_occ_compare_copy (the drop-in's check that a new tensor still holds the grid the tables were built from) runs at most
    8192 workgroups the same way: those cells are its third lap.  A second call with a new tensor that differs in one of them
    alone, a voxel the first call hit, must rebuild the tables and lose that voxel."""
    import voxproj_host
    s = make_scene(210000, 2, 64, 48, seed=3)
    lap = 16384 * 256
    assert lap < s.occ.size < lap + lap // 64 and lap == 2 * 8192 * 256
    feats = make_features_np(2, 48, 64, 8, seed=3)[None]
    case = (s.c2w, s.intr, s.opts(), s.grid_origin, s.voxel_size, s.n_vox + 1)
    r, _, _ = _compare(oracle_mod, feats, s.occ[None], *case, expect_boxmiss=None)
    builds = voxproj_host.table_builds(_last_ws())
    tail = s.occ.reshape(-1)[lap:]
    late = np.isin(r["hits"], tail[tail > 0])
    assert late.sum() > 300
    gone = int(np.bincount(r["hits"][late]).argmax())        # the voxel of the tail that most pixels hit
    occ = s.occ.copy()
    occ[occ == gone] = 0
    assert (occ != s.occ).sum() == 1 and int(np.flatnonzero(occ.reshape(-1) != s.occ.reshape(-1))[0]) >= lap
    r2, _, _ = _compare(oracle_mod, feats, occ[None], *case, expect_boxmiss=None)
    assert voxproj_host.table_builds(_last_ws()) == builds + 1
    assert not (r2["hits"] == gone).any() and (r["hits"] == gone).sum() >= 1


def test_far_from_origin_disables_leaping_but_stays_exact(oracle_mod):
    # world coordinates ~1e6 voxel sizes from zero: fp32 positions are too coarse for the leap bound, the kernel
    # must fall back to evaluating every sample (leap_ok = false) and still match the oracle bit for bit
    s = make_scene(2000, 2, 40, 24, seed=51, room=(5.0, 4.0, 2.4))
    shift = np.array([30000.0, -20000.0, 10000.0], np.float32)
    c2w = s.c2w.copy()
    c2w[:, :3, 3] += shift
    feats = make_features_np(2, 24, 40, 8, seed=51)[None]
    r, _, _ = _compare(oracle_mod, feats, s.occ[None], c2w, s.intr, s.opts(), s.grid_origin + shift, s.voxel_size,
                       s.n_vox + 1)
    assert (r["hits"] > 0).mean() > 0.3


def test_degenerate_and_scaled_poses(oracle_mod):
    # view 0: singular camera matrix (all rays collapse; the search box falls back to whole images);
    # view 1: non-rigid pose (anisotropic scale + shear) -- the box uses the true inverse, rays are the reference's
    s = make_scene(2000, 3, 40, 24, seed=52, room=(5.0, 4.0, 2.4))
    c2w = s.c2w.copy()
    c2w[0, :3, :3] = 0.0
    c2w[0, 0, 2] = 1.0                                   # rank-1: every direction maps onto +x
    c2w[1, :3, :3] = c2w[1, :3, :3] @ np.array([[1.3, 0.2, 0.0], [0.0, 0.8, 0.1], [0.0, 0.0, 1.1]], np.float32)
    feats = make_features_np(3, 24, 40, 8, seed=52)[None]
    _compare(oracle_mod, feats, s.occ[None], c2w, s.intr, s.opts(), s.grid_origin, s.voxel_size, s.n_vox + 1)


def test_non_finite_poses_and_intrinsics(oracle_mod):
    # ScanNet marks a frame whose tracking was lost with a pose of -inf; a NaN can come out of a bad calibration file.
    # The reference marches such rays all the same (K.cu:47-82: every comparison with a NaN is false, the float -> int
    # conversion of a NaN is 0 and saturates otherwise, so the samples all land in cell (0,0,0) or nowhere); the
    # oracle restates that, the kernels must neither hang nor differ.  Cell (0,0,0) is occupied in one of the grids.
    s = make_scene(2000, 5, 40, 24, seed=56, room=(5.0, 4.0, 2.4))
    feats = make_features_np(5, 24, 40, 8, seed=56)[None]
    c2w = s.c2w.copy()
    c2w[0, :, :] = -np.inf                               # ScanNet's "invalid pose"
    c2w[1, :3, 3] = np.nan                               # position unknown
    c2w[2, 0, 0] = np.inf                                # one infinite rotation entry
    c2w[3, 1, 2] = np.nan
    for corner_id in (0, 7):
        occ = s.occ[None].copy()
        occ[0, 0, 0, 0] = corner_id
        _compare(oracle_mod, feats, occ, c2w, s.intr, s.opts(), s.grid_origin, s.voxel_size, s.n_vox + 1, expect_boxmiss=None)
    for intr in (np.array([0.0, s.intr[1], s.intr[2], s.intr[3]], np.float32),          # fx = 0: directions divide by zero
                 np.array([s.intr[0], np.nan, s.intr[2], s.intr[3]], np.float32),
                 np.array([s.intr[0], s.intr[1], np.inf, s.intr[3]], np.float32)):
        _compare(oracle_mod, feats, s.occ[None], s.c2w, intr, s.opts(), s.grid_origin, s.voxel_size, s.n_vox + 1, expect_boxmiss=None)
    for opts in (np.array([40, 24, np.nan, 10.0, 0.5 * s.voxel_size], np.float32),      # NaN range: no sample is taken
                 np.array([40, 24, 0.01, np.inf, 0.5 * s.voxel_size], np.float32)):     # dmax = inf: direction (0,0,NaN)
        _compare(oracle_mod, feats, s.occ[None], s.c2w, s.intr, opts, s.grid_origin, s.voxel_size, s.n_vox + 1, expect_boxmiss=None)


def test_non_finite_poses_in_job_mode(oracle_mod):
    # the same nulls through the merged gather (calls of >= 8 views) and the grouped first-tile fetch, pipelined
    import voxproj_host
    dev = torch.device(DEV)
    s = make_scene(2000, 10, 40, 24, seed=58, room=(5.0, 4.0, 2.4))
    feats = make_features_np(10, 24, 40, 16, seed=58)[None]
    c2w = s.c2w.copy()
    c2w[1, :, :] = -np.inf
    c2w[4, :3, 3] = np.nan
    c2w[6, 2, 1] = np.inf
    occ = s.occ[None].astype(np.int64).copy()
    occ[0, 0, 0, 0] = 9                                   # the cell every NaN sample lands in is occupied
    n_rows = s.n_vox + 1
    count, out = np.zeros(n_rows, np.int32), np.zeros((n_rows, 16), np.float32)
    for _ in range(2):
        r = oracle_mod.project_features(feats, occ, c2w.reshape(-1), s.intr[None], s.opts(), s.grid_origin, s.voxel_size, count, out)
    assert r["rc"] == 0 and count[9] >= 2 * 960
    for f in (feats, feats.astype(np.float16)):
        if f.dtype == np.float16:
            count[:] = 0; out[:] = 0
            for _ in range(2):
                oracle_mod.project_features(f.astype(np.float32), occ, c2w.reshape(-1), s.intr[None], s.opts(), s.grid_origin,
                                            s.voxel_size, count, out)
        count_t = torch.zeros(n_rows, dtype=torch.int32, device=dev)
        out_t = torch.zeros(n_rows, 16, device=dev)
        ws = voxproj_host.Workspace()
        args = (torch.from_numpy(f).to(dev), torch.from_numpy(occ).to(dev), torch.from_numpy(c2w).reshape(-1).to(dev),
                torch.from_numpy(s.intr[None]).to(dev), [float(v) for v in s.opts()], count_t, out_t,
                [float(v) for v in s.grid_origin], s.voxel_size)
        for _ in range(2):
            voxproj_host.project_features_raw(*args, workspace=ws, sync=False, pipeline=True)
        voxproj_host.workspace_status(ws, dev)
        torch.cuda.synchronize()
        assert np.array_equal(count_t.cpu().numpy(), count)
        assert out_t.cpu().numpy().tobytes() == out.tobytes()
        ws.release()


def test_non_finite_feature_values_propagate_like_the_reference(oracle_mod):
    # a NaN / Inf in a feature map ends up in exactly the voxels the reference's atomicAdd would poison (AGG:303-304 looks
    # for them afterwards); compared NaN-for-NaN, since inf - inf makes a NaN whose sign bit is the processor's choice
    s = make_scene(2000, 3, 40, 24, seed=57, room=(5.0, 4.0, 2.4))
    feats = make_features_np(3, 24, 40, 8, seed=57)[None]
    feats[0, 0, 3, 5, 2] = np.nan
    feats[0, 1, 10, 20, :] = np.inf
    feats[0, 2, 11, 21, 4] = -np.inf
    feats[0, 2, 12, 22, 4] = np.inf
    n_rows = s.n_vox + 1
    count, out = np.zeros(n_rows, np.int32), np.zeros((n_rows, 8), np.float32)
    r = oracle_mod.project_features(feats, s.occ[None].astype(np.int64), s.c2w.reshape(-1), s.intr[None], s.opts(), s.grid_origin,
                                    s.voxel_size, count, out)
    assert r["rc"] == 0 and np.isnan(out).any() and np.isinf(out).any()
    count_t = torch.zeros(n_rows, dtype=torch.int32, device=DEV)
    out_t = torch.zeros(n_rows, 8, device=DEV)
    _gpu_call(feats, s.occ[None], s.c2w, s.intr, s.opts(), s.grid_origin, s.voxel_size, count_t, out_t)
    got = out_t.cpu().numpy()
    assert np.array_equal(count_t.cpu().numpy(), count)
    assert np.array_equal(np.isnan(got), np.isnan(out))
    fin = ~np.isnan(out)
    assert got[fin].tobytes() == out[fin].tobytes()


def test_zero_depth_min_and_coarse_steps(oracle_mod):
    s = make_scene(2000, 2, 40, 24, seed=53, room=(5.0, 4.0, 2.4))
    feats = make_features_np(2, 24, 40, 8, seed=53)[None]
    for opts in (np.array([40, 24, 0.0, 10.0, 0.5 * s.voxel_size], np.float32),        # dmin = 0: t starts at 0
                 np.array([40, 24, 0.01, 3.0, 2.7 * s.voxel_size], np.float32),        # steps longer than a voxel
                 np.array([40, 24, 0.5, 2.0, 0.013 * s.voxel_size], np.float32)):      # very fine steps, short range
        _compare(oracle_mod, feats, s.occ[None], s.c2w, s.intr, opts, s.grid_origin, s.voxel_size, s.n_vox + 1)


def test_image_sizes_not_multiples_of_the_tiles(oracle_mod):
    for (W, H) in ((1, 1), (7, 3), (17, 33), (65, 9)):
        s = make_scene(2000, 2, W, H, seed=54, room=(5.0, 4.0, 2.4))
        feats = make_features_np(2, H, W, 4, seed=54)[None]
        _compare(oracle_mod, feats, s.occ[None], s.c2w, s.intr, s.opts(), s.grid_origin, s.voxel_size, s.n_vox + 1)


def test_camera_inside_and_next_to_voxels(oracle_mod):
    # cameras sitting on the wall / inside an occupied block: cubes straddle the near plane, boxes are clipped
    s = make_scene(2000, 4, 40, 24, seed=55, room=(5.0, 4.0, 2.4))
    c2w = s.c2w.copy()
    c2w[0, :3, 3] = s.points[100] + np.float32(0.3 * s.voxel_size)
    c2w[1, :3, 3] = s.points[900] - np.float32(0.6 * s.voxel_size)
    c2w[2, 2, 3] = s.grid_origin[2] + np.float32(1.2 * s.voxel_size)     # just above the floor
    feats = make_features_np(4, 24, 40, 8, seed=55)[None]
    r, _, _ = _compare(oracle_mod, feats, s.occ[None], c2w, s.intr, s.opts(), s.grid_origin, s.voxel_size, s.n_vox + 1)


def test_march_ab_arm_exact_loop_equals_leaping(oracle_mod, monkeypatch):
    s = make_scene(2000, 2, 40, 24, seed=56, room=(5.0, 4.0, 2.4))
    feats = make_features_np(2, 24, 40, 8, seed=56)[None]
    import project_features_cuda
    import voxproj_host
    monkeypatch.setattr(voxproj_host, "EXACT_MARCH", True)
    project_features_cuda.set_exact_march(True)
    try:
        _compare(oracle_mod, feats, s.occ[None], s.c2w, s.intr, s.opts(), s.grid_origin, s.voxel_size, s.n_vox + 1)
    finally:
        project_features_cuda.set_exact_march(False)
    monkeypatch.setattr(voxproj_host, "EXACT_MARCH", False)
    _compare(oracle_mod, feats, s.occ[None], s.c2w, s.intr, s.opts(), s.grid_origin, s.voxel_size, s.n_vox + 1)


def test_ray_parameter_closed_form_over_many_increments(oracle_mod):
    # the march reproduces t += inc by a closed form per binade; sweep increments with awkward bit patterns
    # (powers of two, one-bit / all-bits mantissas, increments larger than early t values) on a sparse grid where
    # most rays run the whole [dmin, dmax) range through every binade
    rng = np.random.default_rng(77)
    occ = np.zeros((16, 24, 28), np.int32)
    idx = rng.choice(occ.size, 150, replace=False)
    occ.reshape(-1)[idx] = np.arange(1, 151)
    s = make_scene(2000, 2, 24, 16, seed=78, room=(5.0, 4.0, 2.4))
    feats = make_features_np(2, 16, 24, 4, seed=79)[None]
    incs = [0.125, 0.03125, np.float32(0.1), np.float32(1.0) / 3, np.float32(0.0625) + np.float32(2.0 ** -27),
            np.float32(0.02) , np.float32(0.7), np.float32(2.5), np.float32(0.011111111)]
    incs += [np.float32(v) for v in np.exp(rng.uniform(np.log(0.004), np.log(1.5), 8))]
    for dmin, dmax in ((0.01, 10.0), (0.0, 33.0), (1e-4, 5.0)):
        for inc in incs:
            opts = np.array([24, 16, dmin, dmax, inc], np.float32)
            _compare(oracle_mod, feats, occ[None], s.c2w, s.intr, opts, np.array([-2.1, -1.7, 0.05], np.float32), 0.2, 151)


@pytest.mark.parametrize("lds_kb", [None, 0, 64])
def test_pipelined_occupancy_knob_stays_exact(oracle_mod, lds_kb):
    # the march's occupancy cap in pipelined mode (a dynamic-LDS reservation, VP_OPT_MARCH_LDS_KB) is a scheduling hint only
    import voxproj_host
    s = make_scene(2000, 9, 48, 32, seed=71, room=(5.0, 4.0, 2.4))
    C = 16
    feats = make_features_np(9, 32, 48, C, seed=71)
    n_rows = s.n_vox + 1
    count = np.zeros(n_rows, np.int32)
    out = np.zeros((n_rows, C), np.float32)
    dev = torch.device(DEV)
    feats_t = torch.from_numpy(feats[None]).to(dev)
    occ_t = torch.from_numpy(s.occ[None].astype(np.int64)).to(dev)
    c2w_t = torch.from_numpy(s.c2w).to(dev)
    intr_t = torch.from_numpy(s.intr[None]).to(dev)
    count_t = torch.zeros(n_rows, dtype=torch.int32, device=dev)
    out_t = torch.zeros(n_rows, C, device=dev)
    ws = voxproj_host.Workspace()
    ws.set_option(voxproj_host.VP_OPT_MARCH_LDS_KB, lds_kb)
    splits = [(0, 5), (5, 6), (6, 9), (0, 9)]
    vmis = [c2w_t[a:b].reshape(-1).contiguous() for a, b in splits]
    for (a, b), vmi in zip(splits, vmis):
        oracle_mod.project_features(feats[None, a:b], s.occ[None].astype(np.int64), s.c2w[a:b].reshape(-1), s.intr[None],
                                    s.opts(), s.grid_origin, s.voxel_size, count, out)
        voxproj_host.project_features_raw(feats_t[:, a:b], occ_t, vmi, intr_t, [float(v) for v in s.opts()], count_t, out_t,
                                          [float(v) for v in s.grid_origin], s.voxel_size, workspace=ws, sync=False,
                                          pipeline=True)
    voxproj_host.workspace_status(ws, dev)
    assert np.array_equal(count_t.cpu().numpy(), count)
    assert out_t.cpu().numpy().tobytes() == out.tobytes()
    # a reservation beyond a kernel's 64-KiB dynamic-LDS limit is refused when it is SET (it used to fail every
    # launch on the workspace with a generic HIP error, in pipelined mode calls later); the workspace stays usable
    with pytest.raises(voxproj_host.VoxprojError, match="limited to 64 KiB"):
        voxproj_host.check(voxproj_host.lib().vp_workspace_set_option(ws.ptr(), voxproj_host.VP_OPT_MARCH_LDS_KB, 80))
    voxproj_host.project_features_raw(feats_t[:, :5], occ_t, vmis[0], intr_t, [float(v) for v in s.opts()], count_t, out_t,
                                      [float(v) for v in s.grid_origin], s.voxel_size, workspace=ws, sync=True)
    ws.release()


def test_fp16_feature_maps_give_the_fp32_bits(oracle_mod):
    # the same data stored as binary16 must produce bit-identical sums/counts (exact widening,
    # same summation order) -- normal wavefront path, C = 512 / 64 / 1000-rounded-to-8, and a pipelined sequence
    import voxproj_host
    dev = torch.device(DEV)
    s = make_scene(2000, 5, 48, 32, seed=81, room=(5.0, 4.0, 2.4))
    for C in (512, 64, 1000):
        f16 = make_features_np(5, 32, 48, C, seed=81).astype(np.float16)
        f32 = f16.astype(np.float32)
        n_rows = s.n_vox + 1
        count = np.zeros(n_rows, np.int32)
        out = np.zeros((n_rows, C), np.float32)
        oracle_mod.project_features(f32[None], s.occ[None].astype(np.int64), s.c2w.reshape(-1), s.intr[None], s.opts(),
                                    s.grid_origin, s.voxel_size, count, out)
        count_t = torch.zeros(n_rows, dtype=torch.int32, device=dev)
        out_t = torch.zeros(n_rows, C, device=dev)
        ws = voxproj_host.Workspace()
        occ_t = torch.from_numpy(s.occ[None].astype(np.int64)).to(dev)
        c2w_t = torch.from_numpy(s.c2w).to(dev)
        intr_t = torch.from_numpy(s.intr[None]).to(dev)
        f_t = torch.from_numpy(f16[None]).to(dev)
        vm = [c2w_t[a:b].reshape(-1).contiguous() for a, b in ((0, 2), (2, 5))]
        for (a, b), v in zip(((0, 2), (2, 5)), vm):
            voxproj_host.project_features_raw(f_t[:, a:b], occ_t, v, intr_t, [float(x) for x in s.opts()], count_t, out_t,
                                              [float(x) for x in s.grid_origin], s.voxel_size, workspace=ws, sync=False,
                                              pipeline=True)
        voxproj_host.workspace_status(ws, dev)
        assert np.array_equal(count_t.cpu().numpy(), count)
        assert out_t.cpu().numpy().tobytes() == out.tobytes()


def test_fp16_heavy_path(oracle_mod, heavy_threshold):
    import voxproj_host
    heavy_threshold(6)
    dev = torch.device(DEV)
    s = make_scene(2000, 4, 48, 32, seed=82, room=(5.0, 4.0, 2.4))
    C = 512
    f16 = make_features_np(4, 32, 48, C, seed=82).astype(np.float16)
    n_rows = s.n_vox + 1
    count = np.zeros(n_rows, np.int32)
    out = np.zeros((n_rows, C), np.float32)
    r = oracle_mod.project_features(f16.astype(np.float32)[None], s.occ[None].astype(np.int64), s.c2w.reshape(-1), s.intr[None],
                                    s.opts(), s.grid_origin, s.voxel_size, count, out, want_f64=True)
    count_t = torch.zeros(n_rows, dtype=torch.int32, device=dev)
    out_t = torch.zeros(n_rows, C, device=dev)
    ws = voxproj_host.project_features_raw(torch.from_numpy(f16[None]).to(dev), torch.from_numpy(s.occ[None].astype(np.int64)).to(dev),
                                           torch.from_numpy(s.c2w).reshape(-1).to(dev), torch.from_numpy(s.intr[None]).to(dev),
                                           [float(x) for x in s.opts()], count_t, out_t, [float(x) for x in s.grid_origin],
                                           s.voxel_size, sync=True)
    assert voxproj_host.counters(ws, dev)["n_heavy"] > 50
    assert np.array_equal(count_t.cpu().numpy(), count)
    assert (np.abs(out_t.cpu().numpy() - r["out64"]) / (np.abs(r["out64"]).max(axis=1, keepdims=True) + 1e-30)).max() <= 1e-4


def test_negative_depth_min_marches_from_behind_the_camera(oracle_mod):
    # depthMin < 0: the reference's loop starts at negative t and can hit voxels BEHIND the camera; the search boxes
    # assume samples in front, so such voxels take the whole-image fallback -- results must still be exact
    s = make_scene(2000, 2, 40, 24, seed=57, room=(5.0, 4.0, 2.4))
    feats = make_features_np(2, 24, 40, 8, seed=57)[None]
    opts = np.array([40, 24, -1.5, 6.0, 0.5 * s.voxel_size], np.float32)
    _compare(oracle_mod, feats, s.occ[None], s.c2w, s.intr, opts, s.grid_origin, s.voxel_size, s.n_vox + 1, expect_boxmiss=None)


def test_increment_too_small_to_advance_raises_instead_of_hanging(oracle_mod):
    # inc below half an ulp of t: the reference's while-loop never terminates (K.cu:47,81); here it is an error
    s = make_scene(2000, 1, 16, 8, seed=58, room=(5.0, 4.0, 2.4))
    feats = make_features_np(1, 8, 16, 4, seed=58)[None]
    count_t = torch.zeros(s.n_vox + 1, dtype=torch.int32, device=DEV)
    out_t = torch.zeros(s.n_vox + 1, 4, device=DEV)
    opts = np.array([16, 8, 0.01, 10.0, 1e-8], np.float32)
    with pytest.raises(RuntimeError, match="never terminate"):
        _gpu_call(feats, s.occ[None], s.c2w, s.intr, opts, s.grid_origin, s.voxel_size, count_t, out_t)


def _random_rotation(rng):
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def test_randomized_differential_against_the_oracle(oracle_mod):
    # 80 random configurations: grid shape and density, voxel size, origin, free camera poses (inside and outside the
    # grid, any orientation), intrinsics, image size, ray range and increment, channel count, views per call
    rng = np.random.default_rng(2025)
    n_hit_cases = 0
    for case in range(80):
        dims = rng.integers(3, 40, 3)                      # Z, Y, X
        dens = float(np.exp(rng.uniform(np.log(0.002), np.log(0.35))))
        occ = np.zeros(dims, np.int32)
        n = max(1, int(occ.size * dens))
        idx = rng.choice(occ.size, n, replace=False)
        occ.reshape(-1)[idx] = rng.permutation(n) + 1
        vs = float(np.float32(np.exp(rng.uniform(np.log(0.02), np.log(0.5)))))
        origin = rng.uniform(-3, 3, 3).astype(np.float32)
        ext = dims[::-1] * vs                               # x, y, z extent
        V = int(rng.integers(1, 5))
        W, H = int(rng.integers(1, 40)), int(rng.integers(1, 30))
        C = int(rng.choice([1, 4, 5, 8, 16, 36]))
        c2w = np.zeros((V, 4, 4), np.float32)
        for v in range(V):
            c2w[v, :3, :3] = _random_rotation(rng)
            c2w[v, :3, 3] = origin + rng.uniform(-0.6, 1.6, 3) * ext
            c2w[v, 3, 3] = 1
        f = float(rng.uniform(0.4, 2.5)) * W
        intr = np.array([f, f * rng.uniform(0.8, 1.25), rng.uniform(0.2, 0.8) * W, rng.uniform(0.2, 0.8) * H], np.float32)
        dmin = float(rng.choice([0.0, 0.01, 0.3]))
        dmax = float(rng.uniform(0.5, 3.0) * np.linalg.norm(ext))
        inc = float(np.float32(vs * np.exp(rng.uniform(np.log(0.15), np.log(2.0)))))
        opts = np.array([W, H, dmin, dmax, inc], np.float32)
        feats = rng.standard_normal((1, V, H, W, C)).astype(np.float32)
        r, _, _ = _compare(oracle_mod, feats, occ[None], c2w, intr, opts, origin, vs, n + 1, expect_boxmiss=None)
        n_hit_cases += int((r["hits"] > 0).any())
    assert n_hit_cases > 30


def test_randomized_job_mode_against_the_oracle(oracle_mod, heavy_threshold):
    # the raw API the way a job drives it: batches of grids (B 1..3), many views per call (up to 70), sequences of
    # pipelined or plain calls accumulating into the same outputs, fp32 or fp16 feature maps, heavy-voxel thresholds
    # low enough to split voxels into parts, the optional per-view hit counter.  Counts and view counts
    # exact, sums within 1e-4 of the oracle's float64 accumulation.
    import voxproj_host
    dev = torch.device(DEV)
    rng = np.random.default_rng(777)
    saw_heavy = 0
    for case in range(24):
        B = int(rng.integers(1, 4))
        dims = rng.integers(4, 28, 3)
        n_ids = int(rng.integers(5, 400))
        occ = np.zeros((B, *dims), np.int32)
        for b in range(B):
            n = min(n_ids, int(occ[b].size * float(rng.uniform(0.01, 0.3))) + 1)
            idx = rng.choice(occ[b].size, n, replace=False)
            occ[b].reshape(-1)[idx] = rng.choice(n_ids, n, replace=False) + 1
        vs = float(np.float32(rng.uniform(0.05, 0.3)))
        origin = rng.uniform(-1, 1, 3).astype(np.float32)
        ext = dims[::-1] * vs
        W, H = int(rng.integers(4, 36)), int(rng.integers(4, 28))
        C = int(rng.choice([8, 16, 40]))
        f16 = bool(rng.integers(0, 2))
        pipeline = bool(rng.integers(0, 2))
        heavy_threshold(int(rng.choice([3, 20, 100000000])))
        f = float(rng.uniform(0.5, 2.0)) * W
        intr = np.stack([np.array([f, f, W * rng.uniform(0.3, 0.7), H * rng.uniform(0.3, 0.7)], np.float32) for _ in range(B)])
        opts = np.array([W, H, 0.01, float(2.0 * np.linalg.norm(ext)), float(np.float32(vs * rng.uniform(0.3, 1.2)))], np.float32)
        n_rows = n_ids + 1
        count = np.zeros(n_rows, np.int32)
        out = np.zeros((n_rows, C), np.float32)
        out64 = np.zeros((n_rows, C), np.float64)
        views = np.zeros(n_rows, np.int64)
        count_t = torch.zeros(n_rows, dtype=torch.int32, device=dev)
        out_t = torch.zeros(n_rows, C, device=dev)
        views_t = torch.zeros(n_rows, dtype=torch.int32, device=dev)
        occ_t = torch.from_numpy(occ.astype(np.int64)).to(dev)
        intr_t = torch.from_numpy(intr).to(dev)
        ws = voxproj_host.Workspace()
        keep = []
        for call in range(int(rng.integers(1, 4))):
            V = int(rng.choice([1, 2, 5, 17, 70]))
            c2w = np.zeros((B, V, 4, 4), np.float32)
            for b in range(B):
                for v in range(V):
                    c2w[b, v, :3, :3] = _random_rotation(rng)
                    c2w[b, v, :3, 3] = origin + rng.uniform(-0.3, 1.3, 3) * ext
                    c2w[b, v, 3, 3] = 1
            feats = rng.standard_normal((B, V, H, W, C)).astype(np.float32)
            if f16:
                feats = feats.astype(np.float16).astype(np.float32)
            r = oracle_mod.project_features(feats, occ.astype(np.int64), c2w.reshape(-1), intr, opts, origin, vs, count, out,
                                            want_f64=True)
            assert r["rc"] == 0
            out64 += r["out64"]
            for b in range(B):
                for v in range(V):
                    ids = np.unique(r["hits"][b, v])
                    views[ids[ids > 0]] += 1
            ft = torch.from_numpy(feats).to(dev)
            ft = ft.half() if f16 else ft
            vm = torch.from_numpy(c2w).reshape(-1).to(dev)
            keep.append((ft, vm))
            voxproj_host.project_features_raw(ft, occ_t, vm, intr_t, [float(v) for v in opts], count_t, out_t,
                                              [float(v) for v in origin], vs, workspace=ws, sync=not pipeline,
                                              reuse_accel=None, pipeline=pipeline, views_hit=views_t)
            if pipeline:
                voxproj_host.workspace_status(ws, dev)      # needed before the counters below, not between calls in general
            saw_heavy += voxproj_host.counters(ws, dev)["n_heavy"] > 0
        voxproj_host.workspace_status(ws, dev)
        assert np.array_equal(count_t.cpu().numpy(), count), case
        assert np.array_equal(views_t.cpu().numpy().astype(np.int64), views), case
        scale = np.abs(out64).max(axis=1, keepdims=True) + 1e-30
        assert (np.abs(out_t.cpu().numpy().astype(np.float64) - out64) / scale).max() <= 1e-4, case      # of each ROW's magnitude
        ws.release()
    assert saw_heavy >= 3


def test_device_errors_of_an_early_pipelined_call_are_still_reported(oracle_mod):
    # The status words are sticky per workspace: an out-of-range ID (or a ray that cannot advance) raised by the
    # FIRST of five pipelined calls must still surface at workspace_status, although the two buffer sets -- and with
    # them the per-call counters -- have been recycled twice since (the reference only prints device errors,
    # project_image_cuda_kernel.cu:454-457).  Reading the status clears it.
    import voxproj_host
    dev = torch.device(DEV)
    s = make_scene(2000, 6, 48, 32, seed=91, room=(5.0, 4.0, 2.4))
    C = 8
    feats_t = torch.from_numpy(make_features_np(6, 32, 48, C, seed=91)[None]).to(dev)
    occ_t = torch.from_numpy(s.occ[None].astype(np.int64)).to(dev)
    c2w_t = torch.from_numpy(s.c2w).to(dev)
    intr_t = torch.from_numpy(s.intr[None]).to(dev)
    origin = [float(v) for v in s.grid_origin]
    good = [float(v) for v in s.opts()]
    n_rows = s.n_vox + 1
    vmis = [c2w_t[v:v + 1].reshape(-1).contiguous() for v in range(6)]

    occ_bad = occ_t + (occ_t > 0) * 5000                         # every ID beyond the outputs' rows

    def run(first_opts, first_occ):
        ws = voxproj_host.Workspace()
        own = (torch.zeros(n_rows, dtype=torch.int32, device=dev), torch.zeros(n_rows, C, device=dev))
        full = (torch.zeros(n_rows, dtype=torch.int32, device=dev), torch.zeros(n_rows, C, device=dev))
        for k in range(5):
            cnt, out = own if k == 0 else full
            voxproj_host.project_features_raw(feats_t[:, k:k + 1], first_occ if k == 0 else occ_t, vmis[k], intr_t,
                                              first_opts if k == 0 else good, cnt, out, origin, s.voxel_size, workspace=ws,
                                              sync=False, pipeline=True)
        return ws, full

    ws, _ = run(good, occ_bad)                                   # call 0: a grid whose IDs the outputs have no rows for
    with pytest.raises(voxproj_host.VoxprojError, match="outside"):
        voxproj_host.workspace_status(ws, dev)
    voxproj_host.workspace_status(ws, dev)                       # cleared by the read: the workspace is usable again
    bad_inc = list(good)
    bad_inc[4] = 1e-8
    ws, _ = run(bad_inc, occ_t)                                  # call 0: increment below half an ulp of t
    with pytest.raises(voxproj_host.VoxprojError, match="never terminate"):
        voxproj_host.workspace_status(ws, dev)
    voxproj_host.workspace_status(ws, dev)
    ws, full = run(good, occ_t)                                  # and a clean sequence reports nothing
    voxproj_host.workspace_status(ws, dev)
    # calls 1..4 accumulated into `full` (call 0 went into its own tensors)
    h = oracle_mod.first_hit(s.occ[None].astype(np.int64), s.c2w[1:5].reshape(-1), s.intr[None], s.opts(), s.grid_origin,
                             s.voxel_size, 1, 4)
    ref = np.bincount(h.reshape(-1), minlength=n_rows).astype(np.int32) * (np.arange(n_rows) > 0)
    assert np.array_equal(full[0].cpu().numpy(), ref)


def test_reuse_accel_on_a_workspace_without_tables_is_refused():
    # VP_FLAG_REUSE_ACCEL is only honoured for tables the library built on this very workspace for this grid shape
    import voxproj_host
    dev = torch.device(DEV)
    s = make_scene(2000, 1, 40, 24, seed=92, room=(5.0, 4.0, 2.4))
    feats_t = torch.from_numpy(make_features_np(1, 24, 40, 8, seed=92)[None]).to(dev)
    occ_t = torch.from_numpy(s.occ[None].astype(np.int64)).to(dev)
    args = (torch.from_numpy(s.c2w).reshape(-1).to(dev), torch.from_numpy(s.intr[None]).to(dev), [float(v) for v in s.opts()])
    n_rows = s.n_vox + 1
    cnt, out = torch.zeros(n_rows, dtype=torch.int32, device=dev), torch.zeros(n_rows, 8, device=dev)
    tail = ([float(v) for v in s.grid_origin], s.voxel_size)
    ws = voxproj_host.Workspace()
    with pytest.raises(voxproj_host.VoxprojError, match="VP_FLAG_REUSE_ACCEL"):
        voxproj_host.project_features_raw(feats_t, occ_t, *args, cnt, out, *tail, workspace=ws, reuse_accel=True)
    voxproj_host.project_features_raw(feats_t, occ_t, *args, cnt, out, *tail, workspace=ws, reuse_accel=False)
    single = cnt.clone()
    assert int(single.sum()) > 0
    voxproj_host.project_features_raw(feats_t, occ_t, *args, cnt, out, *tail, workspace=ws, reuse_accel=True)     # now fine
    assert torch.equal(cnt, 2 * single)
    cnt2, out2 = torch.zeros(n_rows + 7, dtype=torch.int32, device=dev), torch.zeros(n_rows + 7, 8, device=dev)
    with pytest.raises(voxproj_host.VoxprojError, match="VP_FLAG_REUSE_ACCEL"):                                    # other n_rows
        voxproj_host.project_features_raw(feats_t, occ_t, *args, cnt2, out2, *tail, workspace=ws, reuse_accel=True)


def test_grid_without_voxels_and_single_row_outputs(oracle_mod):
    # an empty occupancy grid with outputs of one row (max_id + 1 = 1, DPF:158-159): nothing to march into, nothing to
    # gather -- the call must simply return and leave the dummy row untouched, for one view and for many
    for V in (1, 9):
        feats = np.random.default_rng(V).standard_normal((1, V, 8, 12, 4)).astype(np.float32)
        occ = np.zeros((1, 5, 6, 7), np.int64)
        count_t = torch.zeros(1, dtype=torch.int32, device=DEV)
        out_t = torch.full((1, 4), 3.5, device=DEV)
        c2w = np.tile(np.eye(4, dtype=np.float32), (V, 1, 1))
        _gpu_call(feats, occ, c2w, np.array([10, 10, 6, 4], np.float32), np.array([12, 8, 0.01, 10.0, 0.05], np.float32),
                  np.zeros(3, np.float32), 0.1, count_t, out_t)
        assert int(count_t[0]) == 0 and bool((out_t == 3.5).all())
