"""vp_voxel_grid on the GPU against the NumPy twin's np.unique result (tests/voxel_grid_reference.py): every output equal."""
import numpy as np
import pytest
import torch

import voxel_grid_reference as vg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check(points, colors, voxel_size, keep=None, workspace=None):
    import voxproj_host
    want = vg.voxelize(points, colors, voxel_size, keep=keep)
    got = voxproj_host.voxel_grid(_dev(points), _dev(colors), voxel_size, keep=_dev(None if keep is None else np.asarray(keep, np.uint8)),
                                  workspace=workspace)
    assert int(got["status"].item()) == want["status"]
    V = len(want["centers"])
    assert int(got["n_voxels"].item()) == V and got["centers"].shape == (V, 3)
    if want["status"]:
        assert (got["point_voxel"] == -1).all()                      # nothing written: the wrapper's fill is still there
        return got
    for k in ("centers", "colors", "counts", "voxel_index", "point_voxel"):
        g = got[k].cpu().numpy()
        assert g.dtype == want[k].dtype and g.tobytes() == want[k].tobytes(), k
    assert np.array_equal(got["min_corner"].cpu().numpy(), want["min_corner"])
    return got


def scene(n, seed, spread=1.0):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 3)) * spread).astype(np.float32), rng.integers(0, 256, (n, 3)).astype(np.uint8)


def test_one_point_and_one_voxel():
    check(np.array([[1.5, -2.25, 3.0]], np.float32), np.array([[9, 8, 7]], np.uint8), 0.25)
    p, c = scene(300, 1, spread=0.001)
    got = check(p, c, 1.0)
    assert got["centers"].shape[0] == 1 and int(got["counts"][0]) == 300
    got = check(np.zeros((2, 3), np.float32), np.array([[254] * 3, [255] * 3], np.uint8), 0.5)
    assert got["colors"].tolist() == [[254, 254, 254]]                  # the mean 254.5 truncates


def test_coordinates_that_are_exact_multiples_of_the_voxel_size():
    rng = np.random.default_rng(2)
    p = (rng.integers(-20, 20, (700, 3)) * 0.25).astype(np.float32)
    got = check(p, rng.integers(0, 256, (700, 3)).astype(np.uint8), 0.25)
    assert got["counts"].max() > 1 and torch.equal(got["centers"], got["voxel_index"].float() * 0.25 + got["min_corner"])


def test_keep_masks_that_leave_one_point_and_none():
    p, c = scene(400, 3)
    keep = np.zeros(400, np.uint8)
    none = check(p, c, 0.1, keep=keep)
    assert none["centers"].shape[0] == 0 and torch.isinf(none["min_corner"]).all()
    keep[123] = 1
    one = check(p, c, 0.1, keep=keep)
    assert one["centers"].cpu().numpy().tobytes() == p[123].tobytes() and int(one["point_voxel"][123]) == 0
    check(p, c, 0.1, keep=np.random.default_rng(4).integers(0, 2, 400).astype(np.uint8))


def test_five_thousand_points_two_runs_and_a_recycled_workspace():
    import voxproj_host
    p, c = scene(5000, 5, spread=0.4)
    ws = voxproj_host.SplatWorkspace()
    a = check(p, c, 0.05, workspace=ws)
    assert 1000 < a["centers"].shape[0] < 5000
    check(*scene(257, 6), 0.3, workspace=ws)                           # a smaller call on the same buffer in between
    b = check(p, c, 0.05, workspace=ws)
    assert all(torch.equal(a[k], b[k]) for k in ("centers", "colors", "counts", "voxel_index", "point_voxel"))


def test_seventy_thousand_points_take_the_min_reduction_round_twice():
    """k_grid_min_part runs min(ceil(N / 256), GRID_PARTS = 256) workgroups of 256 lanes and strides by gridDim * 256: a lane
    takes a second point iff N > 256 * 256 = 65 536.  N = 70 001: the points 65 536.. are second-lap points (the last workgroup
    to get one is 17, its lanes 113.. get none).  The minimum of every axis is attained by one second-lap point alone, a
    different one per axis; first-lap points below those minima are not kept; the sort and the scan see 70 001 keys."""
    import voxproj_host
    N, LAP = 70001, 256 * 256
    rng = np.random.default_rng(9)
    p = np.clip(rng.normal(size=(N, 3)) * 0.5, -2.0, 2.0).astype(np.float32)
    c = rng.integers(0, 256, (N, 3)).astype(np.uint8)
    lows = {LAP + 7: (0, -3.25), 68000: (1, -3.5), N - 1: (2, -2.75)}
    for i, (axis, v) in lows.items():
        p[i, axis] = v
    keep = (rng.uniform(size=N) < 0.9).astype(np.uint8)
    keep[LAP:] = 1
    dropped = np.flatnonzero(keep[:LAP] == 0)[:50]
    p[dropped] = rng.uniform(-6.0, -4.0, (50, 3)).astype(np.float32)   # below every kept point: the mask decides the corner
    assert (keep[:LAP] == 0).sum() > 5000
    ws = voxproj_host.SplatWorkspace()
    got = check(p, c, 0.05, keep=keep, workspace=ws)
    assert got["min_corner"].tolist() == [-3.25, -3.5, -2.75] and 20000 < got["centers"].shape[0] < N
    assert int(got["counts"].sum()) == int(keep.sum()) and (got["point_voxel"][LAP:] >= 0).all()
    # the status word: one non-finite kept point in the second lap refuses the call; not kept, it is a point like any dropped one
    bad = p.copy()
    bad[66000, 1] = np.nan
    check(bad, c, 0.05, keep=keep, workspace=ws)
    off = keep.copy()
    off[66000] = 0
    check(bad, c, 0.05, keep=off, workspace=ws)
    check(p, c, 0.05, workspace=ws)                                     # and without a mask: the dropped points set the corner


def test_status_cases_leave_the_next_call_alone():
    import voxproj_host
    ws = voxproj_host.SplatWorkspace()
    p, c = scene(600, 7)
    far = p.copy()
    far[17, 0] = far[:, 0].min() + 0.01 * 2.0 ** 21                    # cell index 2^21: one past the key's range
    check(far, c, 0.01, workspace=ws)
    near = p.copy()
    near[:, 0] = np.clip(near[:, 0], -1.0, 1.0)
    near[17, 0] = near[:, 0].min() + 2.0 ** 21 - 1                     # the last cell that fits
    ok = check(near, c, 1.0, workspace=ws)
    assert int(ok["voxel_index"][:, 0].max()) == 2 ** 21 - 1
    nan = p.copy()
    nan[300, 1] = np.nan
    check(nan, c, 0.1, workspace=ws)
    inf = p.copy()
    inf[5, 2] = np.inf
    check(inf, c, 0.1, workspace=ws)
    check(nan, c, 0.1, keep=(np.arange(600) != 300), workspace=ws)     # the NaN point is not kept: a valid call
    check(p, c, 0.1, workspace=ws)


def test_a_workspace_one_byte_short_is_refused_on_the_host():
    import voxproj_host
    L = voxproj_host.lib()
    N = 1000
    need = voxproj_host.voxel_grid_workspace_bytes(N)
    assert need > N * 36 and voxproj_host.voxel_grid_workspace_bytes(0) > 0
    buf = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    ptr = (buf.data_ptr() + 255) & ~255
    P = 0x7000_0000_0000                                               # never dereferenced: the call is refused before any launch
    args = (P, P, None, N, 0.1, P, P, P, P, P, P, P, None, ptr)
    assert L.vp_voxel_grid(*args, need - 1, None) == -2 and b"workspace has" in L.vp_last_error()
    p, c = scene(N, 8)
    t = {k: torch.empty(s, dtype=d, device=DEV) for k, s, d in (("cen", (N, 3), torch.float32), ("col", (N, 3), torch.uint8), ("cnt", N, torch.int32),
                                                                 ("idx", (N, 3), torch.int32), ("pv", N, torch.int32), ("nv", 1, torch.int32),
                                                                 ("mc", 3, torch.float32))}
    pd, cd = _dev(p), _dev(c)
    rc = L.vp_voxel_grid(pd.data_ptr(), cd.data_ptr(), None, N, 0.1, t["cen"].data_ptr(), t["col"].data_ptr(), t["cnt"].data_ptr(), t["idx"].data_ptr(),
                         t["pv"].data_ptr(), t["nv"].data_ptr(), t["mc"].data_ptr(), None, ptr, need, torch.cuda.current_stream(DEV).cuda_stream)
    assert rc == 0 and int(t["nv"].item()) == len(vg.voxelize(p, c, 0.1)["centers"])        # exactly the stated size is enough; status may be NULL


def test_no_points():
    import voxproj_host
    got = voxproj_host.voxel_grid(torch.zeros((0, 3), device=DEV), torch.zeros((0, 3), dtype=torch.uint8, device=DEV), 0.1)
    assert got["centers"].shape == (0, 3) and int(got["n_voxels"].item()) == 0 and int(got["status"].item()) == 0
