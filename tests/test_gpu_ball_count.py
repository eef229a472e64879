"""vp_ball_count on the GPU against the NumPy twin (tests/voxel_grid_reference.py): integer equality for every query, and two
runs equal to each other."""
import numpy as np
import pytest
import torch

import voxel_grid_reference as vg
from test_voxel_grid_cpu import lattice

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check(points, radius, queries=None, normals=None, query_normals=None, min_dot=None):
    import voxproj_host
    want_cnt, want_con = vg.ball_stats(points, radius, queries=queries, normals=normals, query_normals=query_normals, min_dot=min_dot)
    r = _dev(np.asarray(radius, np.float32)) if np.ndim(radius) else float(radius)
    runs = [voxproj_host.ball_count(_dev(points), r, queries=_dev(queries), normals=_dev(normals), query_normals=_dev(query_normals),
                                    min_dot=min_dot) for _ in range(2)]
    (cnt, con), (cnt2, con2) = [(c.cpu().numpy(), None if k is None else k.cpu().numpy()) for c, k in runs]
    assert cnt.dtype == np.int32 and np.array_equal(cnt, cnt2) and np.array_equal(cnt, want_cnt)
    if normals is None:
        assert con is None and con2 is None
    else:
        assert np.array_equal(con, con2) and np.array_equal(con, want_con)
    return cnt, con


def cloud(n, seed):
    return np.random.default_rng(seed).uniform(size=(n, 3)).astype(np.float32)


def test_one_point_and_coincident_points():
    assert check(np.array([[0.3, -2.0, 5.0]], np.float32), 0.05)[0].tolist() == [1]
    assert check(np.array([[0.3, -2.0, 5.0]], np.float32), 0.0)[0].tolist() == [1]
    assert check(np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0]], np.float32), 0.0)[0].tolist() == [2, 2]


@pytest.mark.parametrize("n", [257, 1000])
def test_random_clouds(n):
    cnt, _ = check(cloud(n, n), 0.12)
    assert cnt.max() > 3
    check(cloud(n, n + 1), np.random.default_rng(n).uniform(0.02, 0.3, n).astype(np.float32))


@pytest.mark.parametrize("r", [1 / 8, 0.125 * np.sqrt(2), 1 / 4])
def test_lattice_with_points_exactly_on_the_boundary(r):
    cnt, _ = check(lattice(8, 1 / 8), float(r))
    assert cnt.max() == {1 / 8: 7, 1 / 4: 33}.get(r, cnt.max())


def test_radii_that_mix_zero_with_one_larger_than_the_cloud():
    pts = cloud(500, 7)
    radii = np.where(np.arange(500) % 3 == 0, 0.0, 5.0).astype(np.float32)
    radii[1] = 0.07
    cnt, _ = check(pts, radii)
    assert set(cnt[radii == 0.0].tolist()) == {1} and set(cnt[radii == 5.0].tolist()) == {500}


def test_queries_that_are_not_the_points_some_far_outside():
    pts = cloud(700, 11)
    rng = np.random.default_rng(12)
    q = np.concatenate([rng.uniform(size=(300, 3)), rng.uniform(-40, 40, (60, 3)), [[1.05, 0.5, 0.5], [-0.04, -0.04, -0.04], [1e30, 0, 0]]]).astype(np.float32)
    cnt, _ = check(pts, 0.1, queries=q)
    assert cnt[:300].max() > 1 and cnt[-1] == 0
    check(pts, rng.uniform(0.0, 0.4, len(q)).astype(np.float32), queries=q)
    nrm, qn = vg.unit_normals(rng.normal(size=(700, 3)).astype(np.float32)), vg.unit_normals(rng.normal(size=(len(q), 3)).astype(np.float32))
    check(pts, 0.2, queries=q, normals=nrm, query_normals=qn, min_dot=0.0)


def test_a_cloud_in_one_plane():
    pts = cloud(600, 13)
    pts[:, 2] = 0.25
    check(pts, 0.06)
    pts[:, 1] = -1.0                                       # and on one line
    check(pts, 0.01)


def test_a_crowded_bucket_cell_beside_a_sparse_remainder():
    rng = np.random.default_rng(17)
    pts = np.concatenate([rng.uniform(0.5, 0.501, (600, 3)), rng.uniform(0, 4, (150, 3))]).astype(np.float32)
    cnt, _ = check(pts, 0.002)
    assert cnt[:600].min() >= 600
    check(pts, 0.3)


@pytest.mark.parametrize("min_dot", [0.9, 0.0, -1.0])
def test_normals_with_zero_vectors_among_them(min_dot):
    rng = np.random.default_rng(19)
    pts = cloud(800, 19)
    raw = rng.normal(size=(800, 3)).astype(np.float32)
    raw[::7] = 0.0
    raw[1::7] = np.array([0.0, 0.0, 2.0], np.float32)      # equal normals: dot = 1 up to the rounding of 1e-8
    cnt, con = check(pts, 0.15, normals=vg.unit_normals(raw), min_dot=min_dot)
    assert (con <= cnt).all() and con.max() >= 1
    if min_dot == -1.0:
        assert con[::7].tolist() == cnt[::7].tolist()     # a zero normal: every dot is 0 > -1


def test_empty_sets():
    import voxproj_host
    none, some = torch.zeros((0, 3), device=DEV), _dev(cloud(5, 1))
    assert voxproj_host.ball_count(none, 0.1)[0].numel() == 0
    assert voxproj_host.ball_count(none, 0.1, queries=some)[0].tolist() == [0] * 5
    assert voxproj_host.ball_count(some, 0.1, queries=none)[0].numel() == 0
