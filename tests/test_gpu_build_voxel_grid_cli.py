"""build_voxel_grid.py end to end on the GPU: the command line on the golden fixture's input reproduces the reference
script's output files, on a synthetic_gaussians scene it equals the NumPy twin, and the written file goes through the
stage-4 loader (build_sparse_occupancy) as exactly the grid's cells."""
import os
import sys

import numpy as np
import pytest
import torch

import voxel_grid_reference as vg

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_voxel_grid_golden as mk  # noqa: E402  (inputs and file helpers of the fixture; the reference is not read)


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "voxel_grid_golden.npz"))
    cols = mk.inputs()
    for k, v in mk.checksums(cols).items():
        assert v == g[f"checksum_{k}"], f"the rebuilt input column {k} is not the one the fixture was made from"
    return g, cols


def _run_cli(ply, out_dir, args, capsys):
    import build_voxel_grid as bvg
    path = bvg.main(["--ply", ply, "--output_dir", out_dir, "--device", "cuda:0"] + args)
    out = capsys.readouterr().out
    assert os.path.dirname(path) == out_dir and os.listdir(out_dir) == [os.path.basename(path)]
    assert out.strip().endswith(f"[INFO] Saved sparse voxel grid to {path}")
    return path, out


@pytest.mark.parametrize("run", ["fixed", "adaptive", "normals"])
def test_cli_reproduces_the_reference_script_on_the_golden_input(golden, run, tmp_path, capsys):
    g, cols = golden
    ply = mk.scene_ply(str(tmp_path), "golden_" + run)
    mk.write_input_ply(ply, cols, mk.WITH_NORMALS[run])
    path, out = _run_cli(ply, str(tmp_path / "out"), mk.cli_args(ply, "x", run)[4:], capsys)
    assert os.path.basename(path) == str(g[f"{run}_name"])
    vs, origin, xyz, rgb = mk.parse_grid_ply(path)
    assert vs == float(g[f"{run}_voxel_size"]) and np.array_equal(origin.astype(np.float32), g[f"{run}_origin"].astype(np.float32))
    assert xyz.tobytes() == g[f"{run}_xyz"].tobytes() and rgb.tobytes() == g[f"{run}_rgb"].tobytes()
    assert "[INFO] Loaded input PLY with 6000 points." in out and "Filtered out 179 spiky Gaussians (ratio > 10.0)" in out
    assert "[INFO] Filtered to 2910 points with top 50% opacity (N=2910 of 5821)" in out
    assert f"[INFO] Sparse voxel grid: {len(xyz)} voxels" in out and "Using specified voxel size: 0.050000" in out
    assert ("Adaptive density: Kept" in out) == (run == "adaptive") and ("Filtering by normal consistency" in out) == (run == "normals")


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    import gaussian_ply
    import synthetic_gaussians as sg
    g = sg.make_gaussians(4000, room=(1.5, 1.2, 1.0), seed=9)
    op, ls, rot = sg.to_ply_fields(g)
    f_dc = np.random.default_rng(9).uniform(-0.2, 1.2, (4000, 3)).astype(np.float32)
    ply = mk.scene_ply(str(tmp_path_factory.mktemp("scene")), "room9")
    os.makedirs(os.path.dirname(ply))
    gaussian_ply.write_gaussian_ply(ply, g["means"], op, ls, rot, f_dc=f_dc)
    return ply


@pytest.mark.parametrize("adaptive", [False, True])
def test_cli_on_a_synthetic_scene_equals_the_twin_and_hands_over_to_stage_4(synthetic, adaptive, tmp_path, capsys):
    import build_sparse_occupancy as bso
    import build_voxel_grid as bvg
    opts = dict(cell_size=0.05, density_eps=0.1, density_min_neighbors=4, opacity_threshold=0.5, normal_consistency=1.0)
    args = [a for k, v in opts.items() for a in (f"--{k}", str(v))] + (["--adaptive_density"] if adaptive else [])
    path, _ = _run_cli(synthetic, str(tmp_path / "out"), args, capsys)
    cols = bvg.load_columns(synthetic)
    assert cols["normals"] is not None and not cols["normals"].any()                 # 3DGS writes zero normals
    want = vg.pipeline(cols["xyz"], cols["opacity"], cols["scales"], cols["f_dc"], cols["normals"], adaptive_density=adaptive, **opts)
    V = len(want["centers"])
    assert 500 < V and want["survivors"]["density"] < want["survivors"]["opacity"] == 2000
    _, origin, xyz, rgb = mk.parse_grid_ply(path)
    assert xyz.tobytes() == want["centers"].tobytes() and rgb.tobytes() == want["colors"].tobytes()
    assert np.array_equal(origin.astype(np.float32), want["min_corner"])
    # the function's own result, and the stage-4 hand-over of the written file
    got = bvg.build_voxel_grid(synthetic, adaptive_density=adaptive, device="cuda:0", **opts)
    assert {k: v for k, v in got["survivors"].items() if k != "voxels"} == want["survivors"] and got["survivors"]["voxels"] == V
    assert np.array_equal(got["kept"].cpu().numpy(), want["kept"]) and got["voxel_index"].cpu().numpy().tobytes() == want["voxel_index"].tobytes()
    vs, grid_origin, shape, n_name = bso.extract_voxel_params(path)
    assert vs == 0.05 and shape is None and n_name == V
    pts = bso.read_voxel_ply(path)
    assert pts.tobytes() == want["centers"].tobytes()
    coords, dims = bso.voxel_coords(pts, grid_origin, vs)
    assert np.array_equal(coords, want["voxel_index"]) and len(np.unique(coords, axis=0)) == V
    assert np.array_equal(dims, want["voxel_index"].max(axis=0) + 1)


def test_errors_name_the_filter(synthetic):
    import build_voxel_grid as bvg
    with pytest.raises(ValueError, match="the normal consistency filter left no Gaussian"):
        bvg.build_voxel_grid(synthetic, device="cuda:0")                             # zero normals at the default 0.9
    with pytest.raises(ValueError, match="the density filter left no Gaussian"):
        bvg.build_voxel_grid(synthetic, normal_consistency=1.0, density_eps=1e-5, device="cuda:0")
    cols = bvg.load_columns(synthetic, activated=True)
    raw = bvg.load_columns(synthetic)
    assert (cols["scales"] > 0).all() and np.allclose(np.log(cols["scales"]), raw["scales"], atol=1e-5) and (cols["opacity"] <= 1).all()
    got = bvg.build_voxel_grid(cols, normal_consistency=1.0, opacity_threshold=0.5, density_eps=0.1, density_min_neighbors=1, adaptive_density=True,
                               device="cuda:0")
    want = vg.pipeline(cols["xyz"], cols["opacity"], cols["scales"], cols["f_dc"], None, normal_consistency=1.0, opacity_threshold=0.5,
                       density_eps=0.1, density_min_neighbors=1, adaptive_density=True)
    assert got["survivors"]["spikiness"] == want["survivors"]["spikiness"] < 4000    # activated scales: the spikiness filter does remove
    assert got["centers"].cpu().numpy().tobytes() == want["centers"].tobytes() and got["colors"].cpu().numpy().tobytes() == want["colors"].tobytes()
