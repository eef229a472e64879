"""CPU-side checks of stage 2 (include/voxproj_grid.h): the NumPy twin of tests/voxel_grid_reference.py against scipy's
cKDTree and against the reference script's own output (tests/golden/voxel_grid_golden.npz), the fourth signature table
against its header, the entry points' host-side refusals and the command line's parser.  No device call is made here."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

import voxel_grid_reference as vg
from test_abi_cpu import _binding_error          # the comparison of a ctypes binding with a C prototype, written once

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_voxel_grid_golden as mk  # noqa: E402  (the inputs of the fixture, rebuilt from the seed; the reference is not read)


def lattice(n, spacing):
    k = np.arange(n, dtype=np.float64) * spacing
    return np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


# ---- the twin's ball counts against cKDTree ----
def _tree_counts(points, r):
    from scipy.spatial import cKDTree
    p = points.astype(np.float64)
    return np.asarray(cKDTree(p).query_ball_point(p, r=r, return_length=True))


def test_twin_ball_counts_equal_ckdtree_on_a_random_cloud():
    pts = np.random.default_rng(0).uniform(size=(3000, 3)).astype(np.float32)
    count, _, gap = vg.ball_stats(pts, 0.05, want_gap=True)
    print(f"scalar radius: nearest |d2 - r^2| = {gap:.3e}, mean count {count.mean():.2f}")
    assert gap >= 1e-9
    assert np.array_equal(count, _tree_counts(pts, 0.05)) and count.min() >= 1 and count.max() > 5
    radii = np.random.default_rng(1).uniform(0.02, 0.08, 3000).astype(np.float32)
    count, _, gap = vg.ball_stats(pts, radii, want_gap=True)
    print(f"per-point radii: nearest |d2 - r^2| = {gap:.3e}")
    assert gap >= 1e-9
    assert np.array_equal(count, _tree_counts(pts, radii.astype(np.float64)))


@pytest.mark.parametrize("r", [1 / 8, 0.125 * np.sqrt(2), 1 / 4])
def test_twin_ball_counts_equal_ckdtree_on_a_lattice_with_points_on_the_boundary(r):
    """8 x 8 x 8 points of spacing 1/8: every squared distance is a multiple of 1/64, exact in float64, and points lie exactly
    on the sphere, so the <= of the contract decides the count."""
    pts = lattice(8, 1 / 8)
    count, _ = vg.ball_stats(pts, float(r))
    inner = count[np.all((pts > 0.3) & (pts < 0.6), axis=1)]
    print(f"r = {r!r}: interior count {sorted(set(inner.tolist()))}")
    assert np.array_equal(count, _tree_counts(pts, float(r)))
    if r in (1 / 8, 1 / 4):
        assert set(inner.tolist()) == {7 if r == 1 / 8 else 33}            # the 6 / 32 boundary-and-inner neighbours and the point


def test_twin_counts_with_normals_and_queries():
    rng = np.random.default_rng(3)
    pts = rng.uniform(size=(400, 3)).astype(np.float32)
    nrm = vg.unit_normals(rng.normal(size=(400, 3)).astype(np.float32))
    cnt, con = vg.ball_stats(pts, 0.2, normals=nrm, min_dot=-1.0)
    cnt2, con2 = vg.ball_stats(pts, 0.2, normals=nrm, min_dot=0.0)
    assert np.array_equal(cnt, cnt2) and (con2 <= con).all() and (con <= cnt).all() and (con2 >= 1).all()     # the point itself: dot ~ 1
    far = np.array([[50.0, 50.0, 50.0], [0.5, 0.5, 0.5]], np.float32)
    cnt, _ = vg.ball_stats(pts, np.array([1.0, 2.0], np.float32), queries=far)
    assert cnt.tolist() == [0, 400]
    assert np.array_equal(vg.unit_normals(np.zeros((2, 3), np.float32)), np.zeros((2, 3), np.float32))


# ---- the twin's pipeline against the reference script's output ----
@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "voxel_grid_golden.npz"))
    cols = mk.inputs()
    for k, v in mk.checksums(cols).items():
        assert v == g[f"checksum_{k}"], f"the rebuilt input column {k} is not the one the fixture was made from"
    return g, cols


@pytest.mark.parametrize("run", ["fixed", "adaptive", "normals"])
def test_twin_pipeline_reproduces_the_reference_script(golden, run):
    g, cols = golden
    r = vg.pipeline(cols["xyz"], cols["opacity"], cols["scales"], cols["f_dc"], cols["normals"] if mk.WITH_NORMALS[run] else None,
                    **mk.RUNS[run])
    V = len(g[f"{run}_xyz"])
    assert V > 1000 and r["survivors"]["spikiness"] < 6000 and r["survivors"]["density"] < r["survivors"]["opacity"]
    assert r["centers"].tobytes() == g[f"{run}_xyz"].tobytes() and r["colors"].tobytes() == g[f"{run}_rgb"].tobytes()
    assert np.array_equal(r["min_corner"], g[f"{run}_origin"].astype(np.float32)) and float(g[f"{run}_voxel_size"]) == 0.05
    assert f"_{V}vox_" in str(g[f"{run}_name"])
    if run == "adaptive":
        radii = vg.adaptive_radii(cols["scales"], 0.1)
        assert len(np.unique(radii)) > 100 and np.float32(0.05) <= radii.min() < radii.max() == np.float32(0.2)
        assert vg.adaptive_radii(np.array([[0.01, -0.02, 0.03], [-3.0, -4.0, -5.0], [0.125, 0.125, 0.125]], np.float32), 0.1).tolist() == \
            [np.float32(0.05), np.float32(0.2), np.float32(0.125)]
    if run == "normals":
        assert r["survivors"]["normal_consistency"] < r["survivors"]["opacity"]


def test_twin_voxelize_edge_cases_and_errors():
    one = vg.voxelize(np.array([[1.0, 2.0, 3.0]], np.float32), np.array([[9, 8, 7]], np.uint8), 0.25)
    assert one["centers"].tolist() == [[1.0, 2.0, 3.0]] and one["colors"].tolist() == [[9, 8, 7]] and one["point_voxel"].tolist() == [0]
    two = vg.voxelize(np.zeros((2, 3), np.float32), np.array([[254] * 3, [255] * 3], np.uint8), 1.0)
    assert two["colors"].tolist() == [[254, 254, 254]] and two["counts"].tolist() == [2]             # the mean 254.5 truncates
    none = vg.voxelize(np.zeros((2, 3), np.float32), np.zeros((2, 3), np.uint8), 1.0, keep=[0, 0])
    assert len(none["centers"]) == 0 and none["status"] == 0 and none["point_voxel"].tolist() == [-1, -1]
    big = vg.voxelize(np.array([[0, 0, 0], [2.0 ** 21, 0, 0]], np.float32), np.zeros((2, 3), np.uint8), 1.0)
    ok = vg.voxelize(np.array([[0, 0, 0], [2.0 ** 21 - 1, 0, 0]], np.float32), np.zeros((2, 3), np.uint8), 1.0)
    nan = vg.voxelize(np.array([[0, 0, 0], [np.nan, 0, 0]], np.float32), np.zeros((2, 3), np.uint8), 1.0)
    assert big["status"] == 1 and nan["status"] == 1 and ok["status"] == 0 and ok["voxel_index"].tolist() == [[0, 0, 0], [2 ** 21 - 1, 0, 0]]
    cols = mk.inputs()
    with pytest.raises(ValueError, match="the density filter left no Gaussian"):
        vg.pipeline(cols["xyz"][:300], cols["opacity"][:300], cols["scales"][:300], cols["f_dc"][:300], density_eps=1e-4)
    with pytest.raises(ValueError, match="the normal consistency filter left no Gaussian"):
        vg.pipeline(cols["xyz"][:300], cols["opacity"][:300], cols["scales"][:300], cols["f_dc"][:300], np.zeros((300, 3), np.float32))


# ---- the fourth signature table against include/voxproj_grid.h ----
def _grid_prototypes():
    """{name: (return type, [parameter type, ...])} of every vp_* prototype of include/voxproj_grid.h, ``const`` and
    parameter names dropped; a pointer type ends in `` *``."""
    txt = open(os.path.join(ROOT, "include", "voxproj_grid.h")).read()
    txt = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))

    def ctype(decl, named):
        words = [w for w in decl.replace("*", " ").split() if w != "const"]
        return " ".join(words[:-1] if named else words) + (" *" if "*" in decl else "")

    return {name: (ctype(ret, False), [ctype(q, True) for q in params.split(",")])
            for ret, name, params in re.findall(r"([A-Za-z_][\w \t]*?[\s\*]+)(vp_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", txt)}


def test_grid_header_matches_the_fourth_signature_table():
    import voxproj_host
    voxproj_host.build()
    protos = _grid_prototypes()
    assert sorted(protos) == sorted(voxproj_host.EXPORTS_GRID) == ["vp_ball_count", "vp_voxel_grid", "vp_voxel_grid_workspace_bytes"]
    assert len(voxproj_host.EXPORTS) == 64 and len(voxproj_host.EXPORTS_EXT) == 2 and len(voxproj_host.EXPORTS_MESH) == 3
    assert voxproj_host.VP_ABI_VERSION == 4
    assert not set(voxproj_host.EXPORTS_GRID) & (set(voxproj_host.EXPORTS) | set(voxproj_host.EXPORTS_EXT) | set(voxproj_host.EXPORTS_MESH))
    L = voxproj_host.lib()
    for name, proto in protos.items():
        fn = getattr(L, name)
        assert _binding_error(proto, fn.restype, fn.argtypes) is None, (name, _binding_error(proto, fn.restype, fn.argtypes))
    proto, good = protos["vp_ball_count"], list(L.vp_ball_count.argtypes)
    assert len(good) == 18 and proto[1][9] == "int64_t" and proto[1][10] == "double" and good[3] is ctypes.POINTER(ctypes.c_double)
    assert "argument 10 is double" in _binding_error(proto, ctypes.c_int, good[:10] + [ctypes.c_float] + good[11:])
    assert "takes 18 arguments, bound with 17" in _binding_error(proto, ctypes.c_int, good[:-1])


def test_entry_points_validate_on_the_host_before_any_launch():
    """Fake device addresses that are never dereferenced: every refusal is host arithmetic."""
    import voxproj_host
    L = voxproj_host.lib()
    P = 0x7000_0000_0000
    origin = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    bad_origin = (ctypes.c_double * 3)(0.0, float("inf"), 0.0)
    base = dict(pts=P, perm=P + 4096, start=P + 8192, g=origin, h=0.1, nx=4, ny=4, nz=4, q=P + 12288, M=100, r=0.05, radii=None,
                pn=None, qn=None, dot=0.9, count=P + 16384, con=P + 20480)

    def ball(**kw):
        a = dict(base, **kw)
        return L.vp_ball_count(a["pts"], a["perm"], a["start"], a["g"], a["h"], a["nx"], a["ny"], a["nz"], a["q"], a["M"], a["r"],
                               a["radii"], a["pn"], a["qn"], a["dot"], a["count"], a["con"], None)

    for kw, msg in ((dict(pts=None), b"null pointer"), (dict(perm=None), b"null pointer"), (dict(start=None), b"null pointer"),
                    (dict(g=None), b"null pointer"), (dict(q=None), b"null pointer"), (dict(count=None), b"null pointer"),
                    (dict(M=-1), b"M = -1 outside [0, 2^31 - 1]"), (dict(M=1 << 31), b"M = 2147483648"), (dict(h=0.0), b"bad grid"),
                    (dict(h=float("nan")), b"bad grid"), (dict(nx=0), b"bad grid"), (dict(nx=2048, ny=2048, nz=512), b">= 2^31 cells"),
                    (dict(g=bad_origin), b"grid_origin3[1] is not finite"), (dict(r=-0.1), b"radius = -0.1 must be"),
                    (dict(r=float("inf")), b"radius = inf"), (dict(r=float("nan")), b"radius = nan"),
                    (dict(pn=P + 24576), b"normals for only one side"), (dict(qn=P + 24576), b"normals for only one side"),
                    (dict(pn=P + 24576, qn=P + 28672, con=None), b"consistent, with normals"),
                    (dict(pn=P + 24576, qn=P + 28672, dot=float("nan")), b"min_dot is NaN")):
        assert ball(**kw) == -1, kw
        assert msg in L.vp_last_error(), (kw, L.vp_last_error())
    assert ball(M=0) == 0 and ball(M=0, r=-1.0, radii=P + 32768) == 0          # nothing to do is valid; radii replace the radius

    gbase = dict(p=P, c=P + 4096, keep=None, N=100, vs=0.05, cen=P + 8192, col=P + 12288, cnt=P + 16384, idx=P + 20480, pv=P + 24576,
                 nv=P + 28672, mc=P + 32768, st=None, ws=P + 36864, wb=1 << 30)

    def grid(**kw):
        a = dict(gbase, **kw)
        return L.vp_voxel_grid(a["p"], a["c"], a["keep"], a["N"], a["vs"], a["cen"], a["col"], a["cnt"], a["idx"], a["pv"], a["nv"],
                               a["mc"], a["st"], a["ws"], a["wb"], None)

    for kw, code, msg in ((dict(N=-1), -1, b"N = -1 outside [0, 2^31 - 1]"), (dict(N=1 << 31), -1, b"N = 2147483648"),
                          (dict(vs=0.0), -1, b"voxel_size = 0 must be"), (dict(vs=-1.0), -1, b"voxel_size"), (dict(vs=float("nan")), -1, b"voxel_size"),
                          (dict(vs=float("inf")), -1, b"voxel_size"), (dict(vs=1e-60), -1, b"in float32 too"), (dict(p=None), -1, b"null pointer"),
                          (dict(c=None), -1, b"null pointer"), (dict(cen=None), -1, b"null pointer"), (dict(pv=None), -1, b"null pointer"),
                          (dict(nv=None), -1, b"n_voxels or min_corner"), (dict(mc=None), -1, b"n_voxels or min_corner"),
                          (dict(ws=None), -2, b"workspace is NULL"), (dict(ws=P + 36865), -2, b"256-byte aligned")):
        assert grid(**kw) == code, kw
        assert msg in L.vp_last_error(), (kw, L.vp_last_error())
    assert L.vp_voxel_grid_workspace_bytes(-1) == 0 and L.vp_voxel_grid_workspace_bytes(1 << 31) == 0


def test_host_wrappers_refuse_bad_arguments_before_any_device_call(monkeypatch):
    import torch

    import voxproj_host

    def no_call(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(voxproj_host, "_call", no_call)
    p = torch.zeros(5, 3)
    with pytest.raises(ValueError, match="points must be a CUDA tensor: there is no CPU path"):
        voxproj_host.ball_count(p, 0.1)
    with pytest.raises(ValueError, match="points must be a CUDA tensor: there is no CPU path"):
        voxproj_host.voxel_grid(p, torch.zeros(5, 3, dtype=torch.uint8), 0.1)
    with pytest.raises(ValueError, match="points must be torch.float32"):
        voxproj_host.ball_count(p.double(), 0.1)
    monkeypatch.setattr(voxproj_host, "_require_tensors", lambda *specs: None)
    for args, kw, msg in (((torch.zeros(5, 2), 0.1), {}, r"points must be float32 \[M, 3\]"), ((p, -0.1), {}, "radius = -0.1 must be"),
                          ((p, float("inf")), {}, "radius = inf must be"), ((p, torch.zeros(4)), {}, r"radii must be float32 \[5\]"),
                          ((p, 0.1), dict(normals=p), "normals and min_dot go together"),
                          ((p, 0.1), dict(queries=p, normals=p, min_dot=0.5), "need query_normals"),
                          ((p, 0.1), dict(query_normals=p), "query_normals without normals")):
        with pytest.raises(ValueError, match=msg):
            voxproj_host.ball_count(*args, **kw)
    for colors, vs, keep, msg in ((torch.zeros(4, 3, dtype=torch.uint8), 0.1, None, r"colors must be uint8 \[5, 3\]"),
                                  (torch.zeros(5, 3, dtype=torch.uint8), 0.0, None, "voxel_size = 0.0 must be"),
                                  (torch.zeros(5, 3, dtype=torch.uint8), 0.1, torch.zeros(4, dtype=torch.uint8), r"keep must be uint8 or bool \[5\]")):
        with pytest.raises(ValueError, match=msg):
            voxproj_host.voxel_grid(p, colors, vs, keep=keep)
    import build_voxel_grid as bvg
    with pytest.raises(ValueError, match="needs a GPU: there is no CPU path"):
        bvg.build_voxel_grid(dict(xyz=np.zeros((3, 3), np.float32)), device="cpu")


# ---- the bucketing's optional minimum cell ----
def test_bucket_minimum_cell_size_leaves_the_default_alone():
    import torch

    import voxel_to_gaussian_map as v2g
    pts = torch.from_numpy(np.random.default_rng(2).uniform(size=(500, 3)).astype(np.float32))
    a, b = v2g._bucket(pts, torch.device("cpu")), v2g._bucket(pts, torch.device("cpu"), min_cell=None)
    assert a[4] == b[4] and a[5] == b[5] and torch.equal(a[1], b[1])
    small = v2g._bucket(pts, torch.device("cpu"), min_cell=a[4] / 4)
    assert small[4] == a[4] and small[5] == a[5]
    big = v2g._bucket(pts, torch.device("cpu"), min_cell=0.5)
    assert big[4] == 0.5 and max(big[5]) <= 2 and int(big[2][-1]) == 500


# ---- the command line ----
def test_cli_parser_has_the_reference_flags_and_defaults(tmp_path):
    import build_voxel_grid as bvg
    spec = json.load(open(os.path.join(GOLDEN, "voxel_grid_cli.json")))
    ap = bvg.build_parser()
    a = ap.parse_args(["--ply", "p.ply"])
    want = dict(spec["flags"], **spec["added_here"])
    assert {k: getattr(a, k) for k in want if k != "ply"} == {k: v for k, v in want.items() if k != "ply"}
    assert sorted(vars(a)) == sorted(want) and a.ply == "p.ply"
    assert {k: v for k, v in bvg.DEFAULTS.items()} == {k: v for k, v in spec["flags"].items() if k not in ("ply", "output_dir")}
    with pytest.raises(SystemExit):
        ap.parse_args([])                                                       # --ply is required
    a = ap.parse_args(["--ply", "p", "--adaptive_density", "--activated", "--cell_size", "0.03", "--density_min_neighbors", "4"])
    assert a.adaptive_density and a.activated and a.cell_size == 0.03 and a.density_min_neighbors == 4
    # the reference's naming rule, and a file that reads back as the same float32
    name = bvg.grid_file_name(os.path.join("data", "room0", "point_cloud", "iteration_7000", "point_cloud.ply"), 1746, 0.5, 0.05, 0.1, 4)
    assert name == "room0_minkowski_1746vox_iter_opac0.5_cell0.05_eps0.1_neig4_grid.ply"
    assert bvg.grid_file_name(os.path.join("a", "b", "c", "iteration_30.ply"), 7, 0.9, 0.05, 0.05, 10).startswith("b_minkowski_7vox_iter30_")
    import build_sparse_occupancy as bso
    rng = np.random.default_rng(4)
    xyz = (rng.normal(size=(50, 3)) * 10.0 ** rng.integers(-6, 6, (50, 1))).astype(np.float32)
    rgb = rng.integers(0, 256, (50, 3)).astype(np.uint8)
    path = str(tmp_path / name)
    bvg.write_grid_ply(path, xyz, rgb, 0.05, xyz[0])
    vs, origin, shape, n_name = bso.extract_voxel_params(path)
    assert vs == 0.05 and shape is None and n_name == 1746 and np.array_equal(np.array(origin, np.float32), xyz[0])
    assert bso.read_voxel_ply(path).tobytes() == xyz.tobytes()
    _, _, xyz2, rgb2 = mk.parse_grid_ply(path)
    assert xyz2.tobytes() == xyz.tobytes() and np.array_equal(rgb2, rgb)
    head = open(path).read().split("end_header")[0].split("\n")
    assert head[:3] == ["ply", "format ascii 1.0", "comment voxel_size 0.05"] and head[3].startswith("comment grid_origin ")
    assert head[4:11] == ["element vertex 50", "property float x", "property float y", "property float z", "property uchar red",
                          "property uchar green", "property uchar blue"]
