"""Generates tests/golden/voxel_grid_golden.npz by running the REFERENCE's own script/minkowski_voxel_grid_from_ply_advanced.py,
unmodified, in the build container on a seeded synthetic point cloud of 6000 Gaussians: two noisy planes, 200 far outliers,
distinct opacities, scale logs of both signs (so that the spikiness filter and the adaptive radius both vary) and, for one
of the three runs, non-zero normals.  The script imports ``plyfile``; a stand-in made of this repository's own ply reader is
put into sys.modules (PlyData.read(p)['vertex'] with item access and .data.dtype.names is all the script uses).
Runs: fixed density, --adaptive_density, normal consistency 0.9 with normals.  Stored: the parsed voxel rows and header
values of each run, the file names, and checksums of the inputs (the tests rebuild the inputs from the seed).
Usage: python tests/golden/make_voxel_grid_golden.py"""
import os
import runpy
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.join(ROOT, "3d-semantic-segmentation_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

REFERENCE_SCRIPT = "/root/reference/script/minkowski_voxel_grid_from_ply_advanced.py"
COMMON = dict(cell_size=0.05, density_eps=0.1, density_min_neighbors=4, opacity_threshold=0.5)
RUNS = {"fixed": dict(COMMON), "adaptive": dict(COMMON, adaptive_density=True),
        "normals": dict(COMMON, normal_consistency=0.9, normal_consistency_eps=0.1, normal_consistency_min_neighbors=5)}
WITH_NORMALS = {"fixed": False, "adaptive": False, "normals": True}
FIELDS = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2",
          "rot_0", "rot_1", "rot_2", "rot_3"]


def inputs(seed=28):
    """dict(xyz, opacity, scales, f_dc, normals), float32: the columns as a 3DGS ply stores them."""
    rng = np.random.default_rng(seed)
    n_a, n_b, n_out = 2900, 2900, 200
    a = np.stack([rng.uniform(0, 2, n_a), rng.uniform(0, 2, n_a), rng.normal(0, 0.004, n_a)], 1)            # floor z = 0
    b = np.stack([rng.normal(0, 0.004, n_b), rng.uniform(0, 2, n_b), rng.uniform(0, 1.5, n_b)], 1)          # wall x = 0
    out = rng.uniform(-10, 10, (n_out, 3))
    xyz = np.concatenate([a, b, out]).astype(np.float32)
    n = len(xyz)
    # normals from a finite set (the plane's normal tilted by one of four angles towards one of four azimuths), so that the
    # dot products of pairs take finitely many values, none of them near the threshold (check_dot_margin asserts it)
    tilt = rng.choice([0.0, 0.2, 0.35, 0.6], n)
    az = rng.choice(4, n) * (np.pi / 2)
    local = np.stack([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)], 1)               # about +z
    nrm = np.concatenate([local[:n_a], local[n_a:n_a + n_b][:, [2, 0, 1]], local[n_a + n_b:][:, [1, 2, 0]]])
    nrm = nrm * rng.uniform(0.5, 2.0, (n, 1))
    nrm[rng.permutation(n)[:60]] = 0.0                                                                      # zero normals among them
    opacity = rng.permutation(np.linspace(-6.0, 6.0, n)).astype(np.float32)
    assert len(np.unique(opacity)) == n, "the opacities must be distinct"
    scales = rng.normal(np.log(0.03), 0.5, (n, 3))
    kind = rng.uniform(size=n)
    pos = kind < 0.3                                           # all-positive logs: kept by the spikiness filter, varied radius
    scales[pos] = rng.uniform(0.04, 0.3, (int(pos.sum()), 3))
    spiky = (kind >= 0.3) & (kind < 0.33)                      # positive logs with a ratio above 10: removed
    scales[spiky] = rng.uniform(0.02, 0.05, (int(spiky.sum()), 3)) * np.array([1.0, 4.0, 30.0])
    f_dc = rng.uniform(-0.3, 1.3, (n, 3))
    perm = rng.permutation(n)
    cols = dict(xyz=xyz, opacity=opacity, scales=scales.astype(np.float32), f_dc=f_dc.astype(np.float32), normals=nrm.astype(np.float32))
    return {k: np.ascontiguousarray(v[perm]) for k, v in cols.items()}


def checksums(cols):
    return {k: np.float64(v.astype(np.float64).sum()) for k, v in cols.items()}


def write_input_ply(path, cols, with_normals):
    """The binary little-endian 3DGS point cloud of ``cols``; without normals the file has no nx ny nz columns at all."""
    fields = [f for f in FIELDS if with_normals or f not in ("nx", "ny", "nz")]
    n = len(cols["xyz"])
    rec = np.zeros(n, dtype=[(k, "<f4") for k in fields])
    for i, k in enumerate("xyz"):
        rec[k] = cols["xyz"][:, i]
        if with_normals:
            rec["n" + k] = cols["normals"][:, i]
    for i in range(3):
        rec[f"f_dc_{i}"] = cols["f_dc"][:, i]
        rec[f"scale_{i}"] = cols["scales"][:, i]
    rec["opacity"] = cols["opacity"]
    rec["rot_0"] = 1.0
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\n" + f"element vertex {n}\n".encode())
        f.write("".join(f"property float {k}\n" for k in fields).encode() + b"end_header\n")
        f.write(rec.tobytes())


def scene_ply(root, name):
    """Where a run's input goes: <root>/<name>/point_cloud/iteration_7000/point_cloud.ply (the scene is <name>)."""
    return os.path.join(root, name, "point_cloud", "iteration_7000", "point_cloud.ply")


def cli_args(ply, out_dir, run):
    args = ["--ply", ply, "--output_dir", out_dir]
    for k, v in RUNS[run].items():
        args += [f"--{k}"] if v is True else [f"--{k}", str(v)]
    return args


def parse_grid_ply(path):
    """(voxel_size, grid_origin f64 [3], xyz f32 [V,3], rgb u8 [V,3]) of a written grid file."""
    with open(path) as f:
        lines = f.read().split("\n")
    end = lines.index("end_header")
    vs = [float(ln.split()[-1]) for ln in lines[:end] if ln.startswith("comment voxel_size")][0]
    origin = [[float(v) for v in ln.split()[-3:]] for ln in lines[:end] if ln.startswith("comment grid_origin")][0]
    rows = np.array([ln.split() for ln in lines[end + 1:] if ln], dtype=np.float64).reshape(-1, 6)
    return vs, np.array(origin, np.float64), rows[:, :3].astype(np.float32), rows[:, 3:].astype(np.uint8)


def _plyfile_stand_in():
    import gaussian_ply

    class _Vertex:
        def __init__(self, data):
            self.data = data

        def __getitem__(self, key):
            return self.data[key]

    class PlyData:
        @staticmethod
        def read(path):
            return {"vertex": _Vertex(gaussian_ply.read_vertex_records(path))}

    mod = types.ModuleType("plyfile")
    mod.PlyData = PlyData
    return mod


def check_dot_margin(cols, run):
    """No normal dot product of a pair within the ball lies within 1e-5 of the threshold (the reference takes the dot in
    float32, the contract in float64: beyond that margin the two agree)."""
    import voxel_grid_reference as vg
    o = RUNS[run]
    alive = np.flatnonzero(vg.spikiness_keep(cols["scales"], 10.0))
    alive = alive[vg.opacity_rank(cols["opacity"][alive], o["opacity_threshold"])[0]]
    p, u = cols["xyz"][alive].astype(np.float64), vg.unit_normals(cols["normals"])[alive].astype(np.float64)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    dot = (u @ u.T)[d2 <= (o["normal_consistency_eps"] * 1.01) ** 2]
    gap = float(np.abs(dot - o["normal_consistency"]).min())
    assert gap > 1e-5, f"a normal dot product lies {gap:.2e} from the threshold: change the seed"
    return gap


def main():
    sys.modules["plyfile"] = _plyfile_stand_in()
    cols = inputs()
    print("dot margin", check_dot_margin(cols, "normals"))
    out = {f"checksum_{k}": v for k, v in checksums(cols).items()}
    with tempfile.TemporaryDirectory() as tmp:
        for run in RUNS:
            ply = scene_ply(tmp, "golden_" + run)
            write_input_ply(ply, cols, WITH_NORMALS[run])
            out_dir = os.path.join(tmp, "out_" + run)
            argv, sys.argv = sys.argv, [REFERENCE_SCRIPT] + cli_args(ply, out_dir, run)
            try:
                runpy.run_path(REFERENCE_SCRIPT, run_name="__main__")             # the reference script, as it is
            finally:
                sys.argv = argv
            (name,) = os.listdir(out_dir)
            vs, origin, xyz, rgb = parse_grid_ply(os.path.join(out_dir, name))
            out.update({f"{run}_name": np.array(name), f"{run}_voxel_size": np.float64(vs), f"{run}_origin": origin,
                        f"{run}_xyz": xyz, f"{run}_rgb": rgb})
            print(run, name, xyz.shape)
    np.savez_compressed(os.path.join(HERE, "voxel_grid_golden.npz"), **out)
    print("wrote voxel_grid_golden.npz", os.path.getsize(os.path.join(HERE, "voxel_grid_golden.npz")), "bytes")


if __name__ == "__main__":
    main()
