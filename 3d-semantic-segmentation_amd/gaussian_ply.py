"""3D Gaussian Splatting point_cloud.ply files: a reader with the model's activations and a writer for tests and synthetic
scenes.  No plyfile dependency: the header is parsed by hand and the vertex records read as one NumPy structured array.

The reader follows the reference's GaussianModel.load_ply and its activations (scene/gaussian_model.py): x y z as they are,
opacity = sigmoid(opacity), scale = exp(scale_*), rotation = normalize(rot_*) (w, x, y, z), the scale_* and rot_* fields in
the order of their numeric suffix.  The f_dc_* / f_rest_* colour fields (and any others, normals included) are skipped,
unless ``want_dc`` asks for the three f_dc_* columns (the degree-0 colour, raw: colour = 0.5 + 0.28209479 f_dc) or
``want_sh`` for the f_rest_* columns, the spherical-harmonics coefficients of degree 1 .. 3.  The file stores those
channel-major, f_rest_i = channel i // Kr, coefficient i % Kr (scene/gaussian_model.py:385,427-428: the transpose of the
model's [N,Kr,3] parameter, flattened); reader and writer speak the parameter's layout, [N,Kr,3].
Binary little-endian files only, the format 3DGS writes.
"""
import numpy as np

_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
          "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
          "double": "f8", "float64": "f8"}


def _header(f, path):
    if f.readline().strip() != b"ply":
        raise ValueError(f"{path}: not a PLY file")
    fmt, n, props, in_vertex = None, None, [], False
    while True:
        line = f.readline()
        if not line:
            raise ValueError(f"{path}: no end_header")
        tok = line.decode("ascii", "replace").split()
        if not tok:
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            in_vertex = tok[1] == "vertex"
            if in_vertex:
                n = int(tok[2])
            elif n is None:
                raise ValueError(f"{path}: element '{tok[1]}' before the vertices is not supported")
        elif tok[0] == "property" and in_vertex:
            if tok[1] == "list":
                raise ValueError(f"{path}: list properties are not supported in the vertex element")
            if tok[1] not in _TYPES:
                raise ValueError(f"{path}: unknown property type {tok[1]}")
            props.append((tok[2], "<" + _TYPES[tok[1]]))
        elif tok[0] == "end_header":
            break
    if fmt != "binary_little_endian":
        raise ValueError(f"{path}: format {fmt}; 3DGS point clouds are binary_little_endian")
    if n is None:
        raise ValueError(f"{path}: no vertex element")
    return n, np.dtype(props)


def _sorted_fields(names, prefix):
    return sorted((p for p in names if p.startswith(prefix)), key=lambda p: int(p.rsplit("_", 1)[-1]))


SH_MAX_DEGREE = 3


def sh_degree_of_width(kr):
    """The degree D <= 3 with (D + 1)^2 - 1 == kr coefficient rows, or None."""
    return {(D + 1) ** 2 - 1: D for D in range(SH_MAX_DEGREE + 1)}.get(int(kr))


def read_vertex_records(path):
    """The vertex records of a binary little-endian point cloud as one NumPy structured array: every column as stored, no
    field required, no activation (what plyfile's PlyData.read(path)['vertex'].data holds)."""
    with open(path, "rb") as f:
        n, dt = _header(f, path)
        v = np.fromfile(f, dtype=dt, count=n)
    if len(v) != n:
        raise ValueError(f"{path}: {len(v)} of {n} vertex records")
    return v


def read_gaussian_ply(path, want_dc=False, want_raw=False, want_sh=False):
    """dict(means f32 [N,3], quats f32 [N,4] (w,x,y,z, unit norm; a zero quaternion stays zero), scales f32 [N,3],
    opacities f32 [N]) with the model's activations applied.  ``want_dc`` adds f_dc f32 [N,3], the f_dc_0..2 columns as
    stored; ``want_raw`` adds opacity_logits f32 [N], log_scales f32 [N,3] and rots f32 [N,4], the columns as stored (what
    write_gaussian_ply takes, so that a field nobody changed is written back bit for bit); ``want_sh`` adds f_rest f32
    [N,Kr,3] from the f_rest_* columns (Kr = 0, a zero-width array, when the file has none; a column count that is not
    3 ((D + 1)^2 - 1) for a degree D <= 3 is an error)."""
    with open(path, "rb") as f:
        n, dt = _header(f, path)
        v = np.fromfile(f, dtype=dt, count=n)
    if len(v) != n:
        raise ValueError(f"{path}: {len(v)} of {n} vertex records")
    names = dt.names
    for need in ("x", "y", "z", "opacity"):
        if need not in names:
            raise ValueError(f"{path}: no '{need}' property")
    scale_f, rot_f = _sorted_fields(names, "scale_"), _sorted_fields(names, "rot_")
    if len(scale_f) != 3 or len(rot_f) != 4:
        raise ValueError(f"{path}: needs scale_0..2 and rot_0..3 (found {scale_f}, {rot_f})")
    col = lambda names_: np.stack([v[k].astype(np.float64) for k in names_], axis=1)  # noqa: E731
    means = col(("x", "y", "z"))
    rot = col(rot_f)
    norm = np.linalg.norm(rot, axis=1, keepdims=True)
    quats = rot / np.maximum(norm, 1e-12)                       # torch.nn.functional.normalize
    scales = np.exp(col(scale_f))
    op = 1.0 / (1.0 + np.exp(-v["opacity"].astype(np.float64)))
    out = dict(means=means.astype(np.float32), quats=quats.astype(np.float32), scales=scales.astype(np.float32),
               opacities=op.astype(np.float32))
    if want_dc:
        dc_f = _sorted_fields(names, "f_dc_")
        if len(dc_f) != 3:
            raise ValueError(f"{path}: needs f_dc_0..2 (found {dc_f})")
        out["f_dc"] = col(dc_f).astype(np.float32)
    if want_sh:
        rest_f = _sorted_fields(names, "f_rest_")
        kr = len(rest_f) // 3
        if len(rest_f) % 3 or sh_degree_of_width(kr) is None or [int(k.rsplit("_", 1)[-1]) for k in rest_f] != list(range(3 * kr)):
            raise ValueError(f"{path}: {len(rest_f)} f_rest_* columns are not f_rest_0..{{3 ((D + 1)^2 - 1) - 1}} for a degree D <= {SH_MAX_DEGREE}")
        rest = np.stack([v[k] for k in rest_f], axis=1).astype(np.float32) if kr else np.zeros((n, 0), np.float32)
        out["f_rest"] = np.ascontiguousarray(rest.reshape(n, 3, kr).transpose(0, 2, 1))
    if want_raw:
        out.update(opacity_logits=v["opacity"].astype(np.float32), log_scales=col(scale_f).astype(np.float32),
                   rots=rot.astype(np.float32))
    return out


def write_gaussian_ply(path, means, opacity_logits, log_scales, rots, f_dc=None, f_rest=None):
    """A binary little-endian 3DGS point cloud: x y z nx ny nz f_dc_0..2 opacity scale_0..2 rot_0..3 (raw, pre-activation
    values, as 3DGS saves them).  With ``f_rest`` [N,Kr,3] the f_rest_0..3Kr-1 columns stand between f_dc_* and opacity,
    channel-major as the reference writes them; without it the file is the 17-field one."""
    n = len(means)
    rest = None
    if f_rest is not None:
        rest = np.asarray(f_rest, np.float32)
        if rest.ndim != 3 or rest.shape[0] != n or rest.shape[2] != 3 or sh_degree_of_width(rest.shape[1]) is None:
            raise ValueError(f"f_rest must be [{n}, (D + 1)^2 - 1, 3] for a degree D <= {SH_MAX_DEGREE}, not {rest.shape}")
        rest = rest.transpose(0, 2, 1).reshape(n, -1)
    fields = (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] +
              [f"f_rest_{i}" for i in range(rest.shape[1] if rest is not None else 0)] +
              ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"])
    rec = np.zeros(n, dtype=[(k, "<f4") for k in fields])
    if rest is not None:
        for i in range(rest.shape[1]):
            rec[f"f_rest_{i}"] = rest[:, i]
    for i, k in enumerate("xyz"):
        rec[k] = np.asarray(means)[:, i]
    if f_dc is not None:
        for i in range(3):
            rec[f"f_dc_{i}"] = np.asarray(f_dc)[:, i]
    rec["opacity"] = opacity_logits
    for i in range(3):
        rec[f"scale_{i}"] = np.asarray(log_scales)[:, i]
    for i in range(4):
        rec[f"rot_{i}"] = np.asarray(rots)[:, i]
    with open(path, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\n")
        f.write(f"element vertex {n}\n".encode())
        for k in fields:
            f.write(f"property float {k}\n".encode())
        f.write(b"end_header\n")
        f.write(rec.tobytes())
