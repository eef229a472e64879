"""Annotated triangle meshes in PLY files (ScanNet++'s mesh_aligned_0.05_semantic.ply): a reader and a writer for tests.  No
plyfile dependency, as in gaussian_ply.py: the header is parsed by hand, the vertex records are read as one NumPy structured
array and the faces, whose records are all ``3 i0 i1 i2`` plus fixed-size scalars in a triangle mesh, as another.

Binary little-endian files only.  ``vertex`` holds x y z as float or double, optionally an integer ``label``, and any other
scalar properties, which are skipped.  ``face`` holds one ``list uchar int|uint vertex_indices`` (or ``vertex_index``) and any
scalar properties, which are skipped; a face that is not a triangle is an error that names it.
"""
import numpy as np

from gaussian_ply import _TYPES

_INDEX_NAMES = ("vertex_indices", "vertex_index")


def _header(f, path):
    """{element: (count, [property tokens after 'property'])} in file order, after checking the format line."""
    if f.readline().strip() != b"ply":
        raise ValueError(f"{path}: not a PLY file")
    fmt, elements, cur = None, {}, None
    while True:
        line = f.readline()
        if not line:
            raise ValueError(f"{path}: no end_header")
        tok = line.decode("ascii", "replace").split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            cur = tok[1]
            elements[cur] = (int(tok[2]), [])
        elif tok[0] == "property":
            if cur is None:
                raise ValueError(f"{path}: a property before any element")
            elements[cur][1].append(tok[1:])
        elif tok[0] == "end_header":
            break
    if fmt != "binary_little_endian":
        raise ValueError(f"{path}: format {fmt}; only binary_little_endian meshes are read")
    return elements


def _scalar(path, tok):
    if tok[0] not in _TYPES:
        raise ValueError(f"{path}: unknown property type {tok[0]}")
    return tok[1], "<" + _TYPES[tok[0]]


def read_mesh_ply(path):
    """dict(verts f32 [V,3], faces i32 [F,3], labels int64 [V] or None when the vertices carry no ``label``)."""
    with open(path, "rb") as f:
        elements = _header(f, path)
        if list(elements)[:2] != ["vertex", "face"]:
            raise ValueError(f"{path}: needs the elements vertex and face, in that order (found {list(elements)})")
        nv, vprops = elements["vertex"]
        nf, fprops = elements["face"]
        for tok in vprops:
            if tok[0] == "list":
                raise ValueError(f"{path}: list properties are not supported in the vertex element")
        vdt = np.dtype([_scalar(path, tok) for tok in vprops])
        for need in "xyz":
            if need not in vdt.names or vdt[need].kind != "f":
                raise ValueError(f"{path}: no float or double '{need}' property")
        if "label" in vdt.names and vdt["label"].kind not in "iu":
            raise ValueError(f"{path}: the vertex property 'label' must be an integer")
        fields, lists = [], 0
        for tok in fprops:
            if tok[0] == "list":
                if len(tok) != 4 or tok[3] not in _INDEX_NAMES or tok[1] not in ("uchar", "uint8") or tok[2] not in ("int", "int32", "uint", "uint32"):
                    raise ValueError(f"{path}: the face list must be 'list uchar int|uint vertex_indices', not '{' '.join(tok)}'")
                fields += [("_n", "u1"), ("_i", "<" + _TYPES[tok[2]], (3,))]
                lists += 1
            else:
                fields.append(_scalar(path, tok))
        if lists != 1:
            raise ValueError(f"{path}: the face element needs exactly one vertex index list (found {lists})")
        v = np.fromfile(f, dtype=vdt, count=nv)
        if len(v) != nv:
            raise ValueError(f"{path}: {len(v)} of {nv} vertex records")
        # every record has the size of a triangle's as long as every face is one: the first that is not is named
        fc = np.fromfile(f, dtype=np.dtype(fields), count=nf)
        not_tri = np.flatnonzero(fc["_n"] != 3)
        if len(not_tri):
            raise ValueError(f"{path}: face {int(not_tri[0])} has {int(fc['_n'][not_tri[0]])} vertices; only triangles are read")
        if len(fc) != nf:
            raise ValueError(f"{path}: {len(fc)} of {nf} face records")
    idx = fc["_i"]
    if idx.dtype.kind == "u" and len(idx) and idx.max() > 2 ** 31 - 1:
        raise ValueError(f"{path}: a vertex index above 2^31 - 1")
    return dict(verts=np.stack([v[k] for k in "xyz"], axis=1).astype(np.float32), faces=np.ascontiguousarray(idx.astype(np.int32)),
                labels=v["label"].astype(np.int64) if "label" in vdt.names else None)


def write_mesh_ply(path, verts, faces, labels=None, *, double=False, label_type="int", index_type="int", vertex_extra=(),
                   face_extra=(), face_sizes=None):
    """A binary little-endian triangle mesh.  ``vertex_extra`` / ``face_extra``: (name, ply type, values) columns written
    after x y z (label) and after the index list; ``face_sizes``: the list lengths to write instead of 3 (tests: a face that
    is no triangle)."""
    verts, faces = np.asarray(verts), np.asarray(faces).reshape(-1, 3)
    ftype = "double" if double else "float"
    vcols = [(k, ftype, verts[:, i]) for i, k in enumerate("xyz")]
    if labels is not None:
        vcols.append(("label", label_type, np.asarray(labels)))
    vcols += list(vertex_extra)
    vrec = np.zeros(len(verts), dtype=[(k, "<" + _TYPES[t]) for k, t, _ in vcols])
    for k, _, val in vcols:
        vrec[k] = val
    fcols = list(face_extra)
    frec = np.zeros(len(faces), dtype=[("_n", "u1"), ("_i", "<" + _TYPES[index_type], (3,))] + [(k, "<" + _TYPES[t]) for k, t, _ in fcols])
    frec["_n"] = 3 if face_sizes is None else face_sizes
    frec["_i"] = faces
    for k, _, val in fcols:
        frec[k] = val
    with open(path, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\n")
        f.write(f"element vertex {len(verts)}\n".encode())
        f.write("".join(f"property {t} {k}\n" for k, t, _ in vcols).encode())
        f.write(f"element face {len(faces)}\nproperty list uchar {index_type} vertex_indices\n".encode())
        f.write("".join(f"property {t} {k}\n" for k, t, _ in fcols).encode() + b"end_header\n")
        f.write(vrec.tobytes() + frec.tobytes())
