"""CPU-side checks of the label sums (include/voxproj_cluster.h): the fifth signature table against its header, the entry
points' host-side refusals, the NumPy twin of tests/label_sums_reference.py, the seeding of feature_clusters.py and the
condition the GPU clustering tests rest on.  No device call is made here."""
import os
import re

import numpy as np
import pytest

import label_sums_reference as ref
from test_abi_cpu import _binding_error          # the comparison of a ctypes binding with a C prototype, written once

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE_SEEDS = (1, 2, 3, 4)                       # planted_scene(6000, 32, 10, 0.5, seed): the scenes the GPU tests cluster
FIT_SEED = 0                                     # ... with feature_clusters.fit(seed=FIT_SEED, n_init=4)


def _cluster_prototypes():
    """{name: (return type, [parameter type, ...])} of every vp_* prototype of include/voxproj_cluster.h."""
    txt = open(os.path.join(ROOT, "include", "voxproj_cluster.h")).read()
    txt = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))

    def ctype(decl, named):
        words = [w for w in decl.replace("*", " ").split() if w != "const"]
        return " ".join(words[:-1] if named else words) + (" *" if "*" in decl else "")

    return {name: (ctype(ret, False), [ctype(q, True) for q in params.split(",")])
            for ret, name, params in re.findall(r"([A-Za-z_][\w \t]*?[\s\*]+)(vp_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", txt)}


def test_cluster_header_matches_the_fifth_signature_table():
    import ctypes

    import voxproj_host
    voxproj_host.build()
    protos = _cluster_prototypes()
    assert sorted(protos) == sorted(voxproj_host.EXPORTS_CLUSTER) == ["vp_label_sums", "vp_label_sums_workspace_bytes", "vp_row_inv_norms"]
    assert len(voxproj_host.EXPORTS) == 64 and len(voxproj_host.EXPORTS_EXT) == 2 and len(voxproj_host.EXPORTS_MESH) == 3
    assert len(voxproj_host.EXPORTS_GRID) == 3 and voxproj_host.VP_ABI_VERSION == 4
    others = set(voxproj_host.EXPORTS) | set(voxproj_host.EXPORTS_EXT) | set(voxproj_host.EXPORTS_MESH) | set(voxproj_host.EXPORTS_GRID)
    assert not set(voxproj_host.EXPORTS_CLUSTER) & others
    L = voxproj_host.lib()
    for name, proto in protos.items():
        fn = getattr(L, name)
        assert _binding_error(proto, fn.restype, fn.argtypes) is None, (name, _binding_error(proto, fn.restype, fn.argtypes))
    proto, good = protos["vp_label_sums"], list(L.vp_label_sums.argtypes)
    assert len(good) == 15 and proto[1][8] == "int64_t" and proto[1][13] == "size_t"
    assert "argument 8 is int64_t" in _binding_error(proto, ctypes.c_int, good[:8] + [ctypes.c_int] + good[9:])
    assert "takes 15 arguments, bound with 14" in _binding_error(proto, ctypes.c_int, good[:-1])


def test_entry_points_refuse_on_the_host_before_the_device_is_touched():
    """Fake device addresses that are never dereferenced: every refusal is host arithmetic."""
    import voxproj_host
    L = voxproj_host.lib()
    P = 0x7000_0000_0000
    nbase = dict(rows=P, f16=1, n=100, C=32, stride=32, inv=P + 4096, st=P + 8192)

    def norms(**kw):
        a = dict(nbase, **kw)
        return L.vp_row_inv_norms(a["rows"], a["f16"], a["n"], a["C"], a["stride"], a["inv"], a["st"], None)

    for kw, msg in ((dict(rows=None), b"null pointer argument (rows)"), (dict(inv=None), b"inv or status"), (dict(st=None), b"inv or status"),
                    (dict(f16=2), b"rows_f16 = 2 is neither 0 nor 1"), (dict(C=0), b"C = 0 outside [1, 4096]"),
                    (dict(C=4097, stride=4097), b"C = 4097 outside [1, 4096]"), (dict(n=-1), b"n_rows = -1 outside [0, 2^31 - 1]"),
                    (dict(n=1 << 31), b"n_rows = 2147483648"), (dict(stride=31), b"stride 31 < C = 32")):
        assert norms(**kw) == -1, kw
        assert msg in L.vp_last_error(), (kw, L.vp_last_error())

    sbase = dict(rows=P, f16=1, n=100, C=32, stride=32, lab=P + 4096, sc=None, K=10, R=0, sums=P + 8192, cnt=P + 12288, st=P + 16384,
                 ws=P + 20480, wb=1 << 30)

    def sums(**kw):
        a = dict(sbase, **kw)
        return L.vp_label_sums(a["rows"], a["f16"], a["n"], a["C"], a["stride"], a["lab"], a["sc"], a["K"], a["R"], a["sums"], a["cnt"],
                               a["st"], a["ws"], a["wb"], None)

    for kw, code, msg in ((dict(rows=None), -1, b"null pointer argument (rows)"), (dict(lab=None), -1, b"null pointer"),
                          (dict(sums=None), -1, b"null pointer"), (dict(cnt=None), -1, b"null pointer"), (dict(st=None), -1, b"null pointer"),
                          (dict(f16=-1), -1, b"rows_f16 = -1"), (dict(K=0), -1, b"K = 0 outside [1, 65536]"),
                          (dict(K=65537), -1, b"K = 65537 outside [1, 65536]"), (dict(C=0), -1, b"C = 0 outside [1, 4096]"),
                          (dict(C=4097, stride=4097), -1, b"C = 4097 outside"), (dict(n=1 << 31), -1, b"n_rows = 2147483648"),
                          (dict(n=-5), -1, b"n_rows = -5"), (dict(stride=8), -1, b"stride 8 < C = 32"),
                          (dict(R=-1), -1, b"part_rows = -1 is negative"), (dict(ws=None), -2, b"workspace is NULL"),
                          (dict(ws=P + 20481), -2, b"256-byte aligned"), (dict(wb=1024), -2, b"workspace has 1024 bytes, need"),
                          (dict(wb=0), -2, b"workspace has 0 bytes")):
        assert sums(**kw) == code, kw
        assert msg in L.vp_last_error(), (kw, L.vp_last_error())
    # a part_rows below the default needs room for more partial rows: 100 rows as 100 parts of 32 floats, refused at 4 KiB
    assert sums(R=1, wb=4096) == -2 and b"workspace has 4096 bytes, need" in L.vp_last_error()
    for args in ((-1, 10, 32), (1 << 31, 10, 32), (100, 0, 32), (100, 65537, 32), (100, 10, 0), (100, 10, 4097)):
        assert L.vp_label_sums_workspace_bytes(*args) == 0, args


def test_host_wrappers_refuse_bad_arguments_before_any_device_call(monkeypatch):
    import torch

    import voxproj_host

    def no_call(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(voxproj_host, "_call", no_call)
    rows = torch.zeros(5, 8, dtype=torch.float16)
    lab = torch.zeros(5, dtype=torch.int32)
    with pytest.raises(ValueError, match="rows must be a CUDA tensor: there is no CPU path"):
        voxproj_host.row_inv_norms(rows)
    with pytest.raises(ValueError, match="rows must be a CUDA tensor: there is no CPU path"):
        voxproj_host.label_sums(rows, lab, 3)
    with pytest.raises(ValueError, match="rows must be torch.float16 or torch.float32"):
        voxproj_host.label_sums(rows.double(), lab, 3)
    monkeypatch.setattr(voxproj_host, "_require_tensors", lambda *specs: None)
    for args, kw, msg in (((torch.zeros(5), lab, 3), {}, r"rows must be \[N, C\]"), ((torch.zeros(5, 4097), lab, 3), {}, r"C = 4097 must be in \[1, 4096\]"),
                          ((rows, lab, 0), {}, r"K = 0 must be in \[1, 65536\]"), ((rows, lab, 65537), {}, "K = 65537 must be"),
                          ((rows, lab, 3), dict(part_rows=-2), "part_rows = -2 must be >= 0"),
                          ((rows, lab[:4], 3), {}, r"labels must be int32 \[5\]"),
                          ((rows, lab, 3), dict(row_scale=torch.zeros(4)), r"row_scale must be float32 \[5\]")):
        with pytest.raises(ValueError, match=msg):
            voxproj_host.label_sums(*args, **kw)
    import feature_clusters
    for kw, msg in ((dict(K=0), "K = 0 must be"), (dict(K=1025), "K = 1025 must be"), (dict(K=3, max_iter=0), "max_iter = 0 must be")):
        with pytest.raises(ValueError, match=msg):
            feature_clusters.fit(rows, **kw)


# ---- the twin ----
def test_twin_order_is_not_a_plain_float64_sum():
    """Built to show the order: 1 then 2^-24 twice.  In float32, row by row, both small addends are lost (1 + 2^-24 rounds to
    1, to even); in float64 their sum 2^-23 is one float32 ulp of 1 and survives.  Cut into parts of one row the twin's
    float64 combine keeps it, so the part size shows as well."""
    x = np.array([[1.0], [2.0 ** -24], [2.0 ** -24]], np.float32)
    lab = np.zeros(3, np.int64)
    serial, counts, status = ref.label_sums(x, lab, 1)
    parts, _, _ = ref.label_sums(x, lab, 1, part_rows=1)
    ref64, ab64, n64 = ref.sums64(x, lab, 1)
    assert serial[0, 0] == np.float32(1.0) and parts[0, 0] == np.float32(1.0 + 2.0 ** -23) == np.float32(ref64[0, 0])
    assert counts.tolist() == [3] and status.tolist() == [0, 0] and n64.tolist() == [3] and ab64[0, 0] == ref64[0, 0]
    # the scale is applied in float32 before the sum: one rounding per element
    s = np.array([3.0, 1.0, 1.0], np.float32)
    y = np.array([[1.0 / 3.0], [0.0], [0.0]], np.float32)
    got, _, _ = ref.label_sums(y, lab, 1, row_scale=s)
    assert got[0, 0] == np.float32(np.float32(1.0 / 3.0) * np.float32(3.0))
    # left-out rows, empty labels, fp16 input
    h = np.arange(12, dtype=np.float16).reshape(6, 2)
    got, counts, status = ref.label_sums(h, np.array([2, -1, 0, 5, 2, -7]), 4)
    assert got.tolist() == [[4, 5], [0, 0], [8, 10], [0, 0]] and counts.tolist() == [1, 0, 2, 0] and status.tolist() == [2, 1]
    assert ref.default_part_rows(1) == 256 and ref.default_part_rows(32768 * 256) == 256 and ref.default_part_rows(32768 * 256 + 1) == 257


def test_twin_norms_and_helpers():
    x = np.array([[3, 4], [0, 0], [np.inf, 1], [np.nan, 0], [6e-8, 0]], np.float16)
    inv, zero, bad = ref.inv_norms64(x)
    assert inv[0] == 0.2 and inv[1] == 0 and inv[2] == 0 and inv[3] == 0 and zero.tolist() == [0, 1, 0, 0, 0] and bad.tolist() == [0, 0, 1, 1, 0]
    assert inv[4] == 1.0 / float(np.float16(6e-8))                      # a subnormal row has a direction
    assert ref.same_partition([0, 0, 1, -1], [5, 5, 2, -1]) and not ref.same_partition([0, 0, 1], [0, 1, 1])
    assert not ref.same_partition([0, 1, -1], [0, 1, 1])
    from sklearn.metrics import adjusted_rand_score
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 5, 500), rng.integers(0, 4, 500)
    assert abs(ref.adjusted_rand(a, b) - adjusted_rand_score(a, b)) < 1e-12 and ref.adjusted_rand(a, a) == 1.0
    rows, truth, dirs = ref.planted_scene(6000, 32, 10, 0.5, 1)
    assert rows.dtype == np.float16 and rows.shape == (6000, 32) and len(np.unique(truth)) == 10
    norms = np.linalg.norm(rows.astype(np.float64), axis=1)
    assert 0.4 < norms.min() < 0.7 and norms.max() > 6 * norms.min()  # u in [0.5, 4]: the row norms vary by a factor of eight or so


# ---- the seeding ----
def test_seeding_is_deterministic_per_seed_and_makes_no_device_call(monkeypatch):
    import feature_clusters as fc
    import voxproj_host
    monkeypatch.setattr(voxproj_host, "_call", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a device call was made")))
    rows, _, _ = ref.planted_scene(6000, 32, 10, 0.5, 1)
    valid = np.arange(6000)
    a = list(fc.seed_centroids(rows, valid, 10, seed=3, n_init=2))
    b = list(fc.seed_centroids(rows, valid, 10, seed=3, n_init=2))
    c = list(fc.seed_centroids(rows, valid, 10, seed=4, n_init=2))
    assert len(a) == 2 and all(x.dtype == np.float32 and x.shape == (10, 32) for x in a)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not np.array_equal(a[0], c[0]) and not np.array_equal(a[0], a[1])
    assert np.allclose(np.linalg.norm(a[0].astype(np.float64), axis=1), 1.0, atol=1e-6)
    # the centres are rows of the table, and a torch tensor reads as the array does
    unit = rows.astype(np.float64) / np.linalg.norm(rows.astype(np.float64), axis=1, keepdims=True)
    assert all((np.abs(unit.astype(np.float32)[:, None, :] - x[None]).max(axis=2) == 0).any(axis=0).all() for x in a)
    import torch
    t = list(fc.seed_centroids(torch.from_numpy(rows), valid, 10, seed=3, n_init=2))
    assert all(np.array_equal(x, y) for x, y in zip(a, t))
    # a sample: only the listed valid rows are drawn
    some = np.arange(0, 6000, 3)
    s = next(fc.seed_centroids(rows, some, 10, seed=0, n_init=1, sample=500))
    assert (np.abs(unit.astype(np.float32)[some][:, None, :] - s[None]).max(axis=2) == 0).any(axis=0).all()
    assert fc.default_sample(6000, 10) == 6000 and fc.default_sample(10 ** 6, 10) == 8192 and fc.default_sample(10 ** 6, 256) == 16384
    with pytest.raises(ValueError, match="cannot seed K = 10"):
        next(fc.seed_centroids(rows, np.arange(5), 10))
    # the table on the host: an empty label and a zero sum keep their centroid
    c0 = a[0][:3]
    S = np.array([[3.0] + [0.0] * 31, [0.0] * 32, [1.0] * 32], np.float32)
    c1, kept = fc.next_centroids(S, np.array([2, 4, 0]), c0)
    assert kept.tolist() == [False, True, True] and c1[0].tolist() == [1.0] + [0.0] * 31
    assert np.array_equal(c1[1], c0[1]) and np.array_equal(c1[2], c0[2])
    assert fc.objective64(S, c0) == float((S.astype(np.float64) * c0.astype(np.float64)).sum())


@pytest.mark.parametrize("scene", SCENE_SEEDS)
def test_seeding_then_float64_kmeans_recovers_the_planted_partition(scene):
    """The condition the GPU tests rest on: the product's seeding followed by the float64 Lloyd loop, best of four restarts,
    reaches adjusted Rand index exactly 1.0 against the planted labels on every scene the GPU tests cluster."""
    import feature_clusters as fc
    rows, truth, _ = ref.planted_scene(6000, 32, 10, 0.5, scene)
    runs = [ref.kmeans64(rows, c0) for c0 in fc.seed_centroids(rows, np.arange(6000), 10, seed=FIT_SEED, n_init=4)]
    best = max(runs, key=lambda r: r["objective"])
    print(f"scene {scene}: objectives {[round(r['objective'], 3) for r in runs]}, iterations {[r['n_iter'] for r in runs]}")
    assert ref.adjusted_rand(best["labels"], truth) == 1.0 and ref.same_partition(best["labels"], truth)


def test_the_overlapping_scene_takes_many_iterations_from_its_first_rows():
    """The start the GPU chain test uses: planted_scene(.., sigma = 1.0, ..) from its first ten rows runs 15 iterations or more
    in float64, with an objective that never falls."""
    rows, _, _ = ref.planted_scene(6000, 32, 10, 1.0, 1)
    r = ref.kmeans64(rows, rows[:10].astype(np.float64))
    obj = [h[0] for h in r["history"]]
    assert r["n_iter"] >= 15 and all(b >= a for a, b in zip(obj, obj[1:])) and r["history"][-1][1] > 0
