"""CPU checks of the 3D neighbourhood regulariser's float64 statement (tests/reg3d_reference.py) and of its plumbing: the
statement against the reference's own loss_cls_3d (tests/golden/reg3d_golden.npz), its gradient against central differences,
brute-force k-NN against scipy's cKDTree, the reversed table against a Python loop, the new flags of
refine_gaussian_logits.py and the new symbols of the built library.  The last two fail without the feature."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "3d-semantic-segmentation_amd")
for p in (HERE, ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import reg3d_reference as r3  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, "golden", "reg3d_golden.npz"))
CASES = [0, 1, 2, 3]
NEW_SYMBOLS = ["vp_knn_points", "vp_neighbor_kl_workspace_bytes", "vp_neighbor_kl", "vp_neighbor_kl_gradient"]


def golden(i):
    return {k[len(f"c{i}_"):]: GOLDEN[k] for k in GOLDEN.files if k.startswith(f"c{i}_")}


@pytest.mark.parametrize("i", CASES)
def test_statement_reproduces_the_reference(i):
    """The reference computes in fp32: its loss must sit within 1e-6 relative of the float64 statement (about 17 u: a mean of
    N k P fp32 terms with fp32 logarithms; the recorded differences are below 1.1e-7) and its gradient within 4e-6 of the
    largest element (the same arithmetic through autograd's softmax backward)."""
    g = golden(i)
    k = int(g["k"])
    nbr, _ = r3.knn_brute(g["points"], k - 1)
    assert np.array_equal(nbr, g["nbr"])
    st = r3.statement64(g["logits"], None, nbr, k, scale=2.0)
    rel = abs(float(g["loss"]) - st["loss"]) / abs(st["loss"])
    print(f"case {i}: loss {st['loss']:.10g}, reference {float(g['loss']):.8g}, relative difference {rel:.2e} (recorded {float(g['rel_diff']):.2e})")
    assert rel <= 1e-6 and abs(rel - float(g["rel_diff"])) <= 1e-12
    gerr = np.abs(g["grad"].astype(np.float64) - st["grad"]).max()
    assert gerr <= 4e-6 * np.abs(st["grad"]).max()
    assert abs(gerr - float(g["grad_diff"])) <= 1e-15
    # the statement and the same loss written with torch ops agree in float64
    z = torch.tensor(g["logits"].astype(np.float64), requires_grad=True)
    loss = r3.torch_composite(z, None, nbr, k, scale=2.0)
    loss.backward()
    assert abs(float(loss.detach()) - st["loss"]) <= 1e-13 * abs(st["loss"])
    assert np.abs(z.grad.numpy() - st["grad"]).max() <= 1e-12 * np.abs(st["grad"]).max()


def _small_case(seed, N=23, P=6, k=4, with_samples=True):
    g = np.random.default_rng(seed)
    pts = g.uniform(0, 1, (N, 3)).astype(np.float32)
    logits = (2.0 * g.normal(size=(N, P))).astype(np.float32)
    nbr, _ = r3.knn_brute(pts, k - 1)
    samples = None
    if with_samples:
        samples = g.integers(0, N, 17)
        samples[3] = samples[0]                                       # a repeat
        nbr = nbr[samples].copy()
        nbr[2, 1] = -1
    return pts, logits, samples, nbr, k


@pytest.mark.parametrize("with_samples", [False, True])
def test_statement_gradient_against_central_differences(with_samples):
    _, logits, samples, nbr, k = _small_case(5, with_samples=with_samples)
    st = r3.statement64(logits, samples, nbr, k, scale=2.0, grad_loss=0.75)
    z = logits.astype(np.float64)
    h = 1e-6
    num = np.zeros_like(z)
    for i in range(z.shape[0]):
        for c in range(z.shape[1]):
            zp, zm = z.copy(), z.copy()
            zp[i, c] += h
            zm[i, c] -= h
            fp = float(r3.torch_composite(torch.tensor(zp), samples, nbr, k, scale=2.0))
            fm = float(r3.torch_composite(torch.tensor(zm), samples, nbr, k, scale=2.0))
            num[i, c] = 0.75 * (fp - fm) / (2 * h)
    # central differences in float64 at h = 1e-6: truncation h^2 |f'''| ~ 1e-12, cancellation 2^-53 |f| / h ~ 1e-11
    assert np.abs(num - st["grad"]).max() <= 1e-9
    assert np.abs(st["grad"]).max() > 1e-4
    # the statement and the torch composite are the same function
    assert abs(float(r3.torch_composite(torch.tensor(z), samples, nbr, k)) - st["loss"]) <= 1e-14


def test_empty_sample_and_bounds_are_finite():
    _, logits, _, _, k = _small_case(6)
    st = r3.statement64(logits, np.zeros(0, np.int64), np.zeros((0, k - 1), np.int64), k)
    assert st["loss"] == 0.0 and not st["grad"].any()
    _, logits, samples, nbr, k = _small_case(7)
    b = r3.bounds(logits, samples, nbr, k)
    for key in ("row_lse", "sample_loss", "grad"):
        assert np.isfinite(b[key]).all() and (b[key] >= 0).all()
    assert (b["row_lse"] > 0).all() and b["sum"] > 0
    # the bounds are rounding-sized: far below the values they bound
    st = r3.statement64(logits, samples, nbr, k)
    assert b["loss"] <= 1e-4 * abs(st["loss"]) and b["grad"].max() <= 1e-4 * np.abs(st["grad"]).max()


@pytest.mark.parametrize("i", CASES)
def test_brute_force_knn_against_ckdtree(i):
    from scipy.spatial import cKDTree
    g = golden(i)
    k = int(g["k"])
    pts = g["points"].astype(np.float64)
    idx, d2 = r3.knn_brute(g["points"], k - 1)
    d, j = cKDTree(pts).query(pts, k=k)                                # the point itself comes first, at distance 0
    assert (j[:, 0] == np.arange(len(pts))).all()
    # the generator kept every kept / dropped margin above 2e-3, and the golden points are distinct: the sets are unambiguous
    assert np.array_equal(np.sort(idx, 1), np.sort(j[:, 1:], 1))
    assert np.allclose(np.sqrt(d2), d[:, 1:], rtol=1e-12, atol=0)
    assert (np.diff(d2, axis=1) >= 0).all()


def test_knn_ties_and_short_sets():
    pts = np.zeros((5, 3), np.float32)                                 # every point coincident: the lowest indices win
    idx, d2 = r3.knn_brute(pts, 3)
    assert idx.tolist() == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 1, 2]] and not d2.any()
    idx, d2 = r3.knn_brute(pts[:2], 3)
    assert idx.tolist() == [[1, -1, -1], [0, -1, -1]] and np.isinf(d2[:, 1:]).all()
    q = np.array([[1, 0, 0]], np.float32)
    idx, d2 = r3.knn_brute(pts, 2, queries=q)                          # a foreign query leaves nothing out
    assert idx.tolist() == [[0, 1]] and d2.tolist() == [[1.0, 1.0]]
    assert r3.knn_mean_dist2(pts[:1]).tolist() == [0.0]


def test_reversed_table_against_a_loop():
    import voxproj_host
    g = np.random.default_rng(3)
    N, S, km1 = 40, 57, 4
    nbr = g.integers(-1, N, (S, km1)).astype(np.int32)
    nbr[5] = 7                                                         # one row named four times by one sample
    nbr[:, 0][::3] = 11                                                # a hub
    start, entry = voxproj_host.reverse_table(torch.from_numpy(nbr), N)
    want_start, want_entry = r3.reverse_table_loop(nbr, N)
    assert start.dtype == torch.int32 and entry.dtype == torch.int32 and entry.numel() == S * km1
    assert np.array_equal(start.numpy(), want_start)
    assert np.array_equal(entry.numpy()[:want_start[-1]], want_entry)
    tail = entry.numpy()[want_start[-1]:]
    assert (nbr.reshape(-1)[tail] == -1).all() and (np.diff(tail) > 0).all()
    # an empty table
    start, entry = voxproj_host.reverse_table(torch.zeros((0, km1), dtype=torch.int32), N)
    assert not start.numpy().any() and entry.numel() == 0


def test_cli_flags_and_their_defaults():
    import refine_gaussian_logits
    a = refine_gaussian_logits.build_parser().parse_args(
        "--gaussians_ply a --logit_path b --cam_params c --targets_dir d --out e".split())
    assert (a.reg3d_weight, a.reg3d_k, a.reg3d_interval, a.reg3d_sample_size) == (0.0, 5, 2, 0)


def test_library_exports_the_new_symbols():
    import voxproj_host
    voxproj_host.build()
    lib = ctypes.CDLL(voxproj_host.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in voxproj_host.EXPORTS
    L = voxproj_host.lib()
    # host arithmetic and host-side refusals: no GPU is touched
    assert voxproj_host.neighbor_kl_workspace_bytes(1000) >= 4000 + 256 * 8
    assert voxproj_host.neighbor_kl_workspace_bytes(-1) == 0
    P_ = 0x7000_0000_0000
    org = (ctypes.c_double * 3)(0, 0, 0)
    assert L.vp_knn_points(P_, P_, P_, org, 1.0, 2, 2, 2, P_, None, 10, 16, P_, None, None) == -1 and b"k = 16" in L.vp_last_error()
    assert L.vp_knn_points(None, P_, P_, org, 1.0, 2, 2, 2, P_, None, 10, 3, P_, None, None) == -1
    assert L.vp_neighbor_kl(P_, 10, 300, 300, None, 10, P_, 5, P_, None, P_, 0, P_, 1 << 20, None) == -1 and b"P = 300" in L.vp_last_error()
    assert L.vp_neighbor_kl(P_, 10, 8, 8, None, 10, P_, 1, P_, None, P_, 0, P_, 1 << 20, None) == -1 and b"k = 1" in L.vp_last_error()
    assert L.vp_neighbor_kl(P_, 10, 8, 8, None, 9, P_, 5, P_, None, P_, 0, P_, 1 << 20, None) == -1 and b"must be N" in L.vp_last_error()
    assert L.vp_neighbor_kl(P_, 10, 8, 8, None, 10, P_, 5, P_, None, P_, 2, P_, 1 << 20, None) == -1 and b"lanes" in L.vp_last_error()
    assert L.vp_neighbor_kl(P_, 10, 8, 8, None, 10, P_, 5, P_, None, P_, 0, P_, 16, None) == -2
    assert L.vp_neighbor_kl_gradient(P_, 10, 8, 8, P_, 4, P_, 5, P_, P_, P_, None, None, 2.0, None, P_, 8, 0, None) == -1
    assert b"smp_start" in L.vp_last_error()
