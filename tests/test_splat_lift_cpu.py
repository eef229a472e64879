"""The lift without a GPU: identities the float64 reference (tests/splat_lift_reference.py) must satisfy, the lifter's
division, and the host side of the two command lines."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import splat_lift_reference as lref  # noqa: E402
import splat_reference as ref  # noqa: E402
import voxproj_host  # noqa: E402


def small_scene(n=120, seed=3):
    rng = np.random.default_rng(seed)
    means = np.stack([rng.uniform(-1.0, 1.0, n), rng.uniform(-0.8, 0.8, n), rng.uniform(1.0, 4.0, n)], 1)
    s = dict(means=means.astype(np.float32), quats=rng.normal(size=(n, 4)).astype(np.float32),
             scales=(0.08 * np.exp(rng.normal(0, 0.5, (n, 3)))).astype(np.float32),
             opacities=rng.uniform(0.3, 0.95, n).astype(np.float32))
    W, H = 29, 21
    vm = np.eye(4, dtype=np.float32)
    K = np.array([[0.9 * W, 0, W / 2], [0, 0.9 * W, H / 2], [0, 0, 1]], np.float32)
    return s, vm, K, W, H


def test_weight_sums_telescope_to_alpha():
    s, vm, K, W, H = small_scene()
    rng = np.random.default_rng(0)
    m = rng.uniform(0.0, 1.0, (H, W)) * (rng.uniform(size=(H, W)) > 0.2)
    feats = rng.normal(size=(H, W, 5)).astype(np.float16)
    r = lref.lift64(s["means"], s["quats"], s["scales"], s["opacities"], feats, vm, K, W, H, pixel_weight=m)
    o = ref.splat64(s["means"], s["quats"], s["scales"], s["opacities"], np.zeros((len(s["means"]), 1)), vm, K, W, H)
    assert o["alpha"].max() > 0.5 and (r["wsum"] > 0).sum() >= 30
    assert r["wsum"].sum() == pytest.approx((m * o["alpha"]).sum(), rel=1e-12)
    assert (r["M_wsum"] == r["wsum"]).all()                       # weights are never negative


def test_lift_is_the_adjoint_of_the_splat():
    s, vm, K, W, H = small_scene(seed=4)
    rng = np.random.default_rng(1)
    D = 7
    F = rng.normal(size=(H, W, D)).astype(np.float16)
    X = rng.normal(size=(len(s["means"]), D))
    r = lref.lift64(s["means"], s["quats"], s["scales"], s["opacities"], F, vm, K, W, H)
    o = ref.splat64(s["means"], s["quats"], s["scales"], s["opacities"], X, vm, K, W, H)
    lhs = (r["sum"] * X).sum()
    rhs = (F.astype(np.float64).transpose(2, 0, 1) * o["logits"]).sum()
    assert abs(lhs) > 1.0 and lhs == pytest.approx(rhs, rel=1e-11)


def test_masked_pixels_contribute_nothing_whatever_they_hold():
    s, vm, K, W, H = small_scene(seed=5)
    rng = np.random.default_rng(2)
    F = rng.normal(size=(H, W, 3)).astype(np.float16)
    m = np.ones((H, W))
    m[::3] = 0.0
    F2 = F.copy()
    F2[::3] = np.nan
    a = lref.lift64(s["means"], s["quats"], s["scales"], s["opacities"], F, vm, K, W, H, pixel_weight=m)
    b = lref.lift64(s["means"], s["quats"], s["scales"], s["opacities"], F2, vm, K, W, H, pixel_weight=m)
    assert np.isfinite(b["sum"]).all() and np.array_equal(a["sum"], b["sum"]) and np.array_equal(a["wsum"], b["wsum"])


def test_class_scene_reference_leaves_few_gaussians_invalid():
    """The end-to-end scene of test_gpu_splat_lift.py: the float64 lift recovers every valid Gaussian's class and leaves
    fewer than 20 % of the Gaussians below the weight threshold, none of them within 1 % of it."""
    sc = lref.class_scene()
    tot, wt = lref.class_reference(sc)
    avg, valid = lref.finish64(tot, wt, lref.CLASS_MIN_WEIGHT)
    share = 1.0 - valid.mean()
    assert share < 0.2, f"{share:.3f} of the Gaussians are invalid in the reference"
    assert valid.sum() >= 150
    assert (np.abs(wt - lref.CLASS_MIN_WEIGHT) > 0.01 * lref.CLASS_MIN_WEIGHT).all()
    got = (avg @ lref.class_vectors().astype(np.float64).T).argmax(1)
    assert (got[valid] == sc["cls"][valid]).all()


def test_lifter_finish_handles_zero_weight_rows():
    lf = voxproj_host.GaussianFeatureLifter(5, 3, "cpu")
    assert lf.sum.shape == (5, 3) and lf.wsum.shape == (5,) and not lf.sum.any() and not lf.wsum.any()
    lf.sum[:] = torch.tensor([[2.0, 4.0, -6.0], [0.0, 0.0, 0.0], [1e-4, 2e-4, 3e-4], [3.0, 3.0, 3.0], [7.0, 7.0, 7.0]])
    lf.wsum[:] = torch.tensor([2.0, 0.0, 1e-4, 0.5, 0.0])
    avg, weight, valid = lf.finish(min_weight=1e-3)
    assert avg.dtype == torch.float16 and weight.dtype == torch.float32 and valid.dtype == torch.bool
    assert valid.tolist() == [True, False, False, True, False]
    assert avg[0].tolist() == [1.0, 2.0, -3.0] and avg[3].tolist() == [6.0, 6.0, 6.0]
    assert not avg[~valid].any() and torch.isfinite(avg).all()
    assert torch.equal(weight, lf.wsum) and weight.data_ptr() != lf.wsum.data_ptr()
    avg0, _, valid0 = lf.finish(min_weight=0.0)                   # a threshold of 0 still never divides by 0
    assert valid0.tolist() == [True, False, True, True, False] and torch.isfinite(avg0).all()
    assert avg0[2].tolist() == pytest.approx([1.0, 2.0, 3.0], rel=1e-3)


def test_size_function_needs_no_gpu_and_refuses_bad_arguments():
    f = voxproj_host.splat_lift_workspace_bytes
    r256 = lambda v: (v + 255) // 256 * 256  # noqa: E731
    assert f(1000, 512) == r256(1000 * 64 * 4) + r256(1000 * 4)
    assert f(1000, 17) == f(1000, 512) and f(1000, 16) == r256(1000 * 16 * 4) + r256(1000 * 4) == f(1000, 1)
    assert f(0, 8) == f(1, 8) == 512
    assert f(2 ** 31 - 1, 4096) == r256((2 ** 31 - 1) * 64 * 4) + r256((2 ** 31 - 1) * 4)
    for cap, C in ((-1, 8), (2 ** 31, 8), (10, 0), (10, 4097), (10, -3)):
        assert f(cap, C) == 0


def test_lift_cli_parser_and_pt_schema(tmp_path):
    import lift_gaussian_features as lgf
    a = lgf.build_parser().parse_args(["--gaussians_ply", "p", "--cam_params", "c", "--features_dir", "f", "--out", "o"])
    assert (a.views, a.max_images, a.downsample_factor, a.principal_point, a.weights_dir, a.min_weight) == \
        (None, None, None, "center", None, 1e-3)
    with pytest.raises(SystemExit):
        lgf.build_parser().parse_args(["--gaussians_ply", "p", "--cam_params", "c", "--out", "o"])
    rng = np.random.default_rng(0)
    xyz = torch.from_numpy(rng.normal(size=(6, 3))).float()
    avg = torch.from_numpy(rng.normal(size=(6, 4))).to(torch.float16)
    w = torch.tensor([1.0, 0.0, 2.0, 0.5, 0.0, 3.0])
    for name in ("a.pt", "b.pt"):
        lgf.save_lifted(str(tmp_path / name), xyz, avg, w, ["v0", "v1"])
    d = torch.load(str(tmp_path / "a.pt"))
    assert set(d) == {"xyz", "avg_feats", "weight", "views"} and d["views"] == ["v0", "v1"]
    assert d["avg_feats"].dtype == torch.float16 and d["xyz"].dtype == torch.float32 and d["weight"].dtype == torch.float32
    e = torch.load(str(tmp_path / "b.pt"))
    assert all(d[k].numpy().tobytes() == e[k].numpy().tobytes() for k in ("xyz", "avg_feats", "weight"))
    x2, f2, w2 = lgf.load_lifted(str(tmp_path / "a.pt"))
    assert torch.equal(x2, xyz) and torch.equal(f2, avg) and torch.equal(w2, w)
    torch.save({"xyz": xyz}, str(tmp_path / "bad.pt"))
    with pytest.raises(KeyError, match="avg_feats"):
        lgf.load_lifted(str(tmp_path / "bad.pt"))
    # non-finite pixels are masked through the pixel weights and counted
    feats = torch.zeros((3, 4, 2), dtype=torch.float16)
    feats[1, 2, 0] = float("nan")
    feats[0, 0, 1] = float("inf")
    m, n = lgf.mask_nonfinite(feats, None)
    assert n == 2 and m.dtype == torch.float32 and m.sum() == 10 and m[1, 2] == 0 and m[0, 0] == 0
    m2, n2 = lgf.mask_nonfinite(feats, torch.full((3, 4), 0.5))
    assert n2 == 2 and m2[1, 2] == 0 and m2[2, 3] == 0.5
    assert lgf.mask_nonfinite(torch.zeros((3, 4, 2), dtype=torch.float16), None) == (None, 0)


def test_query_cli_gauss_feats(tmp_path, capsys, monkeypatch):
    import lift_gaussian_features as lgf
    import query_voxel_features as qvf
    text = np.eye(3, 4, dtype=np.float32)
    np.save(tmp_path / "t.npy", text)
    t = str(tmp_path / "t.npy")
    base = ["gaussians", "--text_emb", t, "--prompt", "a", "b", "c", "--out", str(tmp_path / "o.npz")]
    for extra in (["--vox", "x.pt"], ["--map", "m.npy"], ["--gauss", "g.npy"]):
        with pytest.raises(SystemExit):
            qvf.main(base + ["--gauss_feats", "l.pt"] + extra)
        assert "--gauss_feats cannot be combined" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        qvf.main(base)
    assert "--gauss_feats" in capsys.readouterr().err
    a = qvf.build_parser().parse_args(base + ["--vox", "x.pt", "--gauss", "g.npy", "--map", "m.npy"])
    assert (a.vox, a.gauss, a.map, a.gauss_feats) == ("x.pt", "g.npy", "m.npy", None)       # the voxel route is unchanged

    # the lifted route with a stubbed query: rows are queried directly; a row of zeros, and a row without weight, get -1 and
    # zero logits
    feats = torch.tensor([[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 2, 0], [0, 3, 0, 0], [0, 0, 5, 0]], dtype=torch.float16)
    xyz = torch.arange(15, dtype=torch.float32).reshape(5, 3)
    lgf.save_lifted(str(tmp_path / "l.pt"), xyz, feats, torch.tensor([1.0, 0.5, 1.0, 1.0, 0.0]), ["v"])
    seen = {}

    def fake_query(rows, txt, scale, device):
        seen["rows"] = rows.clone()
        lg = rows.float() @ txt.float().T
        return lg.argmax(1).to(torch.int32), lg, torch.ones(len(rows))

    monkeypatch.setattr(qvf, "query", fake_query)
    args = qvf.build_parser().parse_args(base + ["--gauss_feats", str(tmp_path / "l.pt")])
    qvf._cmd_gaussians_lifted(args, torch.from_numpy(text), torch.device("cpu"))
    assert torch.equal(seen["rows"], feats)
    d = np.load(tmp_path / "o.npz")
    assert set(d.files) == {"labels", "logits", "prompts"} and d["labels"].dtype == np.int16 and d["logits"].dtype == np.float32
    assert d["labels"].tolist() == [0, -1, 2, 1, -1] and not d["logits"][1].any() and not d["logits"][4].any()
    assert d["logits"][2].tolist() == [0, 0, 2]
    assert [str(x) for x in d["prompts"]] == ["a", "b", "c"]
    import render_semantics_logits as rsl
    assert rsl.pad_logits(d["logits"]).shape == (5, 32)            # what render_semantics_logits.py reads from it
    assert os.path.exists(tmp_path / "o_colored_gaussians.ply")
