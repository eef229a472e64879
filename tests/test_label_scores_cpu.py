"""The label-map scores without a GPU: the two formulations of the boundary band agree, the metric arithmetic of
label_metrics.py on hand-made matrices, the two aggregations, and evaluate_label_maps.py's host side (pairing, loaders,
radius, resize index map, report) with a numpy stand-in for the device call."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import evaluate_label_maps as elm  # noqa: E402
import label_metrics as lm  # noqa: E402
import label_scores_reference as lref  # noqa: E402

# (W, H, r) of every band case of test_gpu_label_scores.py
SCENES = [(1, 1, 1), (1, 9, 1), (1, 9, 3), (9, 1, 1), (9, 1, 3), (37, 23, 1), (37, 23, 2), (37, 23, 5), (100, 70, 40),
          (64, 48, 64), (257, 19, 7), (300, 150, 3), (130, 200, 70)]


@pytest.mark.parametrize("W,H,r", SCENES, ids=[f"{w}x{h}-r{r}" for w, h, r in SCENES])
def test_the_two_band_formulations_agree(W, H, r):
    m = lref.make_map(W, H, 5, seed=1000 * W + H + r, n_rects=6, n_dots=4)
    assert np.array_equal(lref.band_by_erosion(m, r), lref.band_by_window(m, r))


@pytest.mark.parametrize("W,H,r", [(700, 300, 70), (1400, 800, 256)], ids=["700x300-r70", "1400x800-r256"])
def test_the_two_band_formulations_agree_at_large_radii(W, H, r):
    """The GPU file's large-radius maps: both axes exceed 2r + 1, so the band is not all ones."""
    m = lref.sparse_map(W, H, r)
    b = lref.band_by_window(m, r)
    assert np.array_equal(lref.band_by_erosion(m, r), b) and 0.05 < 1 - b.mean() < 0.95
    # the frame, and the square round the centre pixel, are band; a pixel well inside the background is not
    assert b[:r].all() and b[:, :r].all() and b[H // 2 - r:H // 2 + r + 1, W // 2 - r:W // 2 + r + 1].all()
    assert b[H // 2, W // 2 - r - 1] == 0 and b[H // 2, W // 2 + r + 1] == 0


def test_the_two_band_formulations_agree_on_the_special_maps():
    uniform = np.full((17, 33), 4, np.int32)
    frame = np.ones((17, 33), np.uint8)
    frame[3:-3, 3:-3] = 0
    assert np.array_equal(lref.band_by_erosion(uniform, 3), frame) and np.array_equal(lref.band_by_window(uniform, 3), frame)
    y, x = np.mgrid[:23, :41]
    checker = ((x + y) & 1).astype(np.int32)
    assert lref.band_by_erosion(checker, 1).all() and lref.band_by_window(checker, 1).all()
    holes = np.zeros((48, 80), np.int32)
    holes[10:30, 15:40] = -1
    holes[20:44, 50:70] = 255
    for r in (1, 4):
        assert np.array_equal(lref.band_by_erosion(holes, r), lref.band_by_window(holes, r))
    # the boundary counts from either formulation, on maps with invalid labels on both sides
    target = lref.make_map(100, 70, 5, seed=31, n_rects=7, invalid=0.08)
    pred = lref.perturb(target, 5, seed=32, n_rects=5, n_bad=4, bad_values=(-1, 255, 5, 1 << 20))
    for r in (3, 12):
        a = lref.boundary_counts(pred, target, 5, r)
        b = lref.boundary_counts_from_bands(pred, target, 5, lref.band_by_window(pred, r), lref.band_by_window(target, r))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].sum() > 0


def test_counting_reference_by_hand():
    target = np.array([[0, 0, 1], [1, -1, 255], [2, 2, 2]])
    pred = np.array([[0, 1, 1], [0, 0, 1], [2, -1, 7]])
    conf, skipped = lref.confusion(pred, target, 3)
    assert conf.tolist() == [[1, 1, 0], [1, 1, 0], [0, 0, 1]] and skipped.tolist() == [2, 2]


# ------------------------------------------------------------------------------------------------ the metric arithmetic
def test_metrics_of_a_perfect_prediction():
    m = lm.metrics(np.diag([5, 7, 11]), [2, 3, 4], [2, 3, 4])
    assert m["iou"] == [1.0, 1.0, 1.0] and m["miou"] == 1.0 and m["fwiou"] == 1.0 and m["pixel_accuracy"] == 1.0
    assert m["biou"] == [1.0, 1.0, 1.0] and m["mbiou"] == 1.0 and m["row"] == [5, 7, 11]


def test_a_class_absent_from_both_maps_is_null_and_left_out_of_the_mean():
    conf = np.array([[6, 2, 0], [1, 3, 0], [0, 0, 0]])
    m = lm.metrics(conf, [1, 0, 0], [4, 2, 0])
    assert m["iou"][2] is None and m["biou"][2] is None
    assert m["iou"][0] == 6 / 9 and m["iou"][1] == 3 / 6
    assert m["miou"] == pytest.approx((6 / 9 + 3 / 6) / 2, abs=1e-15)
    assert m["biou"][:2] == [0.25, 0.0] and m["mbiou"] == 0.125
    json.dumps(m, allow_nan=False)                     # null, never NaN
    # a class the prediction invents (no ground truth) has a denominator and an IoU of 0: it is in the mean
    m = lm.metrics(np.array([[4, 1], [0, 0]]))
    assert m["iou"] == [0.8, 0.0] and m["miou"] == 0.4 and m["fwiou"] == 0.8 and "biou" not in m


def test_everything_skipped():
    m = lm.metrics(np.zeros((4, 4), np.int64), np.zeros(4, np.int64), np.zeros(4, np.int64))
    assert m["iou"] == [None] * 4 and m["biou"] == [None] * 4
    assert m["miou"] is None and m["fwiou"] is None and m["pixel_accuracy"] is None and m["mbiou"] is None
    assert "NaN" not in json.dumps(m, allow_nan=False)


def test_fwiou_by_hand():
    conf = np.array([[50, 10, 0], [5, 20, 5], [0, 0, 10]])
    # rows 60, 30, 10; columns 55, 30, 15; IoU 50/65, 20/40, 10/15
    m = lm.metrics(conf)
    assert m["iou"] == [50 / 65, 20 / 40, 10 / 15]
    assert m["fwiou"] == pytest.approx((60 * 50 / 65 + 30 * 0.5 + 10 * 10 / 15) / 100, abs=1e-15)
    assert m["miou"] == pytest.approx((50 / 65 + 0.5 + 10 / 15) / 3, abs=1e-15)
    assert m["pixel_accuracy"] == 0.8
    with pytest.raises(ValueError):
        lm.metrics(np.zeros((2, 3)))


def test_lerf_differs_from_dataset_on_two_views():
    # view A: a large view, class 0 almost right, class 1 absent from its ground truth; view B: a small view, class 1 half right
    A = (np.array([[900, 100], [0, 0]]), np.array([90, 0]), np.array([100, 10]))
    B = (np.array([[0, 0], [10, 10]]), np.array([0, 5]), np.array([4, 10]))
    lerf = lm.lerf_aggregate([A, B])
    # class 0 is present in A only: 900/1000; class 1 in B only: 10/20 (its prediction as class 1 in A is not a view of class 1)
    assert lerf["iou"] == [0.9, 0.5] and lerf["miou"] == 0.7 and lerf["views_per_class"] == [1, 1]
    assert lerf["biou"] == [0.9, 0.5] and lerf["mbiou"] == 0.7
    ds = lm.metrics(A[0] + B[0], A[1] + B[1], A[2] + B[2])
    assert ds["iou"] == [900 / 1010, 10 / 120] and ds["miou"] != lerf["miou"]
    assert ds["biou"] == [90 / 104, 5 / 20]
    # a class present in two views: the mean of the two views' IoUs, not the IoU of the summed counts
    C = (np.array([[1, 3], [0, 0]]), None, None)
    two = lm.lerf_aggregate([(A[0], None, None), C])
    assert two["iou"][0] == (0.9 + 0.25) / 2 and two["iou"][1] is None and two["biou"] == [None, None] and two["mbiou"] is None
    assert lm.lerf_aggregate([])["miou"] is None


def test_boundary_radius_is_the_reference_formula():
    assert lm.boundary_radius(1600, 1067) == 38 and lm.boundary_radius(800, 533) == 19
    assert lm.boundary_radius(10, 10) == 1 and lm.boundary_radius(3, 2) == 1          # never below 1
    assert lm.boundary_radius(77, 53) == int(round(0.02 * np.sqrt(77 ** 2 + 53 ** 2)))
    assert lm.boundary_radius(1600, 1067, 0.01) == 19


# ------------------------------------------------------------------------------------------------ the CLI's host side
def numpy_scorer(calls=None):
    """The stand-in for voxproj_host.label_scores: the reference's counts for one view."""
    def score(pred, gt, P, radius):
        if calls is not None:
            calls.append((pred.shape, radius))
        conf, skipped = lref.confusion(pred, gt, P)
        if radius > 0:
            inter, union = lref.boundary_counts(pred, gt, P, radius)
        else:
            inter, union = np.zeros(P, np.int64), np.zeros(P, np.int64)
        return conf, skipped, inter, union
    return score


def test_stems_and_pairing(tmp_path):
    assert elm.stem_of("frame_00012_labels.npy") == "frame_00012" and elm.stem_of("00003_labels.pt") == "00003"
    assert elm.stem_of("frame_00012.png") == "frame_00012" and elm.stem_of("a_labels.PNG") == "a"
    assert elm.stem_of("frame_00012_confidence.npy") is None and elm.stem_of("notes.txt") is None
    assert elm.stem_of("_labels.npy") is None
    gt, pred = tmp_path / "gt", tmp_path / "pred"
    (pred / "labels").mkdir(parents=True)
    gt.mkdir()
    for name in ("b", "a"):
        np.save(gt / f"{name}_labels.npy", np.zeros((2, 3), np.int16))
        np.save(gt / f"{name}_confidence.npy", np.zeros((2, 3), np.float32))
    np.save(pred / "a_labels.npy", np.zeros((2, 3), np.int16))
    with pytest.raises(FileNotFoundError, match=r"b_labels\.npy.*no prediction for 'b'"):
        elm.pair_files(str(pred), str(gt))
    np.save(pred / "labels" / "b_labels.npy", np.zeros((2, 3), np.int16))
    pairs = elm.pair_files(str(pred), str(gt))
    assert [p[0] for p in pairs] == ["a", "b"] and pairs[1][2].endswith(os.path.join("labels", "b_labels.npy"))
    assert [p[0] for p in elm.pair_files(str(pred), str(gt), ["b"])] == ["b"]
    with pytest.raises(KeyError, match="zzz"):
        elm.pair_files(str(pred), str(gt), ["zzz"])
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="no label maps"):
        elm.pair_files(str(pred), str(tmp_path / "empty"))
    np.save(pred / "labels" / "a_labels.npy", np.zeros((2, 3), np.int16))
    with pytest.raises(ValueError, match="two label maps for 'a'"):
        elm.pair_files(str(pred), str(gt))


def test_loaders(tmp_path):
    import torch
    lab = (np.arange(35).reshape(5, 7) % 6 - 1).astype(np.int16)
    np.save(tmp_path / "v_labels.npy", lab)
    a = elm.load_label_map(str(tmp_path / "v_labels.npy"))
    assert a.dtype == np.int32 and np.array_equal(a, lab)
    torch.save({"label_indices": torch.from_numpy(lab.astype(np.uint8))}, tmp_path / "00000_labels.pt")
    b = elm.load_label_map(str(tmp_path / "00000_labels.pt"))
    # the renderer's uint8 container holds its "no label" (-1) as 255: read back as -1, so it is ignored even for P = 256
    assert b.dtype == np.int32 and np.array_equal(b, lab) and (b == -1).sum() == (lab == -1).sum() > 0
    torch.save({"other": 1}, tmp_path / "bad_labels.pt")
    with pytest.raises(ValueError, match="label_indices"):
        elm.load_label_map(str(tmp_path / "bad_labels.pt"))
    np.save(tmp_path / "f_labels.npy", np.zeros((5, 7), np.float32))
    with pytest.raises(ValueError, match="integer"):
        elm.load_label_map(str(tmp_path / "f_labels.npy"))
    np.save(tmp_path / "big_labels.npy", np.array([[1 << 40, 2]], np.int64))
    assert elm.load_label_map(str(tmp_path / "big_labels.npy")).tolist() == [[-1, 2]]


def test_png_loader_or_its_refusal(tmp_path, monkeypatch):
    lab = (np.arange(35).reshape(5, 7) % 5).astype(np.uint8)
    lab[0, 0] = 255
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        Image.fromarray(lab, mode="L").save(tmp_path / "g.png")
        pal = Image.fromarray(lab, mode="P")
        pal.putpalette([(i * 37) % 256 for i in range(768)])
        pal.save(tmp_path / "p.png")
        want = lab.astype(np.int32)
        want[0, 0] = -1
        assert np.array_equal(elm.load_label_map(str(tmp_path / "g.png")), want)
        assert np.array_equal(elm.load_label_map(str(tmp_path / "p.png")), want)
        Image.fromarray(np.zeros((5, 7, 3), np.uint8)).save(tmp_path / "rgb.png")
        with pytest.raises(ValueError, match="mode RGB"):
            elm.load_label_map(str(tmp_path / "rgb.png"))
    # without PIL a .png is refused by name
    (tmp_path / "x.png").write_bytes(b"")
    monkeypatch.setitem(sys.modules, "PIL", None)
    with pytest.raises(RuntimeError, match=r"x\.png.*PIL"):
        elm.load_label_map(str(tmp_path / "x.png"))


def test_resize_index_map():
    for dst, src in ((7, 3), (3, 7), (10, 10), (1600, 800), (5, 1), (1, 5), (1067, 533), (13, 29)):
        idx = elm.resize_index(dst, src)
        want = np.floor((np.arange(dst) + 0.5) * src / dst).astype(np.int64)
        assert np.array_equal(idx, want) and idx.min() >= 0 and idx.max() < src
    assert elm.resize_index(4, 2).tolist() == [0, 0, 1, 1] and elm.resize_index(2, 4).tolist() == [1, 3]
    assert elm.resize_index(3, 5).tolist() == [0, 2, 4]
    a = np.arange(12).reshape(3, 4)
    assert np.array_equal(elm.resize_nearest(a, 8, 6), lref.nearest_resize(a, 8, 6))
    assert elm.resize_nearest(a, 2, 2).tolist() == [[1, 3], [9, 11]]
    try:
        from PIL import Image
    except ImportError:
        return
    src = (np.arange(29 * 13).reshape(13, 29) % 251).astype(np.uint8)
    pil = np.array(Image.fromarray(src).resize((40, 31), resample=Image.NEAREST))
    assert np.array_equal(elm.resize_nearest(src, 40, 31), pil)


def write_views(tmp_path, P=4):
    gt, pred = tmp_path / "gt", tmp_path / "pred"
    gt.mkdir()
    pred.mkdir()
    maps = {}
    for k, (W, H) in enumerate(((40, 30), (25, 35))):
        t = lref.make_map(W, H, P, seed=10 + k, n_rects=5, invalid=0.1)
        p = lref.perturb(t, P, seed=20 + k, n_rects=3)
        np.save(gt / f"v{k}_labels.npy", t.astype(np.int16))
        np.save(pred / f"v{k}_labels.npy", np.clip(p, -1, 255).astype(np.int16))
        maps[f"v{k}"] = (np.clip(p, -1, 255), t)
    return gt, pred, maps


def test_cli_report(tmp_path):
    P = 4
    gt, pred, maps = write_views(tmp_path, P)
    np.savez(tmp_path / "q.npz", prompts=np.array(["wall", "floor", "chair", "plant"]))
    calls = []
    args = ["--pred", str(pred), "--gt", str(gt), "--num_classes", str(P), "--prompts_npz", str(tmp_path / "q.npz")]
    rep = elm.main(args + ["--out", str(tmp_path / "a.json")], score=numpy_scorer(calls))
    assert calls == [((30, 40), 1), ((35, 25), 1)]                       # max(1, round(0.02 * 50)) and round(0.02 * 43.01)
    conf = sum(lref.confusion(*maps[k], P)[0] for k in maps)
    skipped = sum(lref.confusion(*maps[k], P)[1] for k in maps)
    assert rep["confusion"] == conf.tolist() and rep["views"] == 2
    assert rep["skipped"] == dict(target_not_valid=int(skipped[0]), prediction_not_valid=int(skipped[1]))
    want = lm.metrics(conf)
    assert rep["dataset"]["miou"] == want["miou"] and rep["dataset"]["fwiou"] == want["fwiou"]
    assert rep["dataset"]["pixel_accuracy"] == want["pixel_accuracy"] and rep["dataset"]["mbiou"] is not None
    assert [c["name"] for c in rep["classes"]] == ["wall", "floor", "chair", "plant"]
    assert [c["iou"] for c in rep["classes"]] == want["iou"] and [c["pixels"] for c in rep["classes"]] == want["row"]
    per = [lm.metrics(lref.confusion(*maps[k], P)[0]) for k in sorted(maps)]
    assert [v["name"] for v in rep["per_view"]] == ["v0", "v1"] and [v["miou"] for v in rep["per_view"]] == [m["miou"] for m in per]
    lerf = lm.lerf_aggregate([(lref.confusion(*maps[k], P)[0], None, None) for k in sorted(maps)])
    assert rep["lerf"]["miou"] == lerf["miou"] and rep["lerf"]["mbiou"] is not None
    # two runs: the same bytes; and the file is the returned report
    elm.main(args + ["--out", str(tmp_path / "b.json")], score=numpy_scorer())
    assert (tmp_path / "a.json").read_bytes() == (tmp_path / "b.json").read_bytes()
    assert json.loads((tmp_path / "a.json").read_text()) == json.loads(json.dumps(rep))
    # --no_boundary: radius 0, no boundary figures; --boundary_ratio scales the radius
    calls.clear()
    rep0 = elm.main(args + ["--no_boundary", "--out", str(tmp_path / "c.json")], score=numpy_scorer(calls))
    assert [c[1] for c in calls] == [0, 0] and rep0["dataset"]["mbiou"] is None and rep0["bnd_union"] is None
    assert rep0["confusion"] == rep["confusion"] and rep0["lerf"]["mbiou"] is None
    calls.clear()
    elm.main(args + ["--boundary_ratio", "0.1", "--views", "v1", "--out", str(tmp_path / "d.json")], score=numpy_scorer(calls))
    assert calls == [((35, 25), 4)]


def test_cli_size_mismatch_and_resize(tmp_path):
    P = 4
    gt, pred, maps = write_views(tmp_path, P)
    small = lref.make_map(20, 15, P, seed=3).astype(np.int16)
    np.save(pred / "v0_labels.npy", small)
    args = ["--pred", str(pred), "--gt", str(gt), "--num_classes", str(P), "--out", str(tmp_path / "r.json")]
    with pytest.raises(ValueError, match=r"20x15.*40x30"):
        elm.main(args, score=numpy_scorer())
    rep = elm.main(args + ["--resize_pred"], score=numpy_scorer())
    assert [v["resized"] for v in rep["per_view"]] == [True, False]
    up = lref.nearest_resize(small, 40, 30)
    assert np.array_equal(up, np.repeat(np.repeat(small, 2, 0), 2, 1))
    conf = lref.confusion(up, maps["v0"][1], P)[0] + lref.confusion(*maps["v1"], P)[0]
    assert rep["confusion"] == conf.tolist()
    with pytest.raises(ValueError, match="outside"):
        elm.evaluate([], 300, score=numpy_scorer())


def test_parser_defaults_and_refine_flag():
    a = elm.build_parser().parse_args(["--pred", "p", "--gt", "g", "--num_classes", "13", "--out", "o"])
    assert (a.boundary_ratio, a.no_boundary, a.resize_pred, a.views, a.prompts_npz) == (0.02, False, False, None, "")
    import refine_gaussian_logits as rgl
    base = ["--gaussians_ply", "p", "--logit_path", "l", "--cam_params", "c", "--targets_dir", "d", "--out", "o"]
    assert rgl.build_parser().parse_args(base).report_miou is False
    assert rgl.build_parser().parse_args(base + ["--report_miou"]).report_miou is True
