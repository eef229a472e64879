"""refine_gaussian_logits.py without a GPU: the target loader (size check, ignore mapping, weights) and the .npz schema."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import refine_gaussian_logits as rgl  # noqa: E402


def write_view(d, name, lab, conf=None):
    np.save(os.path.join(d, name + "_labels.npy"), lab)
    if conf is not None:
        np.save(os.path.join(d, name + "_confidence.npy"), conf)


def test_target_loader_maps_every_ignored_value_to_minus_one(tmp_path):
    H, W, P = 5, 7, 4
    lab = np.arange(H * W, dtype=np.int16).reshape(H, W) % 6 - 1          # -1 .. 4: -1 and 4 are outside [0, 4)
    lab[0, 0] = 255
    lab[0, 1] = -7
    conf = np.linspace(0, 1, H * W, dtype=np.float32).reshape(H, W)
    write_view(str(tmp_path), "v0", lab, conf)
    t, w = rgl.load_target(str(tmp_path), "v0", W, H, P)
    assert t.dtype == np.int32 and t.shape == (H, W) and w.dtype == np.float32
    inside = (lab >= 0) & (lab < P)
    assert (t[inside] == lab[inside]).all() and (t[~inside] == -1).all() and (~inside).sum() >= 10
    assert np.array_equal(w, conf)
    t2, w2 = rgl.load_target(str(tmp_path), "v0", W, H, P, weight="none")
    assert w2 is None and np.array_equal(t2, t)


def test_target_loader_rejects_a_size_mismatch(tmp_path):
    write_view(str(tmp_path), "v0", np.zeros((5, 7), np.int16), np.zeros((5, 7), np.float32))
    with pytest.raises(ValueError, match=r"7x5.*8x5"):
        rgl.load_target(str(tmp_path), "v0", 8, 5, 3)
    write_view(str(tmp_path), "v1", np.zeros((5, 8), np.int16), np.zeros((5, 7), np.float32))
    with pytest.raises(ValueError, match=r"\(5, 7\).*8x5"):
        rgl.load_target(str(tmp_path), "v1", 8, 5, 3)
    rgl.load_target(str(tmp_path), "v1", 8, 5, 3, weight="none")


def test_npz_schema_round_trips(tmp_path):
    rng = np.random.default_rng(0)
    logits = rng.normal(size=(30, 5)).astype(np.float32)
    prompts = np.array([f"c{i}" for i in range(5)])
    colors = rng.integers(0, 255, (30, 3)).astype(np.uint8)
    path = str(tmp_path / "r.npz")
    rgl.save_refined(path, logits, prompts, colors)
    d = np.load(path)
    assert set(d.files) == {"labels", "logits", "prompts", "colors"}
    assert d["labels"].dtype == np.int16 and np.array_equal(d["labels"], logits.argmax(1))
    assert d["logits"].dtype == np.float32 and d["logits"].tobytes() == logits.tobytes()
    assert [str(x) for x in d["prompts"]] == list(prompts) and np.array_equal(d["colors"], colors)
    # what render_semantics_logits.py reads from it
    import render_semantics_logits as rsl
    assert rsl.pad_logits(d["logits"]).shape == (30, 32)
    rgl.save_refined(path, logits)
    assert set(np.load(path).files) == {"labels", "logits"}


def test_parser_defaults():
    a = rgl.build_parser().parse_args(["--gaussians_ply", "p", "--logit_path", "l", "--cam_params", "c", "--targets_dir", "d",
                                       "--out", "o"])
    assert (a.steps, a.views_per_step, a.lr, a.seed, a.weight) == (200, 4, 0.1, 0, "confidence")
