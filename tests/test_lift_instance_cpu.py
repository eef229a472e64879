"""lift_instance_features.py without a GPU: the parser's refusals, draw_count as a statement, and the float64 twin of the
training loop (tests/instance_twin.py) reaching the end conditions alone, which is what entitles
tests/test_gpu_lift_instance.py to ask them of the command line.

The twin runs two configurations, both --dim 8 --lr 0.05 --seed 0, on the scene of tests/codebook_scene.py:
  A: --steps 60 --all_pixels --views_per_step 1        B: --steps 120 --samples 2048 --views_per_step 2
Measured in float64 (378 of the 600 Gaussians are ``seen``; the untrained start rows give cosines -0.002 / 0.002 and accuracy 0.333):

  config   loss before   loss after   cosine same class   cosine other class   accuracy   association loss    consistent
  A        971.4064      232.2605     0.7704              -0.2204              0.9894     1.1589 -> 0.2665    yes
  B        971.4064      259.0367     0.8957              -0.2657              0.9921     1.0209 -> 0.1925    yes

The last two columns are the hand-off: the twin's rows rounded to binary16, the four images re-rendered with splat64, and
codebook_scene.train64 with its own CODES, STEPS, LR and SEED.  Nothing asserts that the loss falls from step to step: in
configuration B it is higher after 200 steps than after 120 while the rows still separate better.  The command line's values
for the same quantities on the MI355X are in tests/test_gpu_lift_instance.py's docstring."""
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

import codebook_scene as cs  # noqa: E402
import instance_twin as tw  # noqa: E402
import lift_instance_features as lif  # noqa: E402

SEEN = 378


@pytest.fixture(scope="module")
def scene():
    return cs.make()


@pytest.fixture(scope="module")
def matrices(scene):
    return tw.matrices(scene)


def _base(tmp_path):
    return ["--gaussians_ply", "x.ply", "--cam_params", "c.json", "--masks_dir", str(tmp_path), "--out", str(tmp_path / "o.pt")]


def test_parser_refusals(tmp_path):
    base = _base(tmp_path)
    for extra in (["--dim", "0"], ["--dim", "65"], ["--steps", "-1"], ["--views_per_step", "0"], ["--samples", "0"],
                  ["--min_count", "-1"], ["--samples", "100", "--all_pixels"], ["--all_pixels", "--samples", "100"]):
        with pytest.raises(SystemExit) as e:
            lif.main(base + extra)
        assert e.value.code == 2, extra                                    # ap.error, not another exit
    for missing in ("--gaussians_ply", "--cam_params", "--masks_dir", "--out"):
        i = base.index(missing)
        with pytest.raises(SystemExit):
            lif.main(base[:i] + base[i + 2:])
    args = lif.build_parser().parse_args(base)
    assert (args.dim, args.steps, args.views_per_step, args.samples, args.all_pixels, args.min_count, args.ignore_id, args.seed) == \
        (16, 200, 1, 32768, False, 20, -1, 0)
    assert (args.weight_contrast, args.weight_norm, args.lr) == (1.0, 1.0, 0.01)
    # the extremes the refusals leave are accepted
    for extra in (["--dim", "1"], ["--dim", "64"], ["--steps", "0"], ["--min_count", "0"], ["--samples", "1"]):
        lif.build_parser().parse_args(base + extra)


def test_main_has_no_cpu_path(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        lif.main(_base(tmp_path))
    assert not os.path.exists(tmp_path / "o.pt")


def test_draw_count_is_the_bincount_of_one_randint_draw():
    for n, samples, seed in ((64 * 48, 2048, 0), (64 * 48, 32768, 1), (7, 1, 2), (5, 23, 3), (1, 4, 4)):
        got = lif.draw_count(n, samples, torch.Generator().manual_seed(seed))
        assert got.dtype == torch.int32 and tuple(got.shape) == (n,) and got.device.type == "cpu"
        assert int(got.sum()) == samples and int(got.min()) >= 0
        draw = torch.randint(0, n, (samples,), generator=torch.Generator().manual_seed(seed))
        assert torch.equal(got, torch.bincount(draw, minlength=n).to(torch.int32))
        assert torch.equal(got, lif.draw_count(n, samples, torch.Generator().manual_seed(seed)))
    # with replacement: more draws than pixels must hit one twice, and that pixel counts twice
    got = lif.draw_count(5, 23, torch.Generator().manual_seed(3))
    assert int(got.max()) >= 5 and int(got.sum()) == 23
    # one generator, consumed: the second draw is another one, and exactly the second randint of the same stream
    gen, twin = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    a, b = lif.draw_count(3072, 2048, gen), lif.draw_count(3072, 2048, gen)
    torch.randint(0, 3072, (2048,), generator=twin)
    assert not torch.equal(a, b)
    assert torch.equal(b, torch.bincount(torch.randint(0, 3072, (2048,), generator=twin), minlength=3072).to(torch.int32))
    assert int((a > 1).sum()) > 0                                          # 2048 of 3072 with replacement: some pixel twice


def test_render_is_linear_in_the_rows(scene, matrices):
    """A_v @ rows against splat64 of the rows: the same float64 weights summed in another order, so at most N roundings of the
    largest product apart."""
    P0, _ = tw.start_rows()
    assert P0.shape == (cs.N, tw.DIM) and np.array_equal(P0, P0.astype(np.float32))         # fp32 values
    for v in range(cs.VIEWS):
        assert matrices[v].shape == (cs.H * cs.W, cs.N)
        assert (matrices[v] >= 0).all() and matrices[v].sum(1).max() <= 1.0 + 1e-12          # blend weights: sum 1 - T
        assert np.abs(matrices[v].sum(1).reshape(cs.H, cs.W) - scene["alpha"][v]).max() <= cs.N * 2.0 ** -52
        err = np.abs(tw.image_of(matrices[v], P0) - tw.render64(scene, v, P0)).max()
        print(f"view {v}: A @ rows against splat64: {err:.2e}")
        assert err <= cs.N * 2.0 ** -52 * np.abs(P0).max()
    s = tw.seen(matrices)
    assert s.dtype == bool and s.shape == (cs.N,) and int(s.sum()) == SEEN
    # the helper itself: rows that are their class's direction separate perfectly, shuffled classes do not
    cl = scene["g"]["classes"]
    same, other, acc = tw.separation(np.eye(cs.CLASSES)[cl] + 0.01 * P0[:, :cs.CLASSES], cl, s)
    assert same > 0.99 and abs(other) < 0.05 and acc == 1.0
    same, other, acc = tw.separation(P0, cl, s)
    print(f"start rows: cosine same {same:.3f} other {other:.3f} accuracy {acc:.3f}")
    assert abs(same) < 0.05 and abs(other) < 0.05 and acc < 0.6


@pytest.mark.parametrize("name", sorted(tw.CONFIGS))
def test_float64_twin_reaches_the_end_conditions(scene, matrices, name):
    """The loop of lift_instance_features.py in float64, with the step counts the GPU test gives the command line (A: 60,
    B: 120), separates the classes and hands rows to the association that reach its end condition."""
    res = tw.train64(scene, matrices, **tw.CONFIGS[name])
    same, other, acc = tw.separation(res["rows"], scene["g"]["classes"], tw.seen(matrices))
    print(f"twin {name}: loss {res['loss_before']:.4f} -> {res['loss_after']:.4f}, {res['ids']} ids; cosine same {same:.4f} "
          f"other {other:.4f}, accuracy {acc:.4f}")
    assert res["ids"] == cs.VIEWS * cs.CLASSES
    assert np.isfinite(res["rows"]).all() and res["loss_after"] < res["loss_before"]
    assert same > other
    assert acc >= 0.95
    # into the association: binary16 rows, re-rendered, codebook_scene's own loop and parameters
    handed = tw.hand_off(scene, res["rows"])
    _, l0, l1, assigns = cs.train64(handed, codes=cs.CODES, steps=cs.STEPS, lr=cs.LR, seed=cs.SEED)
    table = cs.class_to_code(handed, assigns)
    print(f"twin {name}: association loss {l0:.4f} -> {l1:.4f}\n{table}")
    assert cs.consistent(table)
