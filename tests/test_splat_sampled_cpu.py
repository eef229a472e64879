"""The sampled-pixel float64 reference (splat_reference.splat64_at, splat_grad_reference.splat_grad64_at), the
conditioning-aware bound and the fp32 twin, checked without a GPU.

  * splat64_at / splat_grad64_at over all pixels of small scenes equal the dense splat64 / splat_geom64: masks, labels and
    visit counts identical; values to float64 summation noise, (n + 2) eps64 sum_g w_g |f_g| for a sum of n terms taken in
    two different orders (each order is within (n - 1) eps64 / 2 of the exact sum to first order; the 2 covers the products).
  * every scene of test_gpu_splat_scale.py and test_gpu_splat_cameras.py, built here at full size: the fragile share is
    under the scene's cap, enough non-fragile pixels are reached, and the fp32 twin (NumPy float32 in the kernel's operation
    order) is inside the derived bound at every non-fragile pixel.  The bound is thereby checked against the reference alone.
  * the needle measurement: fp32 sigma is off by more than 1e-3 where the old claim allowed 1e-5, and inside SIGMA_GAMMA u m.
  * the GPU tests can fail: a reversed tie order, a support box one tile short, an ignored far plane and a flipped B each
    move the sampled values by far more than the bound.
"""
import time

import numpy as np
import pytest

import splat_geom_reference as geo
import splat_grad_reference as gref
import splat_reference as ref
import splat_scenes as sc
from test_gpu_splat import camera, scene

EPS = np.finfo(np.float64).eps


def args(s, vm, K, W, H):
    return s["means"], s["quats"], s["scales"], s["opacities"], s["features"], vm, K, W, H


def small(name):
    """The generators of test_gpu_splat.py: a random scene, its crowded tile, its near plane, its zero scales."""
    if name == "crowded":
        W, H, n = 32, 32, 3000
        rng = np.random.default_rng(11)
        s = scene(n, 32, 11)
        s["means"] = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), rng.uniform(1.5, 3.0, n)], 1).astype(np.float32)
        s["scales"] = np.full((n, 3), 0.3, np.float32)
        s["opacities"] = rng.uniform(0.01, 0.03, n).astype(np.float32)
        return s, np.eye(4, dtype=np.float32), np.array([[30, 0, 16], [0, 30, 16], [0, 0, 1]], np.float32), W, H
    W, H = 61, 47
    if name == "near_plane":
        return (scene(600, 8, 5, z=(-0.5, 3.0), spread=3.0),) + camera(W, H, t=(0, 0, 0)) + (W, H)
    if name == "zero_scale":
        s = scene(500, 5, 9)
        s["scales"][::2] = 0.0
        s["opacities"][:] = np.maximum(s["opacities"], 0.5)
        return (s,) + camera(W, H) + (W, H)
    return (scene(400, 13, 0),) + camera(W, H) + (W, H)


@pytest.mark.parametrize("name", ["random", "crowded", "near_plane", "zero_scale"])
def test_sampled_forward_equals_dense(name):
    s, vm, K, W, H = small(name)
    D = s["features"].shape[1]
    tol = 2 * ref.value_bound(s["features"])
    o = ref.splat64(*args(s, vm, K, W, H), value_tol=tol)
    a = ref.splat64_at(*args(s, vm, K, W, H), sc.all_pixels(W, H), value_tol=tol, cond=False)
    img = lambda v: v.reshape(H, W)  # noqa: E731
    assert np.array_equal(img(a["fragile"]), o["fragile"])
    assert np.array_equal(img(a["label"]), o["label"])
    assert np.array_equal(img(a["visits"]), o["visits"]) and o["visits"].max() > (512 if name == "crowded" else 5)
    assert np.array_equal(img(a["alpha"]), o["alpha"])                  # the same products in the same order
    assert (a["extra"] == 0).all() and (a["extra_alpha"] == 0).all()
    err = np.abs(a["logits"].T.reshape(D, H, W) - o["logits"])
    assert (err <= (o["visits"] + 2) * EPS * a["scale"].T.reshape(D, H, W)).all()
    assert np.abs(img(a["confidence"]) - o["confidence"]).max() <= 1e-12
    # the conditioning-aware bands contain the flat ones, and on these benign scenes add next to nothing
    c = ref.splat64_at(*args(s, vm, K, W, H), sc.all_pixels(W, H), value_tol=tol)
    assert (c["fragile"] >= a["fragile"]).all() and c["fragile"].sum() <= a["fragile"].sum() + 0.01 * W * H
    assert np.array_equal(c["logits"], a["logits"]) and (c["extra"] >= 0).all()
    assert c["extra"].max() <= 0.5 * ref.value_bound(s["features"])


@pytest.mark.parametrize("name", ["random", "crowded", "near_plane"])
def test_sampled_backward_equals_dense(name):
    s, vm, K, W, H = small(name)
    D = s["features"].shape[1]
    rng = np.random.default_rng(3)
    pix = sc.all_pixels(W, H)[rng.choice(W * H, 150, replace=False)]
    Gp, Gap = rng.normal(size=(len(pix), D)), rng.normal(size=len(pix))
    G, Ga = np.zeros((D, H, W)), np.zeros((H, W))
    G[:, pix[:, 0], pix[:, 1]] = Gp.T
    Ga[pix[:, 0], pix[:, 1]] = Gap
    d = geo.splat_geom64(*args(s, vm, K, W, H), G=G, G_alpha=Ga)
    a = gref.splat_grad64_at(*args(s, vm, K, W, H), pix, Gp, Gap, cond=False)
    assert np.array_equal(a["fragile"], d["fragile"][pix[:, 0], pix[:, 1]])
    assert np.array_equal(a["visits"], d["visits"][pix[:, 0], pix[:, 1]])
    n = d["visits"].max() + len(pix) + 2                     # terms of the longest sum: a pixel's Gaussians, a Gaussian's pixels
    for k, m in (("grad_f", "M_f"), ("grad_o", "M_o"), ("grad_screen", "M_screen")):
        assert (np.abs(d[k]) > 0).sum() >= 50
        assert (np.abs(a[m] - d[m]) <= n * EPS * d[m]).all(), m
        assert (np.abs(a[k] - d[k]) <= n * EPS * d[m]).all(), k
        assert (a["X_" + k[5:]] == 0).all()
    # a dense G restricted to those pixels is the same loss: splat_grad64 agrees as well
    e = gref.splat_grad64(*args(s, vm, K, W, H), G=G, G_alpha=Ga)
    assert (np.abs(a["grad_f"] - e["grad_f"]) <= n * EPS * e["M_f"]).all()
    assert (np.abs(a["grad_o"] - e["grad_o"]) <= n * EPS * e["M_o"]).all()


# ---------------------------------------------------------------------------------------- the GPU tests' scenes, oracle and twin
def oracle_and_twin(S, flip_b=False):
    s, W, H = S["s"], S["W"], S["H"]
    pix = S["pixels"] if S["pixels"] is not None else sc.all_pixels(W, H)
    rec = ref.records(*args(s, S["vm"], S["K"], W, H)[:4], S["vm"], S["K"], W, H, **S["kw"])
    o = ref.splat64_at(*args(s, S["vm"], S["K"], W, H), pix, value_tol=2 * ref.value_bound(s["features"]), rec=rec, **S["kw"])
    return rec, pix, o, ref.splat32_at(rec, s["features"], pix, flip_b=flip_b)


def ratios(S, o, tw):
    """The twin's error over the bound, per output, on the non-fragile pixels."""
    good = ~o["fragile"]
    B = ref.value_bound_at(S["s"]["features"], o)
    return dict(logits=float((np.abs(tw["logits"] - o["logits"]) / B)[good].max()),
                alpha=float((np.abs(tw["alpha"] - o["alpha"]) / (1e-5 + o["extra_alpha"]))[good].max()),
                confidence=float((np.abs(tw["confidence"] - o["confidence"]) / (2 * B.max(1) + 1e-6))[good].max()),
                labels=int((tw["label"] != o["label"])[good].sum()))


SCENES = [("camera", n) for n in sc.CAMERAS] + [("ties", ""), ("ties", "reversed")] + [("hard", n) for n in sc.HARD] + \
    [("production", (200_000, 13, 0)), ("production", (200_000, 32, 1)), ("production", (1_000_000, 13, 1))]


def build(kind, what):
    if kind == "camera":
        return sc.camera_scene(what)
    if kind == "ties":
        return sc.ties_scene(reverse=what == "reversed")
    if kind == "hard":
        return sc.hard_scene(what)
    n, D, view = what
    return sc.production(n, D, view, **(dict(n_scatter=150, few=True) if n > 500_000 else {}))


@pytest.mark.parametrize("kind,what", SCENES, ids=lambda v: str(v).replace(" ", ""))
def test_scene_oracle_and_twin(kind, what):
    t0 = time.time()
    S = build(kind, what)
    rec, pix, o, tw = oracle_and_twin(S)
    good = ~o["fragile"]
    share = 1.0 - good.mean()
    reached = int((good & (o["visits"] > 0)).sum())
    r = ratios(S, o, tw)
    flat = float((np.abs(tw["logits"] - o["logits"]) / ref.value_bound(S["s"]["features"]))[good].max())
    print(f"sampled-cpu {kind} {what}: pixels {len(pix)} kept {len(rec['order'])} fragile {share:.4f} reached {reached} "
          f"twin err/bound logits {r['logits']:.4f} alpha {r['alpha']:.4f} confidence {r['confidence']:.4f} "
          f"(over the flat bound {flat:.4f}) max extra {o['extra'].max():.3e} wall {time.time() - t0:.1f} s", flush=True)
    assert share <= S["cap"], f"fragile share {share:.3f} above the scene's cap {S['cap']}"
    assert reached >= len(pix) // 2
    assert r["labels"] == 0
    assert r["logits"] <= 1.0 and r["alpha"] <= 1.0 and r["confidence"] <= 1.0, r


def test_production_scene_reaches_what_the_issue_names():
    S = sc.production(200_000, 13, 0)
    rec = ref.records(*args(S["s"], S["vm"], S["K"], S["W"], S["H"])[:4], S["vm"], S["K"], S["W"], S["H"])
    count, close = ref.tile_counts(rec, S["s"]["opacities"])
    assert count.sum() > 400_000 and close.sum() <= 5          # several radix passes' worth of keys, three-digit tile indices
    pix = S["pixels"]
    assert (pix[:, 0] >= 1056).sum() >= 100 and (pix[:, 1] >= 1584).sum() >= 100 and len(pix) >= 1800
    assert ((pix[:, 0] >= 1056) & (pix[:, 1] >= 1584)).sum() == 11 * 16          # the last, partial tile whole


def test_needle_sigma_error_exceeds_the_flat_band_and_meets_the_derived_one():
    # scales (2, 0.002, 0.002) turned pi / 4 about the view axis at z = 2, f = 120, 256 x 256
    W = H = 256
    s = dict(means=np.float32([[0, 0, 2]]), quats=sc._rot_z_quat(np.pi / 4)[None].astype(np.float32),
             scales=np.float32([[2, 0.002, 0.002]]), opacities=np.float32([0.9]))
    vm, K = np.eye(4, dtype=np.float32), np.float32([[120, 0, 128], [0, 120, 128], [0, 0, 1]])
    rec = ref.records(s["means"], s["quats"], s["scales"], s["opacities"], vm, K, W, H)
    worst, worst_used, mmax = 0.0, 0.0, 0.0
    for i, j in sc.all_pixels(W, H)[::7]:
        s64, s32, m = ref.sigma_pair(rec, i, j)
        err = abs(s32[0] - s64[0])
        assert err <= ref.SIGMA_GAMMA * ref.U32 * m[0]
        worst, mmax = max(worst, err), max(mmax, m[0])
        if 0 <= s64[0] <= np.log(255 * 0.9):
            worst_used = max(worst_used, err)
    print(f"sampled-cpu needle sigma: worst |sigma32 - sigma64| {worst:.3e} (where the pair is used {worst_used:.3e}) "
          f"max m {mmax:.3e} bound there {ref.SIGMA_GAMMA * ref.U32 * mmax:.3e}", flush=True)
    assert worst > 1e-3 and worst_used > 1e-4 and mmax > 1e4      # the old claim: a few 1e-6 relative, a band of 1e-5


# ---------------------------------------------------------------------------------------- the tests can fail
def test_reversed_ties_move_the_oracle_far_beyond_the_bound():
    a, b = sc.ties_scene(), sc.ties_scene(reverse=True)
    oa, ob = (ref.splat64(*args(S["s"], S["vm"], S["K"], S["W"], S["H"])) for S in (a, b))
    B = ref.value_bound(a["s"]["features"])
    good = ~(oa["fragile"] | ob["fragile"])
    moved = (np.abs(oa["logits"] - ob["logits"]).max(0) > 100 * B) & good
    assert np.array_equal(np.sort(a["s"]["opacities"]), np.sort(b["s"]["opacities"]))
    assert moved.sum() >= 0.3 * a["W"] * a["H"], f"only {moved.sum()} pixels move by more than 100 bounds"
    assert oa["visits"].max() > 256 and max(len(g) for g in a["groups"]) > 256
    z = ref.depth32(a["s"]["means"], a["vm"])
    assert all(len(np.unique(z[g])) == 1 for g in a["groups"])
    # the long group alone, reversed, moves its pixels as well: the order inside a run of more than 256 equal keys counts
    c = sc.ties_scene()
    g = c["groups"][-1]
    for k in c["s"]:
        c["s"][k][g] = c["s"][k][g[::-1]]
    oc = ref.splat64(*args(c["s"], c["vm"], c["K"], c["W"], c["H"]))
    assert ((np.abs(oa["logits"] - oc["logits"]).max(0) > 10 * B) & good & ~oc["fragile"]).sum() >= 100


def test_a_box_one_tile_short_loses_terms_far_above_the_bound():
    # floaters: a pixel of an image-corner tile adds a floater whose (clipped) box ends in that very tile
    S = sc.hard_scene("floaters")
    s, W, H = S["s"], S["W"], S["H"]
    rec = ref.records(*args(s, S["vm"], S["K"], W, H)[:4], S["vm"], S["K"], W, H)
    count, _ = ref.tile_counts(rec, s["opacities"])
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    floaters = np.nonzero(count == tiles)[0]
    assert len(floaters) >= 5
    B = ref.value_bound(s["features"])
    lost = 0
    for i, j in ((3, 2), (250, 251), (5, 250)):
        r = ref.pixel64(rec, i, j)
        g = rec["order"][r["sel"]]
        hit = np.isin(g, floaters)
        assert hit.any()
        lost += int((r["w"][hit, None] * np.abs(s["features"][g[hit]]) > 100 * B).any())
    assert lost == 3


def test_an_ignored_far_plane_moves_the_oracle_far_beyond_the_bound():
    S = sc.camera_scene("near_far")
    a = ref.splat64(*args(S["s"], S["vm"], S["K"], S["W"], S["H"]), **S["kw"])
    B = ref.value_bound(S["s"]["features"])
    z = ref.depth32(S["s"]["means"], S["vm"])
    assert (z < S["kw"]["near"]).sum() >= 60 and (z > S["kw"]["far"]).sum() >= 60
    for drop in ("far", "near"):
        kw = {k: v for k, v in S["kw"].items() if k != drop}
        b = ref.splat64(*args(S["s"], S["vm"], S["K"], S["W"], S["H"]), **kw)
        moved = (np.abs(a["logits"] - b["logits"]).max(0) > 100 * B) & ~a["fragile"] & ~b["fragile"]
        assert moved.sum() >= 0.1 * S["W"] * S["H"], (drop, moved.sum())


@pytest.mark.parametrize("kind,what", [("hard", "needles"), ("camera", "rolled"), ("production", (200_000, 13, 0))],
                         ids=lambda v: str(v).replace(" ", ""))
def test_a_flipped_b_leaves_the_bound(kind, what):
    S = build(kind, what)
    _, pix, o, tw = oracle_and_twin(S, flip_b=True)
    good = ~o["fragile"]
    B = ref.value_bound_at(S["s"]["features"], o)
    out = ((np.abs(tw["logits"] - o["logits"]) > B).any(1) & good).sum()
    assert out >= 0.2 * len(pix), f"only {out} of {len(pix)} pixels leave the bound"
