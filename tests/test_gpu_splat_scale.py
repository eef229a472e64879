"""Gaussian splatting at the size it ships at (1600x1067, 200 k and 1 M Gaussians of synthetic_gaussians, D = 13 and 32,
trajectory views as tools/bench_splat.py renders them), forward and backward, against the sampled-pixel float64 reference
splat_reference.splat64_at / splat_grad_reference.splat_grad64_at: a few whole 16x16 tiles (the image's corners, the last tile
column, the partial last tile row) plus scattered pixels of a seeded generator, about 2 000 in all, each against every kept
Gaussian with no tiles and no support box.  What only this size exercises: tile keys with three-digit tile indices, offsets
in the hundreds of thousands, several radix passes, long runs, and the emission slots the backward writes to.

Bounds, on the sampled pixels the reference does not mark fragile (splat_reference's conditioning-aware bands):
  labels      exact
  logits      |err| <= 1e-4 max|f| + 1e-6 + extra_c,   extra_c = sum_g w_g |f_gc| E_g (splat_reference.value_bound_at)
  alpha       |err| <= 1e-5 + sum_g w_g E_g
  confidence  |err| <= 2 max_c bound + 1e-6
  n_isect     the sum of the reference's tile counts (splat_reference.tile_counts); a Gaussian with a box edge within 1e-9
              of an integer may differ by the tiles one step of that edge adds, and there are at most 5 of those
  gradients   |err| <= 1e-4 M + 1e-6 max|G| + X (splat_grad_reference.grad_bound and splat_grad64_at's X_*), upstream
              gradients nonzero on the sampled non-fragile pixels only; grad_features / grad_opacities of the fused geometry
              call bit-identical to the plain backward's.
test_splat_sampled_cpu.py holds the reference to the dense oracle and the bound to an fp32 twin, on these very scenes.
Every case prints its worst error / bound (profiles/r11_splat_test_accuracy.txt keeps one run's figures).
"""
import os
import sys
import time

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import splat_grad_reference as gref  # noqa: E402
import splat_reference as ref  # noqa: E402
import splat_scenes as sc  # noqa: E402
import voxproj_host  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def ratio(err, bound):
    return float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0


def gpu_forward(S):
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in S["s"].items()}
    ws = voxproj_host.SplatWorkspace()
    r = voxproj_host.splat_features(t["means"], t["quats"], t["scales"], t["opacities"], t["features"], S["vm"], S["K"], S["W"],
                                    S["H"], want_logits=True, want_alpha=True, workspace=ws, check=False, **S["kw"])
    return t, ws, r


def reference(S):
    s = S["s"]
    pix = S["pixels"] if S["pixels"] is not None else sc.all_pixels(S["W"], S["H"])
    rec = ref.records(s["means"], s["quats"], s["scales"], s["opacities"], S["vm"], S["K"], S["W"], S["H"], **S["kw"])
    o = ref.splat64_at(s["means"], s["quats"], s["scales"], s["opacities"], s["features"], S["vm"], S["K"], S["W"], S["H"], pix,
                       value_tol=2 * ref.value_bound(s["features"]), rec=rec, **S["kw"])
    return rec, pix, o


def check_forward(name, S, r, rec, pix, o, min_reached):
    good = ~o["fragile"]
    share = 1.0 - good.mean()
    reached = int((good & (o["visits"] > 0)).sum())
    rows, cols = torch.from_numpy(pix[:, 0]).to(DEV), torch.from_numpy(pix[:, 1]).to(DEV)
    at = lambda img: img[..., rows, cols].cpu().numpy()  # noqa: E731
    B = ref.value_bound_at(S["s"]["features"], o)
    el = np.abs(at(r.logits).T.astype(np.float64) - o["logits"])[good]
    ea = np.abs(at(r.alpha) - o["alpha"])[good]
    ec = np.abs(at(r.confidence) - o["confidence"])[good]
    ba, bc = (1e-5 + o["extra_alpha"])[good], (2 * B.max(1) + 1e-6)[good]
    wrong = int((at(r.labels) != o["label"])[good].sum())
    count, close = ref.tile_counts(rec, S["s"]["opacities"])
    print(f"scale-accuracy forward {name}: pixels {len(pix)} fragile {share:.4f} reached {reached} err/bound logits "
          f"{ratio(el, B[good]):.4f} (over the flat bound {ratio(el, ref.value_bound(S['s']['features'])):.4f}) alpha "
          f"{ratio(ea, ba):.4f} confidence {ratio(ec, bc):.4f} wrong labels {wrong} n_isect {r.n_isect} reference "
          f"{int(count.sum())} close {int(close.sum())} most Gaussians at a pixel {int(o['visits'].max())}", flush=True)
    assert share <= S["cap"], f"fragile share {share:.3f} above the scene's cap"
    assert reached >= min_reached, f"only {reached} non-fragile sampled pixels are reached by a Gaussian"
    assert wrong == 0, f"{wrong} labels differ"
    assert (el <= B[good]).all(), f"logit error {el.max():.3e} over its bound"
    assert (ea <= ba).all(), f"alpha error {ea.max():.3e} over its bound"
    assert (ec <= bc).all(), f"confidence error {ec.max():.3e} over its bound"
    # one step of a close edge adds or drops at most one row or column of the box's tiles
    tiles_x, tiles_y = (S["W"] + 15) // 16, (S["H"] + 15) // 16
    assert close.sum() <= 5
    assert abs(r.n_isect - int(count.sum())) <= int(close.sum()) * (tiles_x + tiles_y), (r.n_isect, int(count.sum()))
    return good


def check_backward(name, S, t, ws, r, rec, pix, o, good, seed, min_nonzero):
    """Upstream gradients on the sampled non-fragile pixels only; the plain backward and the fused geometry call."""
    s, W, H = S["s"], S["W"], S["H"]
    D = s["features"].shape[1]
    rng = np.random.default_rng(seed)
    Gp = np.where(good[:, None], rng.normal(size=(len(pix), D)), 0.0).astype(np.float32)
    Gap = np.where(good, rng.normal(size=len(pix)), 0.0).astype(np.float32)
    rows, cols = torch.from_numpy(pix[:, 0]).to(DEV), torch.from_numpy(pix[:, 1]).to(DEV)
    G = torch.zeros((D, H, W), device=DEV)
    Ga = torch.zeros((H, W), device=DEV)
    G[:, rows, cols] = torch.from_numpy(Gp.T.copy()).to(DEV)
    Ga[rows, cols] = torch.from_numpy(Gap).to(DEV)
    N = len(s["means"])
    gf, go = voxproj_host.splat_rasterize_backward(t["features"], N, W, H, r.n_isect, ws, G, Ga)
    g = voxproj_host.splat_rasterize_backward_geometry(t["means"], t["quats"], t["scales"], t["features"], S["vm"], S["K"], W,
                                                       H, r.n_isect, ws, G, Ga, eps2d=S["kw"].get("eps2d", 0.3),
                                                       want_screen=True)
    torch.cuda.synchronize()
    assert torch.equal(g["features"], gf) and torch.equal(g["opacities"], go), "not the plain backward's bits"
    e = gref.splat_grad64_at(s["means"], s["quats"], s["scales"], s["opacities"], s["features"], S["vm"], S["K"], W, H, pix, Gp,
                             Gap, rec=rec, **S["kw"])
    out = {}
    for key, got in (("f", gf), ("o", go), ("screen", g["screen"])):
        want = e["grad_" + key]
        bound = gref.grad_bound(e["M_" + key], [Gp, Gap]) + e["X_" + key]
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        out[key] = (err, bound, int((want != 0).sum()))
    print(f"scale-accuracy backward {name}: err/bound grad_f {ratio(*out['f'][:2]):.4f} grad_o {ratio(*out['o'][:2]):.4f} "
          f"grad_screen {ratio(*out['screen'][:2]):.4f} nonzero {[v[2] for v in out.values()]}", flush=True)
    for key, (err, bound, nz) in out.items():
        assert nz >= min_nonzero, f"grad_{key}: only {nz} nonzero reference entries"
        assert (err <= bound).all(), f"grad_{key} error over its bound at {np.unravel_index((err - bound).argmax(), err.shape)}"
    zero = torch.from_numpy(e["added"] == 0).to(DEV)
    assert (gf[zero] == 0).all() and (go[zero] == 0).all() and (g["screen"][zero] == 0).all()
    for k in ("means", "quats", "scales"):
        assert g[k].isfinite().all() and (g[k][zero] == 0).all() and (g[k] != 0).any()


def run_case(name, S, min_reached, min_nonzero, seed=0):
    t0 = time.time()
    rec, pix, o = reference(S)
    t1 = time.time()
    t, ws, r = gpu_forward(S)
    good = check_forward(name, S, r, rec, pix, o, min_reached)
    check_backward(name, S, t, ws, r, rec, pix, o, good, seed, min_nonzero)
    print(f"scale-accuracy wall {name}: forward reference {t1 - t0:.1f} s, all {time.time() - t0:.1f} s", flush=True)


@pytest.mark.parametrize("D,view", [(13, 0), (13, 1), (32, 0), (32, 1)])
def test_production_200k(D, view):
    S = sc.production(200_000, D, view)
    assert len(S["pixels"]) >= 1800
    run_case(f"200k D={D} view {view}", S, min_reached=len(S["pixels"]) * 3 // 4, min_nonzero=500, seed=D + view)


def test_production_1m():
    S = sc.production(1_000_000, 13, 1, n_scatter=150, few=True)
    run_case("1M D=13 view 1", S, min_reached=len(S["pixels"]) * 3 // 4, min_nonzero=200, seed=5)
