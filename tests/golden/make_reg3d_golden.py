"""Generates tests/golden/reg3d_golden.npz by calling the REFERENCE's own ``loss_cls_3d`` (utils/loss_utils.py:74-115) on the
CPU on four seeded point sets.  Usage: python tests/golden/make_reg3d_golden.py --reference <checkout of the reference>

The reference is called with max_points = sample_size = N, so that it draws no subset and its one randperm is a permutation
of all points: the loss (a mean over the samples) and the gradient do not depend on it.  The gradient is torch autograd's,
through softmax, with respect to the logits.

The reference picks its neighbours from an fp32 cdist; on a plainly jittered lattice that disagrees with the exact sets at
about 0.1 % of the points, where the last neighbour kept and the first one dropped are closer than about 1e-4 relative.  The
jitter of every point whose margin (d_dropped - d_kept) / d_dropped is below 2e-3 is therefore redrawn until none is left,
and the generator asserts that the reference's way (cdist + topk on the final points) then picks the brute-force sets at
EVERY point.  The relative difference between the reference's fp32 loss and the float64 statement is recorded per case: it is
the margin the golden comparison gets on top of the derived bound.

Arrays only: per case i  c{i}_points f32 [N,3], c{i}_logits f32 [N,P], c{i}_k, c{i}_nbr i32 [N,k-1] (brute force),
c{i}_loss f32, c{i}_grad f32 [N,P], c{i}_rel_diff f64 (loss, relative), c{i}_grad_diff f64 (the largest absolute difference
between the reference's fp32 gradient and the statement's: the gradient comparison's margin), c{i}_rounds."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import reg3d_reference as r3  # noqa: E402

CASES = [dict(n=12, P=5, k=5, seed=1), dict(n=9, P=40, k=5, seed=2), dict(n=6, P=256, k=8, seed=3), dict(n=9, P=17, k=16, seed=4)]
CELL, JITTER, MARGIN, SCALE = 0.07, 0.35, 2e-3, 2.0


def separated_points(n, k, seed):
    """The jittered lattice with every point's kept / dropped margin at least MARGIN: (points f32, rounds of redraws)."""
    g = np.random.default_rng(seed)
    ax = np.arange(n) * CELL
    base = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    pts = (base + g.uniform(-JITTER, JITTER, base.shape) * CELL).astype(np.float32)
    for rounds in range(100):
        _, d2 = r3.knn_brute(pts, k)                                  # k others: k - 1 kept, the k-th is the first dropped
        d = np.sqrt(d2)
        bad = np.flatnonzero((d[:, k - 1] - d[:, k - 2]) / d[:, k - 1] < MARGIN)
        if not len(bad):
            return pts, rounds
        pts[bad] = (base[bad] + g.uniform(-JITTER, JITTER, (len(bad), 3)) * CELL).astype(np.float32)
    raise RuntimeError("the margins did not clear in 100 rounds")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference (holds utils/loss_utils.py)")
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_loss_utils", os.path.join(args.reference, "utils", "loss_utils.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for i, c in enumerate(CASES):
        pts, rounds = separated_points(c["n"], c["k"], c["seed"])
        N, k, P = len(pts), c["k"], c["P"]
        logits = r3.smooth_logits(pts, P, c["seed"] + 100)
        nbr, _ = r3.knn_brute(pts, k - 1)
        feats = torch.from_numpy(pts)
        # the reference's neighbour choice, restated on the same tensors: every set must be the brute-force one
        picked = torch.cdist(feats, feats).topk(k, largest=False).indices.numpy()
        want = np.concatenate([np.arange(N)[:, None], nbr], 1)
        assert all(set(picked[j].tolist()) == set(want[j].tolist()) for j in range(N)), "the reference's fp32 neighbour sets differ"
        z = torch.from_numpy(logits).requires_grad_(True)
        torch.manual_seed(c["seed"])
        loss = ref.loss_cls_3d(feats, torch.softmax(z, 1), k=k, lambda_val=SCALE, max_points=N, sample_size=N)
        loss.backward()
        st = r3.statement64(logits, None, nbr, k, scale=SCALE)
        rel = abs(float(loss.detach()) - st["loss"]) / abs(st["loss"])
        gdiff = float(np.abs(z.grad.numpy().astype(np.float64) - st["grad"]).max())
        gerr = gdiff / float(np.abs(st["grad"]).max())
        print(f"case {i}: N {N} P {P} k {k}, {rounds} redraw round(s), loss {float(loss.detach()):.8g} (float64 statement {st['loss']:.10g}, "
              f"relative difference {rel:.2e}), gradient off by {gerr:.2e} of its largest element")
        out.update({f"c{i}_points": pts, f"c{i}_logits": logits, f"c{i}_k": np.int32(k), f"c{i}_nbr": nbr.astype(np.int32),
                    f"c{i}_loss": np.float32(float(loss.detach())), f"c{i}_grad_diff": np.float64(gdiff), f"c{i}_grad": z.grad.numpy().astype(np.float32),
                    f"c{i}_rel_diff": np.float64(rel), f"c{i}_rounds": np.int32(rounds)})
    path = os.path.join(HERE, "reg3d_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
