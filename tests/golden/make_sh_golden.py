"""Generates tests/golden/sh_golden.npz by RUNNING the reference's own utils/sh_utils.eval_sh on the CPU in float64, as its
renderer does (gaussian_renderer/__init__.py:67-72):

    dir    = (means - campos) / |means - campos|
    colour = clamp_min(eval_sh(d, features.transpose(1, 2), dir) + 0.5, 0)

with autograd for the gradients of sum(colour * upstream) with respect to the coefficients [N,K,3] and, through the
normalised direction, the means, on the seeded inputs of tests/sh_reference.make_inputs.  One case per active degree d = 0 .. 3
(Dmax = 3: the coefficients beyond d are present and must receive zeros).  Recorded per case: the inputs (f32), the colours,
grad_sh and grad_means (f64).  It also prints, for the larger inputs the GPU tests use, the share of clamped channels and of
channels within 1e-4 of the kink.

Run by hand where a checkout of the reference exists; the tests only read the npz.

Usage:  python tests/golden/make_sh_golden.py --reference /path/to/reference/checkout
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sh_reference as shref  # noqa: E402

N = 96
MAX_DEGREE = 3


def evaluate(eval_sh, inp, degree, want_grad=True):
    sh = torch.cat([torch.from_numpy(inp["f_dc"]).double()[:, None], torch.from_numpy(inp["f_rest"]).double()], dim=1)
    sh.requires_grad_(want_grad)
    means = torch.from_numpy(inp["means"]).double().requires_grad_(want_grad)
    p = means - torch.from_numpy(inp["campos"]).double()
    pre = eval_sh(degree, sh.transpose(1, 2), p / p.norm(dim=1, keepdim=True)) + 0.5
    colour = torch.clamp_min(pre, 0.0)
    if want_grad:
        (colour * torch.from_numpy(inp["grad_colors"]).double()).sum().backward()
    return pre.detach().numpy(), colour.detach().numpy(), sh.grad, means.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project (holds utils/sh_utils.py)")
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    from utils.sh_utils import eval_sh

    out = {"n": np.int64(N), "max_degree": np.int64(MAX_DEGREE)}
    for d in range(MAX_DEGREE + 1):
        inp = shref.make_inputs(N, MAX_DEGREE, 100 + d)
        _, colour, gsh, gmeans = evaluate(eval_sh, inp, d)
        for name, a in inp.items():
            out[f"{name}_{d}"] = a
        # degree 0 does not touch the direction: autograd then leaves the means without a gradient, which is a zero
        out[f"colors_{d}"], out[f"grad_sh_{d}"] = colour, gsh.numpy()
        out[f"grad_means_{d}"] = gmeans.numpy() if gmeans is not None else np.zeros((N, 3))
    path = os.path.join(HERE, "sh_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    for Dmax in range(MAX_DEGREE + 1):
        for d in range(Dmax + 1):
            pre, _, _, _ = evaluate(eval_sh, shref.make_inputs(4099, Dmax, 7), d, want_grad=False)
            print(f"N 4099 Dmax {Dmax} d {d}: {100 * (pre < 0).mean():.2f} % clamped, "
                  f"{100 * (np.abs(pre) < 1e-4).mean():.4f} % within 1e-4 of the kink")


if __name__ == "__main__":
    main()
