"""Generates tests/golden/photo_loss_golden.npz by RUNNING the reference's own utils/loss_utils.py (l1_loss, ssim) on the
CPU in float64, with autograd for the gradient of

    loss = (1 - lambda) l1_loss(image, gt) + lambda (1 - ssim(image, gt)),   lambda = 0.2

(train_unified_lift.py's image term), on seeded inputs of tests/photo_loss_reference.make_inputs.  Recorded per case: the
two inputs (f32), l1, ssim, loss, the gradient with respect to the image; and once the reference's 121-weight window
(create_window(11, 1)), whose weights are fp32 products of the row: the float64 statement is compared on that window.

Run by hand where a checkout of the reference exists; the tests only read the npz.

Usage:  python tests/golden/make_photo_loss_golden.py --reference /path/to/reference/checkout
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import photo_loss_reference as pref  # noqa: E402

LAMBDA = 0.2
CASES = (("noise", 3, 5, 7, 11), ("smooth", 3, 37, 21, 12), ("binary", 1, 16, 16, 13), ("flat", 3, 17, 16, 14),
         ("equal", 4, 11, 11, 15), ("noise", 1, 1, 1, 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project (holds utils/loss_utils.py)")
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    from utils import loss_utils

    out = {"window2d": loss_utils.create_window(11, 1)[0, 0].numpy(), "lambda_dssim": np.float64(LAMBDA),
           "cases": np.array(["%s,%d,%d,%d,%d" % c for c in CASES])}
    assert out["window2d"].dtype == np.float32
    for i, (kind, C, W, H, seed) in enumerate(CASES):
        x, y = pref.make_inputs(kind, C, W, H, seed)
        img = torch.from_numpy(x).double().requires_grad_(True)
        gt = torch.from_numpy(y).double()
        l1 = loss_utils.l1_loss(img, gt)
        ss = loss_utils.ssim(img, gt)
        loss = (1.0 - LAMBDA) * l1 + LAMBDA * (1.0 - ss)
        loss.backward()
        out[f"x{i}"], out[f"y{i}"] = x, y
        out[f"l1_{i}"], out[f"ssim_{i}"], out[f"loss_{i}"] = l1.item(), ss.item(), loss.item()
        out[f"grad_{i}"] = img.grad.numpy()
    path = os.path.join(HERE, "photo_loss_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
