"""View-dependent colour at the production shape: vp_sh_colors and vp_sh_colors_backward (with and without grad_means) against
a torch composite of the same formula under autograd and against a plain device copy of the same byte count, all on the same
GPU in the same run; JSON lines (metric sh_kernels) appended to --out (default profiles/r26_sh.jsonl).

  python tools/bench_sh.py [--gaussians 1000000] [--degree 3] [--warmup 3] [--repeats 10] [--inner 20]

Legs, one JSON line each:
  forward            f_dc, f_rest, means in; colors and the clamp bytes out (217 B per Gaussian at degree 3)
  backward_means     grad_colors, clamp bytes, means, f_rest in; grad_dc, grad_rest, grad_means out (409 B)
  backward_no_means  grad_colors, clamp bytes, means in; grad_dc, grad_rest out (217 B)
Each line has the launch's time (outputs made beforehand, nothing but the C call between the events), the bytes it must move,
the rate, the rate of torch's device-to-device copy of the same byte count (half read, half written) and the kernel's share of
that rate, and the time of the torch composite (one element-wise multiply-add per coefficient row; its backward through
autograd).
Method: --warmup windows, then --repeats rounds in which the sides alternate; a window is --inner calls between two events on
the stream, so a 0.1 ms kernel is timed over milliseconds; the median window over --inner.  Needs a GPU."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd")]
import voxproj_host  # noqa: E402

# the real SH constants by degree, unsigned (the signs stand with the polynomials below, as in csrc/vp_sh.h)
K0, K1 = 0.28209479177387814, 0.4886025119029199
K2A, K2B, K2C = 1.0925484305920792, 0.31539156525252005, 0.5462742152960396
K3A, K3B, K3C, K3D, K3E = 0.5900435899266435, 2.890611442640554, 0.4570457994644658, 0.3731763325901154, 1.445305721320277


def timed_alternating(fns, warmup, repeats, inner):
    """{name: (median, min, max) ms per call}: the callables take turns inside every round, ``inner`` calls per window."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / inner)
    return {k: (round(float(np.median(v)), 5), round(float(np.min(v)), 5), round(float(np.max(v)), 5)) for k, v in ms.items()}


def torch_basis(d, degree):
    """Y_1 .. Y_{(degree+1)^2 - 1} of unit directions d [N,3], each [N]: the polynomials of include/voxproj_ext.h."""
    x, y, z = d.unbind(1)
    Y = []
    if degree > 0:
        Y += [-K1 * y, K1 * z, -K1 * x]
    if degree > 1:
        xx, yy, zz = x * x, y * y, z * z
        Y += [K2A * x * y, -K2A * y * z, K2B * (2 * zz - xx - yy), -K2A * x * z, K2C * (xx - yy)]
    if degree > 2:
        Y += [-K3A * y * (3 * xx - yy), K3B * x * y * z, -K3C * y * (4 * zz - xx - yy), K3D * z * (2 * zz - 3 * xx - 3 * yy),
              -K3C * x * (4 * zz - xx - yy), K3E * z * (xx - yy), -K3A * x * (xx - 3 * yy)]
    return Y


def torch_sh_colors(f_dc, f_rest, means, campos, degree):
    """max(0.5 + sum_k Y_k(dir) sh[k], 0) on plain tensors, one element-wise multiply-add per coefficient row (a batched
    contraction of [N,K] with [N,K,3] is slower by an order of magnitude in torch: N products of 1 x 15 by 15 x 3)."""
    p = means - campos
    pre = K0 * f_dc
    for k, Yk in enumerate(torch_basis(p / p.norm(dim=1, keepdim=True), degree)):
        pre = pre + Yk[:, None] * f_rest[:, k]
    return torch.clamp_min(pre + 0.5, 0.0)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--degree", type=int, default=3, help="Dmax and the active degree")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_sh.jsonl"))
    args = ap.parse_args(argv)
    N, D = args.gaussians, args.degree
    kr = voxproj_host.sh_rest_width(D)
    if not torch.cuda.is_available():
        raise SystemExit("bench_sh.py needs a GPU: there is no CPU path and no time without one")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    f_dc = torch.randn(N, 3, generator=gen).to(dev)
    f_rest = (0.4 * torch.randn(N, kr, 3, generator=gen)).to(dev)
    means = (4.0 * torch.rand(N, 3, generator=gen) - 2.0).to(dev)
    up = torch.randn(N, 3, generator=gen).to(dev)
    cam = [0.3, -0.2, 0.1]
    vm = torch.eye(4, dtype=torch.float64)
    vm[:3, 3] = -torch.tensor(cam, dtype=torch.float64)
    campos_t = torch.tensor(cam, device=dev)
    L = voxproj_host.lib()
    c_cam = (ctypes.c_float * 3)(*cam)
    stream = torch.cuda.current_stream(dev).cuda_stream
    colors, clamped = voxproj_host.sh_colors(f_dc, f_rest, means, vm, D)
    g_dc, g_rest, g_means = voxproj_host.sh_colors_backward(f_dc, f_rest, means, vm, D, up, clamped)
    p = voxproj_host._ptr

    def forward():
        voxproj_host.check(L.vp_sh_colors(p(f_dc), p(f_rest), p(means), c_cam, N, D, D, p(colors), p(clamped), stream))

    def backward(with_means):
        voxproj_host.check(L.vp_sh_colors_backward(None, p(f_rest) if with_means else None, p(means), c_cam, N, D, D, p(up),
                                                   p(clamped), p(g_dc), p(g_rest), p(g_means) if with_means else None, stream))

    # the torch composite, and how far it is from the kernels
    leaf = [t.clone().requires_grad_(True) for t in (f_dc, f_rest, means)]
    ref = torch_sh_colors(*leaf, campos_t, D)
    ref.backward(up)
    grad = [t.grad if t.grad is not None else torch.zeros_like(t) for t in leaf]       # degree 0 leaves two of them untouched
    gap = dict(colors=float((ref.detach() - colors).abs().max()), grad_dc=float((grad[0] - g_dc).abs().max()),
               grad_rest=float((grad[1] - g_rest).abs().max()) if kr else 0.0, grad_means=float((grad[2] - g_means).abs().max()))

    def torch_forward():
        with torch.no_grad():
            torch_sh_colors(f_dc, f_rest, means, campos_t, D)

    def torch_both(with_means):
        def run():
            a = [f_dc.detach().requires_grad_(True), f_rest.detach().requires_grad_(True), means.detach().requires_grad_(with_means)]
            torch_sh_colors(*a, campos_t, D).backward(up)
        return run

    nbytes = dict(forward=N * (12 + 12 * kr + 12 + 12 + 1), backward_means=N * (12 + 1 + 12 + 12 * kr + 12 + 12 * kr + 12),
                  backward_no_means=N * (12 + 1 + 12 + 12 + 12 * kr))
    copies = {}
    for leg, b in nbytes.items():                       # a copy of b / 2 bytes reads b / 2 and writes b / 2
        src = torch.empty(b // 2, dtype=torch.uint8, device=dev).random_(0, 255)
        copies[leg] = (src, torch.empty_like(src))
    base = dict(metric="sh_kernels", N=N, max_degree=D, degree=D, warmup=args.warmup, repeats=args.repeats, inner=args.inner,
                device=torch.cuda.get_device_name(0))
    t = timed_alternating(dict(forward=forward, copy_forward=lambda: copies["forward"][1].copy_(copies["forward"][0]),
                               backward_means=lambda: backward(True),
                               copy_backward_means=lambda: copies["backward_means"][1].copy_(copies["backward_means"][0]),
                               backward_no_means=lambda: backward(False),
                               copy_backward_no_means=lambda: copies["backward_no_means"][1].copy_(copies["backward_no_means"][0])),
                          args.warmup, args.repeats, args.inner)
    tt = timed_alternating(dict(forward=torch_forward, backward_means=torch_both(True), backward_no_means=torch_both(False)),
                           args.warmup, args.repeats, max(1, args.inner // 10))
    lines = []
    for leg, b in nbytes.items():
        k, c = t[leg], t["copy_" + leg]
        rate, copy_rate = b / k[0] / 1e6, 2 * (b // 2) / c[0] / 1e6
        line = dict(base, call=leg, bytes=b, bytes_per_gaussian=b // N, kernel_ms=k[0], kernel_ms_min_max=k[1:],
                    kernel_gb_per_s=round(rate, 1), copy_ms=c[0], copy_ms_min_max=c[1:], copy_gb_per_s=round(copy_rate, 1),
                    share_of_copy_rate=round(rate / copy_rate, 4), torch_ms=tt[leg][0], torch_ms_min_max=tt[leg][1:])
        if leg == "forward":
            line.update(torch_over_kernel=round(tt[leg][0] / k[0], 2), max_abs_gap_to_torch=gap)
        else:                                           # the composite's time holds its forward too: autograd needs it
            line.update(torch_forward_and_backward_over_kernels=round(tt[leg][0] / (k[0] + t["forward"][0]), 2))
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        for line in lines:
            print(json.dumps(line), flush=True)
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
