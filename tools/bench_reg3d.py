"""The 3D neighbourhood regulariser at the production shape: vp_knn_points, vp_neighbor_kl and vp_neighbor_kl_gradient against
what the same work costs through torch on the same GPU in the same run, JSON lines (metric reg3d_kernels) appended to --out
(default profiles/r23_reg3d.jsonl).

  python tools/bench_reg3d.py [--gaussians 1000000] [--classes 40 256] [--k 5] [--warmup 3] [--repeats 10]

Points: synthetic_gaussians.make_gaussians' means.  Legs, one JSON line each:
  search       vp_knn_points for the k - 1 nearest others of every Gaussian, launched in the grid's cell order (what
               NeighborTable does) and in the caller's order (the same result), the kernel alone between two events; the
               whole NeighborTable build (bucketing, search, reversed table) on the wall clock; and the reference's way
               restated here: torch.cdist of 1000 samples against 300 000 points plus topk, which is what one application of
               loss_cls_3d pays for 1000 points.
  loss P       neighbor_kl plus neighbor_kl_gradient over every row against a torch composite on the same table under
               autograd (softmax, log(p + 1e-10), row gather, KL, backward to the logits); the input bytes the fused path has
               to read (N P 4 for the log-sum-exp pass, S k P 4 forward, N (2 k - 1) P 4 backward, plus the gradient's N P 4
               written) over its time, as a share of this GPU's measured streaming-read rate; and the forward, and forward plus
               gradient, at every lanes-per-row layout the switch allows.
Method: --warmup calls, then --repeats calls each between two events on the stream, the median.  Needs a GPU."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd")]
import synthetic_gaussians  # noqa: E402
import voxel_to_gaussian_map  # noqa: E402
import voxproj_host  # noqa: E402


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def r4(t):
    return [round(v, 4) for v in t]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--classes", type=int, nargs="*", default=[40, 256])
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_reg3d.jsonl"))
    args = ap.parse_args(argv)
    N, k = args.gaussians, args.k
    dev = torch.device("cuda:0")
    g = synthetic_gaussians.make_gaussians(N, seed=0)
    pts = torch.from_numpy(np.ascontiguousarray(g["means"], np.float32)).to(dev)
    base = dict(metric="reg3d_kernels", N=N, k=k, warmup=args.warmup, repeats=args.repeats, device=torch.cuda.get_device_name(0))
    lines = []

    # ---- the search
    L = voxproj_host.lib()
    spts, perm, start, origin, h, dims = voxel_to_gaussian_map._bucket(pts, dev)
    org = (ctypes.c_double * 3)(*origin)
    idx = torch.empty((N, k - 1), dtype=torch.int32, device=dev)
    ident = torch.arange(N, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def search(q, si):
        voxproj_host.check(L.vp_knn_points(spts.data_ptr(), perm.data_ptr(), start.data_ptr(), org, ctypes.c_double(h), dims[0],
                                           dims[1], dims[2], q.data_ptr(), si.data_ptr(), N, k - 1, idx.data_ptr(), None, stream))

    cell = timed(lambda: search(spts, perm), 1, args.repeats)
    by_cell = torch.empty_like(idx).index_copy_(0, perm.long(), idx)
    plain = timed(lambda: search(pts, ident), 1, args.repeats)
    same = bool(torch.equal(by_cell, idx))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    table = voxproj_host.NeighborTable(pts, k)
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    assert torch.equal(table.nbr, idx)
    sub = pts[torch.randperm(N, generator=torch.Generator().manual_seed(0))[:min(N, 300_000)].to(dev)]

    def reference_way():
        return torch.cdist(sub[:1000], sub).topk(k, largest=False)

    ref = timed(reference_way, args.warmup, args.repeats)
    lines.append(dict(base, call="search", grid=dims, cell_size=h, knn_cell_order_ms=round(cell[0], 4),
                      knn_cell_order_ms_min_max=r4(cell[1:]), knn_caller_order_ms=round(plain[0], 4),
                      knn_caller_order_ms_min_max=r4(plain[1:]), caller_over_cell_order=round(plain[0] / cell[0], 3),
                      same_result=same, table_build_wall_ms=round(build_ms, 2), cdist_topk_1000_of_300000_ms=round(ref[0], 4),
                      cdist_topk_ms_min_max=r4(ref[1:]),
                      all_points_over_reference_1000=round(cell[0] / ref[0], 3)))

    # ---- the loss and its gradient
    probe = torch.empty(64 << 20, dtype=torch.float32, device=dev)
    stream_gbs = voxproj_host.stream_read_gbs(probe)
    del probe
    ns = table.all
    nb = ns.nbr.long()
    for P in args.classes:
        logits = torch.from_numpy(synthetic_gaussians.make_logits(g["classes"] % P, P, seed=0)).to(dev)
        ws = voxproj_host.SplatWorkspace()
        out = torch.empty((N, P), dtype=torch.float32, device=dev)
        coef = 2.0 / (N * k * P)

        def fused(lanes=0):
            stats, lse, _, _ = voxproj_host.neighbor_kl(logits, ns, lanes=lanes, workspace=ws)
            return stats, voxproj_host.neighbor_kl_gradient(logits, ns, lse, scale=2.0, lanes=lanes, out=out)

        def forward_only(lanes=0):
            return voxproj_host.neighbor_kl(logits, ns, lanes=lanes, workspace=ws)

        def composite():
            z = logits.detach().requires_grad_(True)
            p = torch.softmax(z, 1)
            lp = torch.log(p + 1e-10)
            kl = (p[:, None, :] * (lp[:, None, :] - lp[nb])).sum()
            loss = coef * kl
            grad, = torch.autograd.grad(loss, z)
            return loss, grad

        stats, grad = fused()
        t_loss, t_grad = composite()
        agree = dict(loss=float(abs(coef * stats[0] - t_loss.detach().double()) / t_loss.detach().double().abs()),
                     grad=float((grad - t_grad).abs().max() / t_grad.abs().max()))
        del t_grad
        f_ms = timed(fused, args.warmup, args.repeats)
        fw_ms = timed(forward_only, args.warmup, args.repeats)
        c_ms = timed(composite, 1, max(3, args.repeats // 3))
        nbytes = 4 * P * (N + N * k + N * (2 * k - 1) + N)
        lanes_ms, lanes_fused_ms = {}, {}
        for lanes in (4, 8, 16, 32, 64):
            if (P + lanes - 1) // lanes <= 4:
                lanes_ms[str(lanes)] = round(timed(lambda: forward_only(lanes), 1, args.repeats)[0], 4)
                lanes_fused_ms[str(lanes)] = round(timed(lambda: fused(lanes), 1, args.repeats)[0], 4)
        lines.append(dict(base, call="loss", P=P, fused_ms=round(f_ms[0], 4), fused_ms_min_max=r4(f_ms[1:]),
                          forward_ms=round(fw_ms[0], 4), composite_ms=round(c_ms[0], 4), composite_ms_min_max=r4(c_ms[1:]),
                          composite_over_fused=round(c_ms[0] / f_ms[0], 3), input_bytes=nbytes,
                          fused_gb_per_s=round(nbytes / f_ms[0] / 1e6, 2), stream_read_gb_per_s=round(stream_gbs, 1),
                          share_of_stream_rate=round(nbytes / f_ms[0] / 1e6 / stream_gbs, 4), forward_ms_by_lanes=lanes_ms, fused_ms_by_lanes=lanes_fused_ms,
                          lanes_chosen=max(8 if P > 8 else 4, min(64, 1 << max((P + 3) // 4 - 1, 0).bit_length())), relative_difference=agree))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        for line in lines:
            print(json.dumps(line), flush=True)
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
