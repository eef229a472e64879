"""Time the label sums and one Lloyd iteration of feature_clusters on fp16 tables of 512 channels (1 M, 4 M and 16 M rows,
K = 10, 64, 256), and beside them, in the same process, the streaming-read rate of the device and a torch composite of the
same iteration on the same tensors.

One JSON line per (rows, K), device-event times (median of --reps windows after --warmup):
  inv_norms_ms           voxproj_host.row_inv_norms (once per table, not per iteration)
  assign_ms              voxproj_host.query_features with the centroids as the text, labels only
  label_sums_ms          voxproj_host.label_sums with row_scale = the inverse norms, on the labels of that assignment
  table_bytes            what the sum pass reads once: rows * C * 2;  sums_fraction_of_stream = table_bytes / label_sums_ms over
                         stream_read_gbs, the rate voxproj_host.stream_read_gbs measures on this table in this run (the WHOLE
                         call against one read of the table: sort, plan and combine are inside it)
  lloyd_iteration_ms     assign + label_sums + the [K,C] table on the host (feature_clusters._lloyd, max_iter = 1 minus its last assign)
  torch_iteration_ms     matmul + argmax of the raw fp16 rows against fp16 centroids (the argmax of the cosine needs no row
                         norm), then index_add_ (float atomics) of the rows scaled in float32, in chunks of --torch_chunk rows
                         (the float32 copy of a chunk is chunk * C * 4 bytes);  torch_index_add_ms: the second half alone, on
                         the labels label_sums_ms was timed on
  skew                   true for the extra line with half the rows in label 0
The split of label_sums by stage (sort, plan, sum, combine) comes from a kernel trace of ``--stages ROWS K`` in a run of its own:
that mode only repeats the call.  GPU only: without a device the program fails, it does not fall back.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-semantic-segmentation_amd"))
C = 512


def timed(fn, warmup, reps):
    import torch
    out = None
    for _ in range(warmup):
        out = fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), out


def make_table(n, K, dev, seed=30):
    """fp16 [n, C] on the device, built in slices: K planted directions with noise and row norms in [0.5, 4]."""
    import torch
    gen = torch.Generator(device=dev).manual_seed(seed)
    dirs = torch.nn.functional.normalize(torch.randn(K, C, device=dev, generator=gen), dim=1)
    rows = torch.empty((n, C), dtype=torch.float16, device=dev)
    step = 1 << 20
    for b in range(0, n, step):
        m = min(step, n - b)
        lab = torch.randint(0, K, (m,), device=dev, generator=gen)
        x = dirs[lab] + torch.randn(m, C, device=dev, generator=gen) * (0.5 / C ** 0.5)
        rows[b:b + m] = (x * (0.5 + 3.5 * torch.rand(m, 1, device=dev, generator=gen))).half()
    return rows, dirs


def torch_iteration(rows, cent16, inv, K, chunk):
    import torch
    labels = torch.empty(rows.shape[0], dtype=torch.int64, device=rows.device)
    sums = torch.zeros((K, C), dtype=torch.float32, device=rows.device)
    for b in range(0, rows.shape[0], chunk):
        part = rows[b:b + chunk]
        lab = (part @ cent16.T).argmax(dim=1)
        labels[b:b + chunk] = lab
        sums.index_add_(0, lab, part.float() * inv[b:b + chunk, None])
    return labels, sums


def main(argv=None):
    ap = argparse.ArgumentParser(description="Time label sums and a Lloyd iteration beside the stream rate and a torch composite")
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 20, 1 << 22, 1 << 24])
    ap.add_argument("--k", type=int, nargs="+", default=[10, 64, 256])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch_chunk", type=int, default=1 << 20, help="rows per index_add_ of the torch composite")
    ap.add_argument("--stages", type=int, nargs=2, default=None, metavar=("ROWS", "K"), help="only repeat label_sums at one shape (for a kernel trace)")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    args = ap.parse_args(argv)
    import torch

    import feature_clusters as fc
    import gaussian_views
    import voxproj_host as vh
    dev = gaussian_views.require_gpu("bench_cluster")
    ws = vh.SplatWorkspace()

    def emit(line):
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(json.dumps(line) + "\n")

    if args.stages:
        n, K = args.stages
        rows, dirs = make_table(n, K, dev)
        inv = vh.row_inv_norms(rows)[0]
        labels = vh.query_features(rows, dirs, want_logits=False, want_margin=False, check=False)[0]
        t, _ = timed(lambda: vh.label_sums(rows, labels, K, row_scale=inv, check=False, workspace=ws), args.warmup, args.reps)
        emit(dict(stages_of=dict(rows=n, K=K, C=C), label_sums_ms=t, calls=args.warmup + args.reps))
        return
    for n in args.rows:
        rows, _ = make_table(n, max(args.k), dev)
        stream = vh.stream_read_gbs(rows.view(torch.float32))
        t_inv, (inv, _) = timed(lambda: vh.row_inv_norms(rows), args.warmup, args.reps)
        for K in args.k:
            cent = torch.from_numpy(next(fc.seed_centroids(rows, np.arange(n), K, seed=0, n_init=1))).to(dev)
            for skew in (False, True) if K == args.k[-1] else (False,):
                t_assign, out = timed(lambda: vh.query_features(rows, cent, want_logits=False, want_margin=False, check=False),
                                      args.warmup, args.reps)
                labels = out[0]
                if skew:
                    labels = labels.clone()
                    labels[::2] = 0                                   # half the rows in one label
                t_sums, (_, counts, _) = timed(lambda: vh.label_sums(rows, labels, K, row_scale=inv, check=False, workspace=ws),
                                                  args.warmup, args.reps)

                def iteration():
                    lab = vh.query_features(rows, cent, want_logits=False, want_margin=False, check=False)[0]
                    S, cnt, _ = vh.label_sums(rows, lab, K, row_scale=inv, check=False, workspace=ws)
                    Sh = S.cpu().numpy()
                    return fc.objective64(Sh, cent_h), fc.next_centroids(Sh, cnt.cpu().numpy(), cent_h)

                cent_h = cent.cpu().numpy()
                t_iter, _ = timed(iteration, args.warmup, args.reps)
                cent16 = cent.half()
                t_torch, _ = timed(lambda: torch_iteration(rows, cent16, inv, K, args.torch_chunk), 1, max(args.reps // 2, 1))
                t_tsum, _ = timed(lambda: [torch.zeros((K, C), device=dev).index_add_(
                    0, labels[b:b + args.torch_chunk].long().clamp_min(0), rows[b:b + args.torch_chunk].float() * inv[b:b + args.torch_chunk, None])
                    for b in range(0, n, args.torch_chunk)], 1, max(args.reps // 2, 1))
                table_bytes = n * C * 2
                emit(dict(rows=n, K=K, C=C, dtype="float16", skew=skew, part_rows=max(256, -(-n // 32768)),
                          largest_label=int(counts.max()), stream_read_gbs=stream, inv_norms_ms=t_inv,
                          inv_norms_gbs=table_bytes / (t_inv * 1e-3) / 1e9, assign_ms=t_assign, label_sums_ms=t_sums,
                          table_bytes=table_bytes, label_sums_gbs=table_bytes / (t_sums * 1e-3) / 1e9,
                          sums_fraction_of_stream=table_bytes / (t_sums * 1e-3) / 1e9 / stream, lloyd_iteration_ms=t_iter,
                          torch_iteration_ms=t_torch, torch_index_add_ms=t_tsum, torch_chunk_rows=args.torch_chunk,
                          torch_chunk_f32_bytes=args.torch_chunk * C * 4))
        del rows, inv


if __name__ == "__main__":
    main()
