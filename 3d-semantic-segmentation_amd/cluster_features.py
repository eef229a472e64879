"""Cluster a feature table without prompts: what is in here?

Counterpart of the reference's script/debug_checks_scripts/voxel_cluster_to_ply.py (sklearn KMeans on the raw rows, on the
CPU), with the metric every other tool of this project uses: spherical k-means, on the GPU (feature_clusters.fit).

Sub-commands (both take --k 10 [--n_init 4] [--max_iter 100] [--seed 0] [--init CENTROIDS.npy] --out X.npz [--ply X.ply]
[--no_logits] [--device N]):
  voxels     --vox ALL_nonzero_voxel_features_*.pt of the aggregator
  gaussians  --gauss_feats LIFTED.pt of lift_gaussian_features.py

X.npz has the schema of ``query_voxel_features.py``, so ``render_semantics_logits.py --logit_path X.npz`` draws cluster maps
as it draws prompt maps: labels int16 [n] (-1 for an all-zero or non-finite row), logits f32 [n,K] (the cosine to each
centroid, zeros for a row left out; omitted with --no_logits), prompts cluster_00 ..., colors uint8 [n,3] (the query tool's
palette); on top of it centroids f32 [K,C], counts int64 [K], objective and n_iter.  --ply: the points coloured by cluster.
Runs on the GPU only; there is no CPU path.
"""
import argparse

import numpy as np
import torch

import feature_clusters
import query_voxel_features as qvf
import voxproj_host

N_CLUSTERS = 10                                   # the reference scripts' N_CLUSTERS


def load_rows(args):
    """(xyz float32 [n,3], rows [n,C]) of the sub-command's input file."""
    if args.cmd == "voxels":
        xyz, feats, _ = qvf.load_voxels(args.vox)
        return xyz, feats
    import lift_gaussian_features
    xyz, feats, _ = lift_gaussian_features.load_lifted(args.gauss_feats)
    return xyz, feats


def cluster(rows, args):
    """feature_clusters.fit by the command line's options, and the logits of one last query: (result, logits or None)."""
    init = np.load(args.init) if args.init else None
    r = feature_clusters.fit(rows, args.k, init=init, seed=args.seed, n_init=args.n_init, max_iter=args.max_iter)
    logits = None
    if not args.no_logits:
        logits = voxproj_host.query_features(rows, r.centroids, want_margin=False, check=False)[1]
        logits = torch.where((r.labels >= 0)[:, None], logits, torch.zeros((), dtype=logits.dtype, device=logits.device))
    return r, logits


def build_parser():
    ap = argparse.ArgumentParser(description="Cluster a feature table by cosine (spherical k-means on the GPU)")
    sub = ap.add_subparsers(dest="cmd", required=True)

    def common(p):
        p.add_argument("--k", type=int, default=N_CLUSTERS, help="number of clusters")
        p.add_argument("--n_init", type=int, default=4, help="restarts; the highest objective is kept")
        p.add_argument("--max_iter", type=int, default=100)
        p.add_argument("--seed", type=int, default=0)
        p.add_argument("--init", default=None, help="explicit centroids [K, C] (.npy): no seeding, no restarts")
        p.add_argument("--out", required=True, help="output .npz (the schema of query_voxel_features.py)")
        p.add_argument("--ply", default=None, help="also write the points coloured by cluster (ASCII PLY)")
        p.add_argument("--no_logits", action="store_true", help="leave the [n, K] cosines out of the .npz")
        p.add_argument("--device", type=int, default=None, help="GPU index (default: the current device)")

    v = sub.add_parser("voxels", help="cluster the aggregator's per-voxel rows")
    v.add_argument("--vox", required=True, help="ALL_nonzero_voxel_features_*.pt of the aggregator")
    common(v)
    g = sub.add_parser("gaussians", help="cluster the Gaussians' own lifted rows")
    g.add_argument("--gauss_feats", required=True, help="LIFTED.pt of lift_gaussian_features.py")
    common(g)
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if not 1 <= args.k <= 1024:
        ap.error(f"--k must be in [1, 1024], not {args.k}")
    if args.n_init < 1 or args.max_iter < 1:
        ap.error("--n_init and --max_iter must be >= 1")
    if not torch.cuda.is_available():
        raise RuntimeError("cluster_features runs on the GPU: there is no CPU path")
    dev = torch.device("cuda", torch.cuda.current_device() if args.device is None else args.device)
    xyz, feats = load_rows(args)
    rows = feats.to(dev)
    if rows.dtype not in (torch.float16, torch.float32):
        rows = rows.float()
    r, logits = cluster(rows, args)
    lab = r.labels.cpu().numpy()
    prompts = [f"cluster_{k:02d}" for k in range(args.k)]
    colors = qvf.label_colors(lab, args.k)
    lg = logits.cpu().numpy() if logits is not None else np.zeros((len(lab), 0), np.float32)
    qvf.write_npz(args.out, lab, lg, prompts, colors)
    d = dict(np.load(args.out))
    if logits is None:
        del d["logits"]
    d.update(centroids=r.centroids.cpu().numpy(), counts=r.counts.cpu().numpy(), objective=np.float64(r.objective),
             n_iter=np.int64(r.n_iter))
    np.savez(args.out, **d)
    print(f"[CLUSTER] {len(lab)} rows, {r.n_valid} clustered into K = {args.k} ({r.n_zero} all-zero and {r.n_nonfinite} "
          f"non-finite row(s) left out), {r.n_iter} iteration(s){'' if r.converged else ' (max_iter reached)'}, "
          f"objective {r.objective:.6f}, inertia {r.inertia:.6f} -> {args.out}")
    if r.empty:
        print(f"[CLUSTER] label(s) {r.empty} kept their centroid in the last iteration (no rows)")
    if args.ply:
        qvf.write_ply(args.ply, xyz.numpy(), colors)
        print(f"[CLUSTER] coloured points -> {args.ply}")
    if logits is not None:
        qvf.summary(lab, lg, prompts)
    else:
        for k, c in enumerate(r.counts.tolist()):
            print(f"  {prompts[k]:20s} (idx={k}): count={c}")


if __name__ == "__main__":
    main()
