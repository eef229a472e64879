"""The projector's transpose at the bench's shapes, one JSON line per leg: vp_first_hit_ids (the march alone) and
vp_render_features (dst[p] = rows[hit[p]]) on one seeded call of 60 views of each workload (R2: the benign room of bench.py's
metric config, R2T / A1: the hand-held trajectory), C = 512, float32 and float16 destinations.

  render_ms / first_hit_ms   HIP events around --steps launches after --warmup (per launch)
  algo_GB                    n_pixels*4 (IDs) + n_pixels*C*s (dst) + N_touched*C*4 (each touched row read once)
  frac_8TBs / frac_copy      algo_GB / render time against 8 TB/s (spec) and the 6.29 TB/s measured float4 copy

The scenes come from bench.py's workload table (read, not edited).  python tools/bench_render.py [--steps K] [--warmup W]
[--workloads R2 R2T A1] [--views 60]"""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import voxproj_host  # noqa: E402

HBM_SPEC_GBS, COPY_GBS = 8000.0, 6290.0


def bench_module():
    argv = sys.argv
    sys.argv = ["bench.py"]
    try:
        spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        sys.argv = argv
    return m


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workloads", nargs="*", default=["R2", "R2T", "A1"])
    ap.add_argument("--views", type=int, default=60)
    ap.add_argument("--dtypes", nargs="*", default=["f32", "f16"])
    a = ap.parse_args()
    bm = bench_module()
    dev = torch.device("cuda", 0)
    dst_pool = None
    for name in a.workloads:
        n_vox, _, W, H, C = bm.WORKLOADS[name]
        s = bm.workload_scene(name)
        V = min(a.views, s.n_views)
        n_rows = s.n_vox + 1
        occ = torch.from_numpy(s.occ.astype(np.int64))[None].to(dev).contiguous()
        vmi = torch.from_numpy(np.ascontiguousarray(s.c2w[:V])).reshape(-1).to(dev)
        intr = torch.from_numpy(s.intr[None].copy()).to(dev)
        ws = voxproj_host.Workspace()
        march = lambda: voxproj_host.first_hit_ids(occ, vmi, intr, s.opts(), s.grid_origin, s.voxel_size, H, W, n_rows, workspace=ws)  # noqa: E731
        ids = march()                                        # builds the tables; the timed calls reuse them
        fh_ms = timed(march, a.steps, a.warmup)
        n_pix = ids.numel()
        u = torch.unique(ids)
        n_touched = int((u > 0).sum())
        hit_frac = float((ids > 0).float().mean())
        rows = torch.randn(n_rows, C, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        need = n_pix * C * 4
        if dst_pool is None or dst_pool.numel() < need:
            dst_pool = None
            torch.cuda.empty_cache()
            dst_pool = torch.empty(need, dtype=torch.uint8, device=dev)
        for dt in a.dtypes:
            tdt, esize = (torch.float32, 4) if dt == "f32" else (torch.float16, 2)
            out = dst_pool[:n_pix * C * esize].view(tdt).view(tuple(ids.shape) + (C,))
            ms = timed(lambda: voxproj_host.render_features(ids, rows, dtype=tdt, out=out, check=False), a.steps, a.warmup)
            algo = n_pix * 4 + n_pix * C * esize + n_touched * C * 4
            gbs = algo / ms / 1e6
            print(json.dumps({"leg": f"render_{name}_{dt}", "workload": name, "views": V, "W": W, "H": H, "C": C, "dst": dt,
                              "n_pixels": n_pix, "n_touched": n_touched, "hit_fraction": round(hit_frac, 4),
                              "render_ms": round(ms, 4), "first_hit_ms": round(fh_ms, 4), "algo_GB": round(algo / 1e9, 3),
                              "GBps": round(gbs, 1), "frac_8TBs": round(gbs / HBM_SPEC_GBS, 4),
                              "frac_copy": round(gbs / COPY_GBS, 4), "steps": a.steps, "warmup": a.warmup}), flush=True)
        ws.release()
        del ids, rows, occ


if __name__ == "__main__":
    main()
