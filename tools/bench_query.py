"""The text query (vp_query_features) at the shapes of stage 5.1, one JSON line per leg: N in {200k, 2M, 16M} voxel rows,
C = 512, P in {13, 100, 512} prompts, float16 and float32 rows, logits written or not (labels and margin always).

  query_ms             HIP events around --steps calls after --warmup (per call; the text normalisation is included)
  algo_GB              N*C*s (rows) + N*P*4 (logits, when on) + N*(4+4) (labels, margin) + P*C*4 (text)
  frac_8TBs / frac_copy  algo_GB / query time against 8 TB/s (spec) and the 6.29 TB/s measured float4 copy
  tflops               2*N*C*P / query time
  torch_ms             the torch composite on the same tensors: F.normalize(x.float()) @ F.normalize(t).T * scale, softmax,
                       topk(2) -> label and margin, in row blocks of <= 2^30 logits (HIP events, same steps); checked
                       against: labels where the float32 gap of the composite exceeds 2B, max |logit difference| and
                       |margin difference| (first 200k rows)

python tools/bench_query.py [--steps K] [--warmup W] [--n 200000 2000000 16000000] [--p 13 100 512] [--dtype f16 f32]
[--logits on off]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import voxproj_host  # noqa: E402

HBM_SPEC_GBS, COPY_GBS = 8000.0, 6290.0
C = 512


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


def composite(x, t, scale=1.0):
    """The torch composite; in row blocks of at most 2^30 logits when the whole would be larger: torch's kernels on this
    stack faulted on a [16M, 512] logits tensor (8.2e9 elements) in one piece."""
    rows = max(1, (1 << 30) // t.shape[0])
    tn = F.normalize(t, dim=1)
    if rows >= x.shape[0]:
        lg = scale * (F.normalize(x.float(), dim=1) @ tn.T)
        top = lg.softmax(dim=1).topk(2, dim=1)
        return lg, top.indices[:, 0], top.values[:, 0] - top.values[:, 1]
    lg = torch.empty((x.shape[0], t.shape[0]), device=x.device)
    lab = torch.empty(x.shape[0], dtype=torch.long, device=x.device)
    mg = torch.empty(x.shape[0], device=x.device)
    for lo in range(0, x.shape[0], rows):
        blk = scale * (F.normalize(x[lo:lo + rows].float(), dim=1) @ tn.T)
        top = blk.softmax(dim=1).topk(2, dim=1)
        lg[lo:lo + rows], lab[lo:lo + rows], mg[lo:lo + rows] = blk, top.indices[:, 0], top.values[:, 0] - top.values[:, 1]
    return lg, lab, mg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, nargs="+", default=[200_000, 2_000_000, 16_000_000])
    ap.add_argument("--p", type=int, nargs="+", default=[13, 100, 512])
    ap.add_argument("--dtype", nargs="+", default=["f16", "f32"])
    ap.add_argument("--logits", nargs="+", default=["off", "on"])
    ap.add_argument("--no-torch", action="store_true", help="skip the composite (counter runs)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(7)
    B = 2.0 ** -11 + 2 * C * 2.0 ** -24
    for dt in args.dtype:
        dtype = torch.float16 if dt == "f16" else torch.float32
        for N in args.n:
            x = torch.empty((N, C), dtype=dtype, device=dev)
            for lo in range(0, N, 1 << 20):
                x[lo:lo + (1 << 20)].normal_(generator=g)
            for P in args.p:
                t = torch.randn((P, C), generator=g, device=dev)
                torch_ms, ref = None, None
                if not args.no_torch:
                    torch_ms = timed(lambda: composite(x, t), args.steps, args.warmup)
                    k = min(N, 200_000)
                    lg_r, lab_r, mg_r = composite(x[:k], t)
                    ref = (lg_r, lab_r, mg_r)
                for lo_on in args.logits:
                    want = lo_on == "on"
                    ms = timed(lambda: voxproj_host.query_features(x, t, want_logits=want, check=False), args.steps, args.warmup)
                    lab, lg, mg = voxproj_host.query_features(x, t, want_logits=want, check=True)
                    s = x.element_size()
                    algo = (N * C * s + (N * P * 4 if want else 0) + N * 8 + P * C * 4) / 1e9
                    line = dict(leg=f"{dt}-N{N}-P{P}-logits_{lo_on}", dtype=dt, N=N, C=C, P=P, logits=want, query_ms=round(ms, 4),
                                algo_GB=round(algo, 4), GBps=round(algo / ms * 1e3, 1),
                                frac_8TBs=round(algo / ms * 1e3 / HBM_SPEC_GBS, 3), frac_copy=round(algo / ms * 1e3 / COPY_GBS, 3),
                                tflops=round(2.0 * N * C * P / ms / 1e9, 2))
                    if ref is not None:
                        lg_r, lab_r, mg_r = ref
                        k = lab_r.numel()
                        srt = lg_r.topk(2, dim=1).values if P > 1 else None
                        clear = (srt[:, 0] - srt[:, 1] > 2 * B) if P > 1 else torch.ones(k, dtype=torch.bool, device=dev)
                        line.update(torch_ms=round(torch_ms, 4), speedup=round(torch_ms / ms, 2),
                                    labels_match_clear=bool(torch.equal(lab[:k].long()[clear], lab_r[clear])),
                                    max_margin_diff=float((mg[:k] - mg_r).abs().max()))
                        if want:
                            line["max_logit_diff"] = float((lg[:k] - lg_r).abs().max())
                    del lab, lg, mg
                    print(json.dumps(line), flush=True)
                del ref
                torch.cuda.empty_cache()
            del x
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
