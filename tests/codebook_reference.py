"""The contract of vp_codebook_assoc and vp_codebook_loss (include/voxproj.h) in float64, and the bounds the GPU tests hold
the fp32 kernels to.

``statement64`` is the contract as per-id loops in torch float64: for every mask id its pixels, their logits against the
code book, the softmax summed into the id's score row; then, per id with a code, the cross-entropy against that code and
the distance |s - B_v| over the confident pixels.  ``want_grad`` adds the gradients of the two sums with respect to the
code book by torch autograd on the CPU (the image is a constant).  ``closed_form`` is the header's formulas in numpy for any
dtype, with the pixels visited in any order: in float64 it is checked against autograd (tests/test_codebook_cpu.py), in
float32 in other orders it is the yardstick below.

Bounds.  The inputs are float32 values, exact in both arithmetics, so every difference is fp32 rounding; u = 2^-24.

  id_pixels and stats[2] are integers: exact.
  Sums over pixels (score, grad_cls, grad_cluster, stats[0], stats[1]): the worst-case bound of a sum of W H terms says
    nothing useful.  The yardstick is the error of ``closed_form`` in float32 against float64 in four other summation
    orders: the pixels AND the channels (the order of a logit's D-term sum) visited in descending order and in three seeded
    permutations (numpy's pairwise sums and its BLAS), the largest error over the elements of an output and the four
    orders.  The device may be off by 8 times that, because the orders legitimately differ.  Only where a yardstick is
    exactly 0 is it replaced by one rounding of the largest value, u max |.|; a non-zero yardstick is never raised.
    (The first version permuted the pixels only.  On an image of one pixel its four orders were then one and the same
    computation, and the "largest of four" a single sample: at 1 x 1, D = 64, K = 5 numpy's logits were off by 8.5e-7 but
    their errors cancelled in the softmax to 2.2e-9, and the device, whose logits were off by 1.6e-6 -- v_mfma_f32_16x16x4_f32
    is a chain of D fused multiply-adds, reproduced bit for bit on the CPU -- stood at 2.7e-8 = 0.45 u, 1.55 times that
    yardstick.  Every larger case was below 0.1 of its bound.  With the channels permuted as well the four orders are four
    computations at any size.)
  Logits, per pixel: z_k = sum_c B_kc f_c is D products and D - 1 additions in fp32, in whatever order:
        |z32 - z64| <= dz_p = (D + 1) u max_k sum_c |B_kc f_pc|.                                            (logit_bound)
  pixel_loss = (max + log sum_k exp(z_k - max)) - z_v, per pixel.  log-sum-exp moves by at most dz when its arguments move,
    and z_v by dz: 2 dz.  Then the arithmetic: z - max is rounded once, u |z - max| on the exponent, which weighs
    x e^-x <= 0.37 per term; expf is within 1 ulp = 2 u; the sum of K positive terms adds K u: in all at most (2 K + 4) u on
    the sum, relative, hence absolute on its logarithm; logf's own rounding 2 u |log sum| with 1 <= sum <= K; the addition
    of the maximum u |lse|; the subtraction u |ce|:
        |ce32 - ce64| <= 2 dz_p + (2 K + 4 + 2 log K + |lse| + |ce|) u.                                     (pixel_bound)
  pred and stats[3] rest on an argmax.  A logit moves by at most dz_p, the gap of two by 2 dz_p: a pixel whose two largest
    DISTINCT logits are closer than 2 dz_p in float64 is fragile.  (Codes with identical rows have identical logits in any
    arithmetic that treats the codes alike, here and on the device: such a tie is exact, not fragile, and the lowest code
    wins; the gap is therefore taken over the distinct rows of the code book.)  pred is compared on the other pixels only;
    stats[3] must lie between the mismatches among them and that number plus the fragile pixels whose id has a code.
    Fragile pixels may be at most 1 % of a case's valid pixels: ``fragile_share`` is checked on the CPU for the generator's
    cases (tests/test_codebook_cpu.py) and again in every GPU case.
  Every factor above was fixed before the kernels ran against it, the channel permutation excepted, whose history is
  told above.  Measured afterwards on the MI355X over tests/test_gpu_codebook.py's cases, the worst case of any output as
  a fraction of its bound: score 0.215, grad_cls 0.125, grad_cluster 0.045, stats[0] 0.218, stats[1] 0.125, pixel_loss
  0.168 (the worst element of any case); fragile pixels: at most 1 of a case's 8698 valid ones.
"""
import numpy as np
import torch

U = 2.0 ** -24
MAX_IDS = 256
MAX_CODES = 256


def _maps(image, ids, conf, conf_min, ignore_id):
    D, H, W = image.shape
    n = H * W
    idn = np.asarray(ids).reshape(-1).astype(np.int64)
    valid = (idn >= 0) & (idn < MAX_IDS) & (idn != ignore_id)
    confident = valid if conf is None else valid & (np.asarray(conf, np.float32).reshape(-1) > np.float32(conf_min))
    return D, H, W, n, idn, valid, confident


def _labels(assign, idn, valid, K):
    """v_p: the code of the pixel's id, -1 where the id has none."""
    if assign is None:
        return np.full(idn.shape, -1, np.int64)
    a = np.asarray(assign).astype(np.int64)
    a = np.where((a >= 0) & (a < K), a, -1)
    return np.where(valid, a[np.clip(idn, 0, MAX_IDS - 1)], -1)


def statement64(image, ids, codebook, assign=None, conf=None, *, conf_min=0.2, ignore_id=-1, want_grad=False):
    """image [D,H,W] float32, ids [H,W], codebook [K,D] float32, assign [256] or None (no loss), conf [H,W] or None.
    Returns a dict of numpy arrays: score [256,K], id_pixels [256], pred [n], gap [n] (of the two largest distinct logits),
    dz [n] (logit_bound), valid, part [n], v [n], pixel_loss [n], lse [n], stats (4 floats), and with ``want_grad``
    grad_cls, grad_cluster [K,D]."""
    D, H, W, n, idn, valid, confident = _maps(image, ids, conf, conf_min, ignore_id)
    K = codebook.shape[0]
    f = torch.tensor(np.asarray(image, np.float64).reshape(D, n).T.copy())
    B = torch.tensor(np.asarray(codebook, np.float64), requires_grad=want_grad)
    v = _labels(assign, idn, valid, K)
    part = confident & (v >= 0)
    score = np.zeros((MAX_IDS, K))
    id_pixels = np.zeros(MAX_IDS, np.int64)
    pred = np.full(n, -1, np.int64)
    gap = np.full(n, np.inf)
    lse = np.zeros(n)
    pixel_loss = np.zeros(n)
    distinct = np.sort(np.unique(np.asarray(codebook), axis=0, return_index=True)[1])
    ss = (f * f).sum(-1)
    s_hat = f / (torch.sqrt(ss) + 1e-6)[:, None]
    ce_total = torch.zeros((), dtype=torch.float64)
    dist_total = torch.zeros((), dtype=torch.float64)
    for l in np.unique(idn[valid]).tolist():
        sel = torch.from_numpy(valid & (idn == l))
        z = f[sel] @ B.T
        P = torch.softmax(z, dim=1)
        score[l] = P.detach().sum(0).numpy()
        id_pixels[l] = int(sel.sum())
        pred[sel.numpy()] = torch.argmax(z.detach(), dim=1).numpy()          # the first of equal maxima: the lowest code
        if len(distinct) > 1:
            top = torch.topk(z.detach()[:, distinct], 2, dim=1).values
            gap[sel.numpy()] = (top[:, 0] - top[:, 1]).numpy()
        lse[sel.numpy()] = torch.logsumexp(z.detach(), dim=1).numpy()
        code = int(v[np.flatnonzero(valid & (idn == l))[0]])
        if code < 0:
            continue
        selp = torch.from_numpy(part & (idn == l))
        if not bool(selp.any()):
            continue
        zp = f[selp] @ B.T
        ce = torch.logsumexp(zp, dim=1) - zp[:, code]
        ce_total = ce_total + ce.sum()
        pixel_loss[selp.numpy()] = ce.detach().numpy()
        dist_total = dist_total + torch.norm(s_hat[selp] - B[code], dim=1).sum()
    absf = np.abs(np.asarray(image, np.float64).reshape(D, n).T)
    dz = (D + 1) * U * (absf @ np.abs(np.asarray(codebook, np.float64)).T).max(1)
    out = dict(score=score, id_pixels=id_pixels, pred=pred, gap=gap, dz=dz, valid=valid, part=part, v=v, lse=lse,
               pixel_loss=pixel_loss, D=D, H=H, W=W, K=K,
               stats=(float(ce_total.detach()), float(dist_total.detach()), float(part.sum()),
                      float(((v >= 0) & (pred != v)).sum())))
    if want_grad:
        zero = np.zeros((K, D))
        out["grad_cls"] = torch.autograd.grad(ce_total, B, retain_graph=True)[0].numpy() if ce_total.requires_grad else zero
        out["grad_cluster"] = torch.autograd.grad(dist_total, B)[0].numpy() if dist_total.requires_grad else zero
    return out


def closed_form(image, ids, codebook, assign=None, conf=None, *, conf_min=0.2, ignore_id=-1, dtype=np.float64, order=None,
                chan=None):
    """include/voxproj.h's formulas in numpy arithmetic of ``dtype``; ``order``: a permutation of the pixels, ``chan``: one
    of the channels, the orders in which they are visited (another summation order; None: ascending).  Returns a dict:
    score, id_pixels, pred, pixel_loss, grad_cls, grad_cluster, stats."""
    T = dtype
    D, H, W, n, idn, valid, confident = _maps(image, ids, conf, conf_min, ignore_id)
    K = codebook.shape[0]
    order = np.arange(n) if order is None else np.asarray(order)
    chan = np.arange(D) if chan is None else np.asarray(chan)
    f = np.ascontiguousarray(np.asarray(image, T).reshape(D, n).T[order][:, chan])
    B = np.ascontiguousarray(np.asarray(codebook, T)[:, chan])
    v = _labels(assign, idn, valid, K)[order]
    idn, valid, confident = idn[order], valid[order], confident[order]
    part = confident & (v >= 0)
    z = f @ B.T
    mx = z.max(1)
    e = np.exp(z - mx[:, None])
    den = e.sum(1, dtype=T)
    P = e / den[:, None]
    onehot_id = np.zeros((n, MAX_IDS), T)
    onehot_id[valid, idn[valid]] = 1
    score = onehot_id.T @ P
    id_pixels = np.bincount(idn[valid], minlength=MAX_IDS)
    pred = np.where(valid, z.argmax(1), -1)
    onehot_v = np.zeros((n, K), T)
    onehot_v[part, v[part]] = 1
    zv = (z * onehot_v).sum(1, dtype=T)
    ce = np.where(part, (mx + np.log(den)) - zv, 0).astype(T)
    Q = np.where(part[:, None], P - onehot_v, 0).astype(T)
    grad_cls = Q.T @ f
    r = np.sqrt((f * f).sum(1, dtype=T))
    s_hat = f / (r + T(1e-6))[:, None]
    d = s_hat - B[np.where(part, v, 0)]
    dist = np.sqrt((d * d).sum(1, dtype=T))
    with np.errstate(invalid="ignore", divide="ignore"):
        wrow = np.where((part & (dist > 0))[:, None], -d / dist[:, None], 0).astype(T)
    grad_cluster = onehot_v.T @ wrow
    dist = np.where(part, dist, 0).astype(T)
    back, cback = np.argsort(order), np.argsort(chan)
    return dict(score=score, id_pixels=id_pixels, pred=pred[back], pixel_loss=ce[back], grad_cls=grad_cls[:, cback],
                grad_cluster=grad_cluster[:, cback],
                stats=(float(ce.sum(dtype=T)), float(dist.sum(dtype=T)), float(part.sum()),
                       float(((v >= 0) & (pred != v)).sum())))


def orders(n, D):
    """The summation orders of the yardstick, (pixels, channels) each: descending, and three seeded permutations."""
    return [(np.arange(n)[::-1], np.arange(D)[::-1])] + [(np.random.default_rng(seed).permutation(n),
                                                          np.random.default_rng(seed + 10).permutation(D)) for seed in (1, 2, 3)]


SUMS = ("score", "grad_cls", "grad_cluster", "stats0", "stats1")


def bounds(image, ids, codebook, assign=None, conf=None, *, conf_min=0.2, ignore_id=-1, verbose=True):
    """The yardstick of the module's docstring: a dict with 8 E (or the floor where E is exactly 0) for each of SUMS, and
    E itself under "E"."""
    kw = dict(conf_min=conf_min, ignore_id=ignore_id)
    a = closed_form(image, ids, codebook, assign, conf, dtype=np.float64, **kw)
    n = image.shape[1] * image.shape[2]

    def pick(res, key):
        return np.asarray(res["stats"][int(key[-1])]) if key.startswith("stats") else res[key]
    E = dict.fromkeys(SUMS, 0.0)
    for order, chan in orders(n, image.shape[0]):
        b = closed_form(image, ids, codebook, assign, conf, dtype=np.float32, order=order, chan=chan, **kw)
        assert (b["id_pixels"] == a["id_pixels"]).all() and b["stats"][2] == a["stats"][2]
        for key in SUMS:
            E[key] = max(E[key], float(np.abs(pick(a, key) - pick(b, key).astype(np.float64)).max()))
    out = {key: 8 * (E[key] if E[key] > 0 else U * float(np.abs(pick(a, key)).max())) for key in SUMS}
    out["E"] = E
    if verbose:
        print("float32 numpy against float64, largest over %d orders: " % len(orders(n, image.shape[0])) +
              "  ".join(f"{key} {E[key]:.3e}" for key in SUMS))
    return out


def pixel_bound(ref):
    """[n]: the bound on |pixel_loss - ce| of the module's docstring; ``ref`` from statement64."""
    K = ref["K"]
    return 2 * ref["dz"] + (2 * K + 4 + 2 * np.log(K) + np.abs(ref["lse"]) + np.abs(ref["pixel_loss"])) * U


def fragile(ref):
    """[n] bool: the valid pixels whose argmax fp32 may take the other way."""
    return ref["valid"] & (ref["gap"] < 2 * ref["dz"])


def fragile_share(ref):
    nv = int(ref["valid"].sum())
    return float(fragile(ref).sum()) / nv if nv else 0.0


# ------------------------------------------------------------------------------------------------
# The generator of the random cases (tests/test_gpu_codebook.py runs them on the device, tests/test_codebook_cpu.py checks
# on the CPU that the float64 statement alone keeps every one of them under the cap on fragile pixels).
# ------------------------------------------------------------------------------------------------
IGNORE = 7
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def make_case(D, K, W, H, layout, seed, conf_kind="null", assign_kind="identity", ties=False):
    """(image f32 [D,H,W], ids i32 [H,W], codebook f32 [K,D], assign i32 [256], conf f32 [H,W] or None).  Rows scatter round
    one direction per id, the first codes sit near some of those directions, the others are random.  layout: "one", "two",
    "37", "256", "edge" (ids -1, 256, the ignored id, INT_MIN, INT_MAX; id 42 confined to the first tile of 64 pixels, id 43
    with a pixel in every tile; ids 50 and 51 alternating pixel by pixel over a stretch).  ``ties``: code 1 is a copy of code
    0's row (K >= 2), and some rows point along it, so that the lowest of two equal logits decides."""
    g = np.random.default_rng(seed)
    n = W * H
    tiles = (n + 63) // 64
    if layout == "one":
        ids = np.full(n, 5)
    elif layout == "two":
        ids = (np.arange(n) * 2 // max(n, 1)) * 200                    # ids 0 and 200
    elif layout == "37":
        ids = 3 + 6 * (g.integers(0, 37, (n + 8) // 9).repeat(9)[:n])   # runs of nine pixels
    elif layout == "256":
        ids = g.permutation(np.arange(n) % 256)
    else:
        assert layout == "edge"
        ids = 10 + g.integers(0, 5, (n + 4) // 5).repeat(5)[:n]
        if n >= 256:
            ids[128:224] = 50 + np.arange(96) % 2                       # alternating pixel by pixel, across a tile's end
            ids[n // 2:n // 2 + 12] = np.array([-1, 256, IGNORE, INT_MIN, INT_MAX, 300] * 2)
            ids[:64][g.choice(64, 20, replace=False)] = 42              # confined to the first tile
            ids[np.arange(tiles) * 64 + g.integers(0, 64, tiles) % np.minimum(64, n - np.arange(tiles) * 64)] = 43
    dirs = g.normal(size=(258, D))
    f = dirs[np.clip(ids, -1, 256) + 1] * g.uniform(0.5, 1.6, (n, 1)) + 0.4 * g.normal(size=(n, D))
    codebook = g.normal(size=(K, D)) * 0.7
    near = min(K, 40)
    codebook[:near] = dirs[g.integers(0, 258, near)] * 0.9 + 0.1 * g.normal(size=(near, D))
    if ties and K >= 2:
        codebook[1] = codebook[0]
        sel = g.choice(n, max(n // 8, 1), replace=False)
        f[sel] = 3.0 * codebook[0] * g.uniform(0.8, 1.2, (len(sel), 1)) + 0.05 * g.normal(size=(len(sel), D))
    if n > 1:
        f[n // 3] = 0.0                                                 # the pixel with f = 0
    present = np.unique(ids[(ids >= 0) & (ids < 256)])
    assign = np.full(256, -1, np.int64)
    if assign_kind != "none":
        assign[present[:K]] = g.permutation(K)[:len(present[:K])] if assign_kind != "identity" else np.arange(len(present[:K]))
        if assign_kind == "some":
            assign[present[::3]] = -1
            assign[3] = K                                               # outside [0, K): takes no part either
    conf = None
    if conf_kind == "below":
        conf = g.uniform(0.0, 0.2, n)
    elif conf_kind == "mixed":
        conf = g.uniform(0.0, 1.0, n)
        conf[::7] = 0.2                                                 # exactly the threshold: not confident
    image = np.ascontiguousarray(f.T.reshape(D, H, W)).astype(np.float32)
    return (image, ids.reshape(H, W).astype(np.int32), codebook.astype(np.float32), assign.astype(np.int32),
            None if conf is None else conf.reshape(H, W).astype(np.float32))


SIZES = [(1, 1), (37, 19), (130, 67), (145, 113)]   # 145 x 113 = 16385 pixels = 257 tiles: the smallest image at which the
                                                    # 256-workgroup cap makes a workgroup walk more than one tile
DS = [1, 3, 16, 17, 64]
KS = [1, 5, 16, 17, 256]


def shape_cases():
    """Every D and every K meet every size once (D[i] with K[(i + shift) % 5], the shift moving with the size; at 130 x 67
    the shift is 0, so D = 64 meets K = 256), the layouts, confidence maps and assignments rotating through.  A list of
    make_case keyword dicts."""
    layouts = ["edge", "37", "two", "one", "edge"]
    confs = ["null", "mixed", "null", "below", "mixed"]
    assigns = ["identity", "some", "perm", "identity", "none"]
    out = []
    for si, (W, H) in enumerate(SIZES):
        shift = (si + 2) % 4 if (W, H) != (130, 67) else 0
        for i, D in enumerate(DS):
            j = (i + si) % 5
            out.append(dict(D=D, K=KS[(i + shift) % 5], W=W, H=H, layout=layouts[j], conf_kind=confs[(j + i) % 5],
                            assign_kind=assigns[(i + 2 * si) % 5], seed=1000 * D + W, ties=False))
    out.append(dict(D=16, K=256, W=130, H=67, layout="256", conf_kind="mixed", assign_kind="perm", seed=5, ties=False))
    out.append(dict(D=3, K=5, W=130, H=67, layout="256", conf_kind="null", assign_kind="identity", seed=6, ties=False))
    out.append(dict(D=16, K=17, W=37, H=19, layout="37", conf_kind="null", assign_kind="perm", seed=7, ties=True))
    return out


def case_name(c):
    return f"D{c['D']}-K{c['K']}-{c['W']}x{c['H']}-{c['layout']}-{c['conf_kind']}-{c['assign_kind']}" + ("-ties" if c["ties"] else "")
