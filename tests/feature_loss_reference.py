"""The contract of vp_feature_loss and vp_feature_loss_gradient (include/voxproj.h) in float64 numpy, and the bounds the GPU
tests hold the fp32 kernels to.

The inputs of the tests are binary16 or float32 values, exact in both arithmetics, so every difference between the kernel
and this file is the kernel's fp32 rounding.  With u = 2^-24 (half an ulp of fp32, relative):

Cosine, per pixel.  a = sum o^2, b = sum t^2, d = sum o t: a sum of C products in any order carries at most (C - 1) u from
the additions and u from each product, so each of a, b, d is within C u of sum |terms| (second order dropped; the bounds
below carry spare units for it).  |d| <= sum |o t| <= sqrt(a b), so d's error is at most C u sqrt(a b).  cos = d / (sqrt a
sqrt b): the two roots, the product and the quotient add 4 u, the relative errors of a and b enter halved (C u / 2 each),
and |cos| <= 1:  |cos32 - cos64| <= C u + C u + 4 u,  and the subtraction from 1 adds u |l| <= 2 u:
    |l32 - l64| <= (2 C + 8) u.                                                                       (cosine_loss_bound)

L2, per pixel.  l = (sum (o - t)^2) / C: the difference is rounded once (relative u, entering squared: 2 u), the square
once (u), the sum of C non-negative terms in any order carries (C - 1) u, the division u: (C + 3) u l in first order.  The
bound is stated as (C + 4) u l for the sum and its spare unit plus one rounding for each of the difference, the square and
the scale, (C + 4) u l + 4 u l:
    |l32 - l64| <= (C + 8) u l64.                                                                     (l2_loss_bound)

Statistics.  loss_stats[0] sums the fp32 products m_p l_p in float64: each product adds u m_p l_p, the float64 sum nothing
that matters:  |stats0 - sum m_p l64_p| <= sum m_p (bound_p + u l64_p), within W H times the largest per-pixel term.
loss_stats[1] is a float64 sum of fp32 weights: exact to 1e-12 relative.

Gradient image.  G = (s m) (A t + B o).  A and B are quotients of a, b, d: their relative error is within (2 C + 8) u by
the argument above (L2: two roundings), the two products, the sum and the product with s m add 4 u, and s itself one or
two: with E = (2 C + 16) u |s| m (|A t| + |B o|),  |G32 - G64| <= E.  Scaling by 2^k is exact; the rounding to binary16 adds
2^-11 of the scaled value, or 2^-25 absolutely where it is subnormal:
    |Gq 2^-k - G64| <= 2^-11 (|G64| + E) + 2^-25 2^-k + E.                                            (gradient_bound)
"""
import numpy as np

U = 2.0 ** -24
KINDS = ("cosine", "l2")


def feature_loss64(image, target, weight=None, alpha=None, min_alpha=0.0, kind="cosine"):
    """image [H,W,C] (float16 or float32), target [H,W,C] float16, weight / alpha [H,W] float32 or None.  Returns a dict:
    valid bool [H,W]; m f64 [H,W] (0 where invalid); l f64 [H,W] (0 where invalid); pixel_loss = m l; stats = (sum m l,
    sum m); A, B f64 [H,W]; v = A t + B o f64 [H,W,C] (zeros where invalid); vmax = max_p m_p max_c |v|; o, t in float64 with
    the rows of invalid pixels zeroed."""
    assert kind in KINDS
    H, W, C = image.shape
    w = np.ones((H, W), np.float32) if weight is None else np.asarray(weight, np.float32)
    with np.errstate(invalid="ignore"):
        valid = w > 0                                            # false for 0, -0, negative and NaN
        if alpha is not None:
            valid &= np.asarray(alpha, np.float32) >= np.float32(min_alpha)
    o = np.where(valid[..., None], image, 0).astype(np.float64)  # rows of pixels already invalid are never read
    t = np.where(valid[..., None], target, 0).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        a, b, d = (o * o).sum(-1), (t * t).sum(-1), (o * t).sum(-1)
        if kind == "cosine":
            valid = valid & (a > 0) & (b > 0)                    # false for a NaN sum as well
    o = np.where(valid[..., None], o, 0.0)
    t = np.where(valid[..., None], t, 0.0)
    a, b, d = (o * o).sum(-1), (t * t).sum(-1), (o * t).sum(-1)
    m = np.where(valid, w.astype(np.float64), 0.0)
    if kind == "cosine":
        nn = np.where(valid, np.sqrt(a) * np.sqrt(b), 1.0)
        cs = d / nn
        l = np.where(valid, 1.0 - cs, 0.0)
        A = np.where(valid, -1.0 / nn, 0.0)
        B = np.where(valid, cs / np.where(valid, a, 1.0), 0.0)
    else:
        l = np.where(valid, ((o - t) ** 2).sum(-1) / C, 0.0)
        B = np.where(valid, 2.0 / C, 0.0)
        A = -B
    v = A[..., None] * t + B[..., None] * o
    pl = m * l
    return dict(valid=valid, m=m, l=l, pixel_loss=pl, stats=(float(pl.sum()), float(m.sum())), A=A, B=B, v=v, o=o, t=t,
                vmax=float((m * np.abs(v).max(-1)).max()), kind=kind, C=C)


def mean_loss(r):
    return r["stats"][0] / r["stats"][1] if r["stats"][1] > 0 else 0.0


def scalar(r, reduction, grad_loss=1.0):
    """s of the contract: grad_loss for "sum"; (float32)(grad_loss / sum m) for "mean", 0 when sum m = 0."""
    g = float(np.float32(grad_loss))
    if reduction == "sum":
        return g
    assert reduction == "mean"
    return float(np.float32(g / r["stats"][1])) if r["stats"][1] > 0 else 0.0


def exponent(x):
    """k = 14 - ceil(log2 x), at most 126; 0 for x = 0: quantize_gradient_map's rule, x the map's largest magnitude."""
    x = float(x)
    if not x > 0.0:
        return 0
    mant, ex = np.frexp(x)                                       # x = mant 2^ex, mant in [0.5, 1)
    return int(min(14 - (ex - 1 if mant == 0.5 else ex), 126))


def near_power_of_two(x, rel=1e-5):
    """Whether x lies within a relative `rel` of a power of two: there the fp32 maximum may fall on the other side."""
    if not x > 0.0:
        return False
    mant, _ = np.frexp(float(x))
    return mant <= 0.5 * (1 + rel) or mant >= 1 - rel


def gradient64(r, s):
    """G [H,W,C] = s m (A t + B o)."""
    return s * r["m"][..., None] * r["v"]


def dequantised(Gq, k):
    return np.asarray(Gq, np.float64) * 2.0 ** -int(k)


def cosine_loss_bound(C):
    return (2 * C + 8) * U


def l2_loss_bound(C, l64):
    return (C + 8) * U * l64


def loss_bound(r):
    return np.full(r["l"].shape, cosine_loss_bound(r["C"])) if r["kind"] == "cosine" else l2_loss_bound(r["C"], r["l"])


def stats_bound(r):
    return float((r["m"] * (loss_bound(r) + U * r["l"])).sum()) + 1e-12 * abs(r["stats"][0])


def gradient_bound(r, s, k):
    G = gradient64(r, s)
    E = (2 * r["C"] + 16) * U * abs(s) * r["m"][..., None] * (np.abs(r["A"][..., None] * r["t"]) + np.abs(r["B"][..., None] * r["o"]))
    return 2.0 ** -11 * (np.abs(G) + E) + 2.0 ** -25 * 2.0 ** -int(k) + E
