"""The photometric loss (L1 + D-SSIM) of include/voxproj.h in float64, and derived error bounds for an fp32 evaluation of it.

statement64(image, target) is the contract written out in numpy float64, nothing shared with the library: the 121-tap window
applied tap by tap with zero padding, the five window sums, m and the three maps P, Q, R, the three statistics and, for a
lambda and an upstream scalar s, the gradient image

    grad = s ((1 - lambda) / n sgn(x - y) - lambda / n ((w * P) + 2 x (w * Q) + y (w * R))).

The window is the outer product of ROW, the eleven fp32 numbers of the header.  ``window2d`` replaces it: the recorded
results of tests/golden/photo_loss_golden.npz come from a window whose 121 weights are those products rounded to fp32 once
more, and test_photo_loss_cpu.py passes that window to compare at 1e-12.

bounds(image, target) traces the fp32 evaluation operation by operation with a running error: every quantity is a pair
(value in float64, bound on |fp32 result - value|), and every operation adds the propagated input errors (with the
denominator of a quotient taken at its smallest, |b| - E_b) plus one rounding, u = 2^-24, of the largest result the bound
admits.  That is rigorous for the traced order, not a first-order estimate.  The trace:

  * a window sum is 11 products and 10 additions along a row, then 11 products and 10 additions down a column, of terms that
    for x^2, y^2, x y carry one rounding of their own: at most K_SUM = 24 roundings per term, so the sum is off by at most
    gamma_24 sum w |term|, gamma_k = k u / (1 - k u).  The terms are non-negative in e11 and e22, where the bound is a
    relative one; it is the later e - mu^2 beside C2 = 9e-4 that turns it into a large relative error of s1 + s2 on a smooth
    image.  (An fp32 window whose weights are rounded products has one more rounding per term: still within 24.)
  * C1 and C2 are fp32 constants: each is off by at most u of itself.
  * mu1^2, mu2^2, mu1 mu2; s1, s2, s12; A1, A2, B1, B2; D = B1 B2; m = A1 A2 / D; R = 2 A1 / D; Q = -(m / B2);
    P = mu2 (2 A2 / D - R) - 2 mu1 (m / B1 + Q).  B1 >= C1 and B2 >= C2 - E(s1 + s2) bound the denominators from below.
  * the gradient: three more window sums, now of maps that carry the errors above -- sum w E_map (1 + gamma) + gamma sum w |map|
    each, 33 terms in all -- combined with the exact x and y, the fp32 a = (1 - lambda) / n and b = lambda / n, and s.
  * the statistics: the fp32 terms |x - y| (one rounding), (x - y)^2 (two and the doubling) and m, added in float64; the
    float64 additions contribute n 2^-53 of the sum of magnitudes, which is added.

SAFETY = 2 is the one safety factor, applied once to every bound handed out.  It pays for evaluations that reach the same
quantities by other routes than the traced one -- m^2 formed before a division instead of after, a product associated the
other way, an autograd chain that forms dm/dmu1 from four terms instead of two -- whose rounding counts per quantity differ
from the trace's by less than a factor of two.  No bound is floored or fitted to any output.
"""
import hashlib

import numpy as np

U = 2.0 ** -24
K_SUM = 24
SAFETY = 2.0
RADIUS = 5
C1, C2 = 0.01 ** 2, 0.03 ** 2
ROW = np.array([float.fromhex(h) for h in (
    "0x1.0d956cp-10", "0x1.f1fe02p-8", "0x1.26eb18p-5", "0x1.bff0fep-4", "0x1.b43c3ep-3", "0x1.10656p-2",
    "0x1.b43c3ep-3", "0x1.bff0fep-4", "0x1.26eb18p-5", "0x1.f1fe02p-8", "0x1.0d956cp-10")], np.float64)
TILE = 32                                                  # the kernel's tile: the tests choose their shapes round it


def gamma(k):
    return k * U / (1.0 - k * U)


_SUMS = {}                                                 # window_sum's results by the digest of the input (see there)
_SUMS_LIMIT = 256 << 20                                    # bytes of results kept
_STRIP = 64                                                # rows summed at a time: one strip and its taps stay in cache


def window_sum(a, window2d=None):
    """sum over the window of w a with zero padding, per plane of a [C,H,W], tap by tap in float64 (every element adds its
    121 products in the order i, j whatever the strips are).  With the contract's window the result is remembered under a
    128-bit digest of the input and handed out read-only: statement64() and bounds() of one pair of images form eight of their
    27 sums twice, and at a million elements a sum takes a fifth of a second."""
    w = np.outer(ROW, ROW) if window2d is None else np.asarray(window2d, np.float64)
    a = np.ascontiguousarray(a, np.float64)
    key = None
    if window2d is None:
        key = (a.shape, hashlib.blake2b(a, digest_size=16).digest())
        if key in _SUMS:
            return _SUMS[key]
    C, H, W = a.shape
    pad = np.zeros((C, H + 2 * RADIUS, W + 2 * RADIUS), np.float64)
    pad[:, RADIUS:RADIUS + H, RADIUS:RADIUS + W] = a
    out = np.zeros_like(a)
    tmp = np.empty((min(_STRIP, H), W), np.float64)
    for c in range(C):
        for r0 in range(0, H, _STRIP):
            h = min(_STRIP, H - r0)
            o, t = out[c, r0:r0 + h], tmp[:h]
            for i in range(2 * RADIUS + 1):
                for j in range(2 * RADIUS + 1):
                    np.multiply(pad[c, r0 + i:r0 + i + h, j:j + W], w[i, j], out=t)
                    o += t
    if key is not None:
        if sum(v.nbytes for v in _SUMS.values()) + out.nbytes > _SUMS_LIMIT:
            _SUMS.clear()
        out.flags.writeable = False
        _SUMS[key] = out
    return out


def statement64(image, target, *, lambda_dssim=None, grad_loss=1.0, window2d=None):
    """The contract in float64.  image, target [C,H,W].  Returns stats [3], m, P, Q, R, the loss and (with lambda_dssim) grad."""
    x, y = np.asarray(image, np.float64), np.asarray(target, np.float64)
    assert x.ndim == 3 and x.shape == y.shape
    n = x.size
    mu1, mu2 = window_sum(x, window2d), window_sum(y, window2d)
    e11, e22, e12 = window_sum(x * x, window2d), window_sum(y * y, window2d), window_sum(x * y, window2d)
    s1, s2, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
    A1, A2 = 2 * mu1 * mu2 + C1, 2 * s12 + C2
    B1, B2 = mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
    m = A1 * A2 / (B1 * B2)
    Q = -A1 * A2 / (B1 * B2 * B2)
    R = 2 * A1 / (B1 * B2)
    P = 2 * mu2 * A2 / (B1 * B2) - 2 * mu1 * A1 * A2 / (B1 * B1 * B2) - 2 * mu1 * Q - mu2 * R
    d = x - y
    stats = np.array([np.abs(d).sum(), (d * d).sum(), m.sum()])
    out = dict(stats=stats, m=m, P=P, Q=Q, R=R, n=n)
    if lambda_dssim is not None:
        lam = float(lambda_dssim)
        dm = window_sum(P, window2d) + 2 * x * window_sum(Q, window2d) + y * window_sum(R, window2d)
        out["dm"] = dm
        out["grad"] = float(grad_loss) * ((1 - lam) / n * np.sign(d) - lam / n * dm)
        out["loss"] = (1 - lam) * stats[0] / n + lam * (1 - stats[2] / n)
    return out


class V:
    """A float64 value with a bound on the distance of its fp32 evaluation from it."""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape)

    @staticmethod
    def _r(v, e):                                          # one rounding of a result that lies within e of v
        return V(v, e + U * (np.abs(v) + e))

    def __add__(self, o):
        return V._r(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        return V._r(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        return V._r(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __truediv__(self, o):
        lo = np.abs(o.v) - o.e
        assert (lo > 0).all(), "a denominator's bound reaches zero"
        q = self.v / o.v
        return V._r(q, (self.e + np.abs(q) * o.e) / lo)

    def twice(self):                                       # exact in binary
        return V(2 * self.v, 2 * self.e)

    def neg(self):
        return V(-self.v, self.e)


def _vsum(term, mag):
    """The fp32 window sum of exact-valued terms: value, gamma_24 sum w |term|."""
    return V(window_sum(term), gamma(K_SUM) * window_sum(mag))


def _vsum_of(q):
    """The fp32 window sum of a map that carries an error of its own."""
    return V(window_sum(q.v), (1 + gamma(K_SUM)) * window_sum(q.e) + gamma(K_SUM) * window_sum(np.abs(q.v)))


def bounds(image, target, *, lambda_dssim=None, grad_loss=1.0):
    """Per-element bounds on |fp32 evaluation - statement64| for m, P, Q, R, the three statistics and (with lambda_dssim)
    the gradient image; SAFETY applied."""
    x, y = np.asarray(image, np.float64), np.asarray(target, np.float64)
    n = x.size
    mu1, mu2 = _vsum(x, np.abs(x)), _vsum(y, np.abs(y))
    e11, e22, e12 = _vsum(x * x, x * x), _vsum(y * y, y * y), _vsum(x * y, np.abs(x * y))
    c1, c2 = V(np.full(x.shape, C1), U * C1), V(np.full(x.shape, C2), U * C2)
    mu11, mu22, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = e11 - mu11, e22 - mu22, e12 - mu12
    A1, A2 = mu12.twice() + c1, s12.twice() + c2
    B1, B2 = (mu11 + mu22) + c1, (s1 + s2) + c2
    D = B1 * B2
    m = (A1 * A2) / D
    R = A1.twice() / D
    Q = (m / B2).neg()
    P = mu2 * (A2.twice() / D - R) - mu1.twice() * (m / B1 + Q)
    d = x - y
    l1 = V(np.abs(d), U * np.abs(d))
    dd = V(d, U * np.abs(d))
    l2 = dd * dd
    f64 = n * 2.0 ** -53
    stats = np.array([l1.e.sum() + f64 * np.abs(l1.v).sum(), l2.e.sum() + f64 * l2.v.sum(),
                      m.e.sum() + f64 * np.abs(m.v).sum()])
    out = dict(m=SAFETY * m.e, P=SAFETY * P.e, Q=SAFETY * Q.e, R=SAFETY * R.e, stats=SAFETY * stats)
    if lambda_dssim is not None:
        lam = float(lambda_dssim)
        a, b = (1 - lam) / n, lam / n
        va, vb = V(np.full(x.shape, a), U * abs(a)), V(np.full(x.shape, b), U * abs(b))
        dm = (_vsum_of(P) + V(x).twice() * _vsum_of(Q)) + V(y) * _vsum_of(R)
        g = V(np.full(x.shape, float(grad_loss))) * (va * V(np.sign(d)) - vb * dm)
        out["grad"] = SAFETY * g.e
    return out


def make_inputs(kind, C, W, H, seed):
    """The seeded inputs of the tests, f32 [C,H,W] in [0, 1]:
    noise: uniform noise against noise.   flat: 0.5 + 1e-3 noise against the constant 0.5.
    smooth: sinusoids plus 0.03 noise, two of them.   binary: independent 0 / 1 images (m goes negative).   equal: x = y."""
    g = np.random.default_rng(seed)
    shape = (C, H, W)
    if kind == "noise":
        x, y = g.uniform(0, 1, shape), g.uniform(0, 1, shape)
    elif kind == "flat":
        x, y = 0.5 + 1e-3 * g.uniform(-1, 1, shape), np.full(shape, 0.5)
    elif kind == "smooth":
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        base = np.stack([0.5 + 0.35 * np.sin(0.11 * xx + 0.7 * c) * np.cos(0.07 * yy - 0.3 * c) for c in range(C)])
        x = np.clip(base + 0.03 * g.normal(size=shape), 0, 1)
        y = np.clip(base + 0.03 * g.normal(size=shape), 0, 1)
    elif kind == "binary":
        x, y = g.integers(0, 2, shape).astype(np.float64), g.integers(0, 2, shape).astype(np.float64)
    else:
        assert kind == "equal"
        x = g.uniform(0, 1, shape)
        y = x
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)


KINDS = ("noise", "flat", "smooth", "binary", "equal")
# W x H of the GPU test: one pixel, smaller than the window, the window, the tile and one column more, odd, many tiles
SIZES = ((1, 1), (5, 7), (11, 11), (TILE, TILE), (TILE + 1, TILE), (37, 21), (130, 67))
CHANNELS = (1, 3, 4)


def gpu_cases():
    """(kind, C, W, H, seed) of every input the GPU test runs: every size at C = 3 with every kind, and C = 1 and 4 with noise
    and smooth at the sizes that have more than one tile."""
    cases = []
    for i, (W, H) in enumerate(SIZES):
        for j, kind in enumerate(KINDS):
            cases.append((kind, 3, W, H, 100 + 10 * i + j))
    for C in (1, 4):
        for i, (W, H) in enumerate(((1, 1), (TILE + 1, TILE), (37, 21), (130, 67))):
            for j, kind in enumerate(("noise", "smooth")):
                cases.append((kind, C, W, H, 300 + 40 * C + 10 * i + j))
    return cases
