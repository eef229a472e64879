"""The view-dependent colour of include/voxproj_ext.h (spherical harmonics of degree 0 .. 3) in float64 NumPy, its adjoints,
and derived error bounds for an fp32 evaluation of both.

Statement (sh[0] = f_dc, sh[k] = f_rest[k - 1], active degree d, K = (d + 1)^2):
    p = mean - campos;  r = |p|;  (x, y, z) = p / r, (0, 0, 0) when r == 0
    pre[c] = sum_{k < K} Y_k(x, y, z) sh[k][c] + 0.5;   colour[c] = max(pre[c], 0);   bit c of clamped = pre[c] < 0
    g[c] = clamped bit c ? 0 : grad_colors[c]
    grad_sh[k][c] = Y_k g[c] (zeros for k >= K);  v_k = sum_c sh[k][c] g[c];  q = sum_k v_k grad Y_k
    grad_mean = (q - dir (dir . q)) / r, 0 when r == 0

The polynomials Y_k and their gradients are written ONCE (basis, basis_adjoint), over any number type with + - * : float64
arrays give the statement, V pairs give the bounds.

bounds(...) traces an fp32 evaluation operation by operation with a running error, as tests/photo_loss_reference.py does: a
V is (value in float64, bound on |fp32 result - value|); every operation adds the propagated input errors (a quotient's or
square root's denominator taken at its smallest) plus one rounding, u = 2^-24, of the largest result the bound allows.
Constants carry the rounding of their fp32 literal; small integers and 0.5 are exact.  The inputs (fp32 arrays, the fp32
camera centre) are exact.  SAFETY = 2 is the one safety factor, applied once to every bound handed out: it pays for
evaluations that associate the same sums differently from the trace.  No bound is floored or fitted to any output.
"""
import numpy as np

U = 2.0 ** -24
SAFETY = 2.0
MAX_DEGREE = 3

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435)


def n_coeffs(degree):
    return (degree + 1) ** 2


def rest_width(max_degree):
    return n_coeffs(max_degree) - 1


def camera_position(viewmat):
    """-R^T t of a [4,4] world-to-camera matrix in float64, then rounded to fp32 as the library receives it."""
    vm = np.asarray(viewmat, np.float64).reshape(4, 4)
    return (-(vm[:3, :3].T @ vm[:3, 3])).astype(np.float32).astype(np.float64)


def basis(x, y, z, degree, const=float):
    """[Y_0 .. Y_{K-1}] at (x, y, z); Y_0 is the constant itself (not an array)."""
    Y = [const(C0)]
    if degree > 0:
        Y += [const(-C1) * y, const(C1) * z, const(-C1) * x]
    if degree > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        Y += [const(C2[0]) * xy, const(C2[1]) * yz, const(C2[2]) * ((2.0 * zz - xx) - yy), const(C2[3]) * xz,
              const(C2[4]) * (xx - yy)]
    if degree > 2:
        Y += [(const(C3[0]) * y) * (3.0 * xx - yy), (const(C3[1]) * xy) * z, (const(C3[2]) * y) * ((4.0 * zz - xx) - yy),
              (const(C3[3]) * z) * ((2.0 * zz - 3.0 * xx) - 3.0 * yy), (const(C3[4]) * x) * ((4.0 * zz - xx) - yy),
              (const(C3[5]) * z) * (xx - yy), (const(C3[6]) * x) * (xx - 3.0 * yy)]
    return Y


def basis_adjoint(x, y, z, v, degree, zero, const=float):
    """q = sum_{k >= 1} v[k] grad Y_k(x, y, z) as (qx, qy, qz); v[0] is not used (Y_0 is a constant)."""
    qx = qy = qz = zero
    if degree > 0:
        qy, qz, qx = const(-C1) * v[1], const(C1) * v[2], const(-C1) * v[3]
    if degree > 1:
        a4, a5, a6, a7, a8 = (const(C2[i]) * v[4 + i] for i in range(5))
        qx, qy = qx + a4 * y, qy + a4 * x
        qy, qz = qy + a5 * z, qz + a5 * y
        qx, qy, qz = qx + a6 * (-2.0 * x), qy + a6 * (-2.0 * y), qz + a6 * (4.0 * z)
        qx, qz = qx + a7 * z, qz + a7 * x
        qx, qy = qx + a8 * (2.0 * x), qy + a8 * (-2.0 * y)
    if degree > 2:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        a9, a10, a11, a12, a13, a14, a15 = (const(C3[i]) * v[9 + i] for i in range(7))
        qx, qy = qx + a9 * (6.0 * xy), qy + a9 * (3.0 * xx - 3.0 * yy)
        qx, qy, qz = qx + a10 * yz, qy + a10 * xz, qz + a10 * xy
        qx, qy, qz = qx + a11 * (-2.0 * xy), qy + a11 * ((4.0 * zz - xx) - 3.0 * yy), qz + a11 * (8.0 * yz)
        qx, qy, qz = qx + a12 * (-6.0 * xz), qy + a12 * (-6.0 * yz), qz + a12 * ((6.0 * zz - 3.0 * xx) - 3.0 * yy)
        qx, qy, qz = qx + a13 * ((4.0 * zz - 3.0 * xx) - yy), qy + a13 * (-2.0 * xy), qz + a13 * (8.0 * xz)
        qx, qy, qz = qx + a14 * (2.0 * xz), qy + a14 * (-2.0 * yz), qz + a14 * (xx - yy)
        qx, qy = qx + a15 * (3.0 * xx - 3.0 * yy), qy + a15 * (-6.0 * xy)
    return qx, qy, qz


def _inputs(f_dc, f_rest, means, campos, degree):
    f_dc, f_rest, means = (np.asarray(a, np.float64) for a in (f_dc, f_rest, means))
    campos = np.asarray(campos, np.float64).reshape(3)
    n = f_dc.shape[0]
    assert f_dc.shape == (n, 3) and means.shape == (n, 3) and f_rest.ndim == 3 and f_rest.shape[0] == n and f_rest.shape[2] == 3
    widths = {rest_width(D): D for D in range(MAX_DEGREE + 1)}
    assert f_rest.shape[1] in widths, f_rest.shape
    assert 0 <= degree <= widths[f_rest.shape[1]], (degree, f_rest.shape)
    return f_dc, f_rest, means, campos, n


def direction(means, campos):
    """(dir [N,3], r [N]): the unit view directions, zero rows where the mean is the camera centre."""
    p = means - campos
    r = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
    safe = np.where(r > 0, r, 1.0)
    return np.where((r > 0)[:, None], p / safe[:, None], 0.0), r


def _coeff(f_dc, f_rest, k):
    return f_dc if k == 0 else f_rest[:, k - 1]


def forward(f_dc, f_rest, means, campos, degree):
    """{"pre", "colors" [N,3], "clamped" u8 [N], "dir" [N,3], "r" [N]} in float64."""
    f_dc, f_rest, means, campos, n = _inputs(f_dc, f_rest, means, campos, degree)
    d, r = direction(means, campos)
    Y = basis(d[:, 0], d[:, 1], d[:, 2], degree)
    acc = np.zeros((n, 3))
    for k in range(n_coeffs(degree)):
        acc = acc + np.reshape(Y[k], (-1, 1)) * _coeff(f_dc, f_rest, k)
    pre = acc + 0.5
    neg = pre < 0
    return {"pre": pre, "colors": np.maximum(pre, 0.0), "dir": d, "r": r,
            "clamped": (neg[:, 0] * 1 + neg[:, 1] * 2 + neg[:, 2] * 4).astype(np.uint8)}


def mask_bits(clamped):
    """u8 [N] -> bool [N,3], True where the channel was clamped."""
    c = np.asarray(clamped).astype(np.int64)
    return np.stack([(c >> j) & 1 for j in range(3)], axis=1).astype(bool)


def backward(f_dc, f_rest, means, campos, degree, grad_colors, clamped=None):
    """{"grad_dc" [N,3], "grad_rest" [N,Kr,3] (zeros beyond the active degree), "grad_means" [N,3]} in float64; ``clamped``
    defaults to the statement's own mask."""
    f_dc, f_rest, means, campos, n = _inputs(f_dc, f_rest, means, campos, degree)
    if clamped is None:
        clamped = forward(f_dc, f_rest, means, campos, degree)["clamped"]
    g = np.where(mask_bits(clamped), 0.0, np.asarray(grad_colors, np.float64))
    d, r = direction(means, campos)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    Y = basis(x, y, z, degree)
    K = n_coeffs(degree)
    grad_rest = np.zeros_like(f_rest)
    for k in range(1, K):
        grad_rest[:, k - 1] = Y[k][:, None] * g
    v = [None] + [(f_rest[:, k - 1, 0] * g[:, 0] + f_rest[:, k - 1, 1] * g[:, 1]) + f_rest[:, k - 1, 2] * g[:, 2]
                  for k in range(1, K)]
    q = np.stack(basis_adjoint(x, y, z, v, degree, np.zeros(n)), axis=1)
    dq = (d * q).sum(1, keepdims=True)
    safe = np.where(r > 0, r, 1.0)[:, None]
    grad_means = np.where((r > 0)[:, None], (q - d * dq) / safe, 0.0)
    return {"grad_dc": C0 * g, "grad_rest": grad_rest, "grad_means": grad_means}


class V:
    """A float64 value with a bound on the distance of its fp32 evaluation from it."""

    __array_priority__ = 100.0                     # ndarray op V defers to V's reflected method

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape)

    @staticmethod
    def const(c):                                  # an fp32 literal of a float64 constant
        return V(c, abs(float(np.float32(c)) - c))

    @staticmethod
    def of(o):                                     # exact operands: input arrays, small integers
        return o if isinstance(o, V) else V(o, 0.0)

    @staticmethod
    def _r(v, e):                                  # one rounding of a result that lies within e of v
        return V(v, e + U * (np.abs(v) + e))

    def __add__(self, o):
        o = V.of(o)
        return V._r(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o)
        return V._r(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return V.of(o) - self

    def __mul__(self, o):
        o = V.of(o)
        return V._r(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o)
        lo = np.abs(o.v) - o.e
        assert (lo > 0).all(), "a denominator's bound reaches zero"
        q = self.v / o.v
        return V._r(q, (self.e + np.abs(q) * o.e) / lo)

    def sqrt(self):
        lo = self.v - self.e
        assert (lo > 0).all(), "a square root's argument may reach zero"
        return V._r(np.sqrt(self.v), self.e / (np.sqrt(self.v) + np.sqrt(lo)))

    def where(self, cond, other=0.0):              # exact `other` where cond is False
        return V(np.where(cond, self.v, other), np.where(cond, self.e, 0.0))


def _traced_direction(means, campos):
    p = [V(means[:, j]) - V(np.full(means.shape[0], campos[j])) for j in range(3)]
    r2 = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]
    ok = r2.v > 0
    r = V(np.where(ok, r2.v, 1.0), np.where(ok, r2.e, 0.0)).sqrt()       # p == 0 exactly in fp32 too: the subtraction is exact there
    return [(c / r).where(ok) for c in p], r, ok


def bounds(f_dc, f_rest, means, campos, degree, grad_colors=None, clamped=None):
    """Bounds on |fp32 evaluation - statement| (SAFETY applied): "pre" (also the colours': max(., 0) does not stretch an
    error) and, with grad_colors, "grad_dc", "grad_rest" and "grad_means", for the gradient mask ``clamped`` (default: the
    statement's).  A mask bit that differs between the two evaluations is not an error these bounds cover: the caller sets
    aside the channels with |pre| below the bound."""
    f_dc, f_rest, means, campos, n = _inputs(f_dc, f_rest, means, campos, degree)
    (x, y, z), r, ok = _traced_direction(means, campos)
    Y = basis(x, y, z, degree, V.const)
    K = n_coeffs(degree)
    pre_e = np.zeros((n, 3))
    for c in range(3):
        acc = Y[0] * V(f_dc[:, c])
        for k in range(1, K):
            acc = acc + Y[k] * V(f_rest[:, k - 1, c])
        pre_e[:, c] = (acc + 0.5).e
    out = {"pre": SAFETY * pre_e, "colors": SAFETY * pre_e}
    if grad_colors is None:
        return out
    if clamped is None:
        clamped = forward(f_dc, f_rest, means, campos, degree)["clamped"]
    g = np.where(mask_bits(clamped), 0.0, np.asarray(grad_colors, np.float64))
    gd, gr = np.zeros((n, 3)), np.zeros_like(f_rest)
    for c in range(3):
        gd[:, c] = (Y[0] * V(g[:, c])).e
        for k in range(1, K):
            gr[:, k - 1, c] = (Y[k] * V(g[:, c])).e
    v = [None] + [(V(f_rest[:, k - 1, 0]) * V(g[:, 0]) + V(f_rest[:, k - 1, 1]) * V(g[:, 1])) + V(f_rest[:, k - 1, 2]) * V(g[:, 2])
                  for k in range(1, K)]
    q = basis_adjoint(x, y, z, v, degree, V(np.zeros(n)), V.const)
    dq = (x * q[0] + y * q[1]) + z * q[2]
    gm = np.stack([((qc - dc * dq) / r).where(ok).e for qc, dc in zip(q, (x, y, z))], axis=1)
    out.update({"grad_dc": SAFETY * gd, "grad_rest": SAFETY * gr, "grad_means": SAFETY * gm})
    return out


def make_inputs(n, max_degree, seed, campos=(0.3, -0.2, 0.1)):
    """The GPU tests' inputs as fp32 arrays: f_dc ~ N(0,1), f_rest ~ N(0,0.4), means uniform in [-2,2]^3, the fp32 camera
    centre, and an upstream gradient ~ N(0,1)."""
    rng = np.random.default_rng(seed)
    return {"f_dc": rng.normal(0, 1, (n, 3)).astype(np.float32),
            "f_rest": rng.normal(0, 0.4, (n, rest_width(max_degree), 3)).astype(np.float32),
            "means": rng.uniform(-2, 2, (n, 3)).astype(np.float32),
            "campos": np.asarray(campos, np.float32),
            "grad_colors": rng.normal(0, 1, (n, 3)).astype(np.float32)}
