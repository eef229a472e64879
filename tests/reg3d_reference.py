"""The contract of vp_knn_points, vp_neighbor_kl and vp_neighbor_kl_gradient (include/voxproj.h) in float64 numpy, and the
bounds the GPU tests hold the fp32 kernels to.

``knn_brute``: every squared distance as the float64 sum of squares of float64-converted fp32 differences, the k smallest by
the key (d2, index), the query's own point left out; -1 / +inf where fewer than k other points exist.  The device must
return the same indices and the same float64 distances, bit for bit.

``statement64``: with p_i = softmax(z_i), eps = 1e-10, over sample positions s (row smp[s]) and their k - 1 table entries j
(-1 skipped):
    sample_loss[s] = sum_j sum_c p_sc (log(p_sc + eps) - log(p_jc + eps)),   sum = sum_s sample_loss[s],
    loss = scale / (S k P) sum  (0 when S = 0),     k counts the point itself (the reference's convention).
    g (gradient with respect to the probabilities, before the factor): a sample row receives log(p_s + eps) - log(p_j + eps) +
    p_s / (p_s + eps) per neighbour, a neighbour row - p_s / (p_j + eps) per sample position that lists it;
    grad = scale / (S k P) p (g - <g, p>).

Bounds (``bounds``).  The logits are float32 values, exact in both arithmetics, so every difference is fp32 rounding;
u = 2^-24.  First-order terms are written out below and the total is multiplied by 1.001 for the second-order ones (the
largest relative error below is about (2 P + 200) u < 5e-5, its square is far below 0.001 of it).
  expf and logf are taken to be within EXP_ULP = LOG_ULP = 2 ulp = 4 u (the ROCm device library documents 1 ulp for both;
  the other ulp is margin that was fixed before any kernel ran).
  row_lse = max + logf(sum_c expf(z_c - max)).  The maximum is exact.  x_c = max - z_c is rounded once, u x_c on the exponent of
    a term e^-x_c: relative to the sum that is u sum_c q_c x_c with q the softmax weights, and sum_c q_c x_c = H(q) - log sum
    <= log P <= P; expf 2 EXP_ULP u; the sum of P positive terms, in any association, at most P u: in all at most
    (2 P + 2 EXP_ULP) u relative on the sum, hence absolute on its logarithm; logf's own rounding 2 LOG_ULP u |log sum| with
    1 <= sum <= P; the addition of the maximum u |lse|:
        dl_i = (2 P + 2 EXP_ULP + 2 LOG_ULP log P + |lse_i|) u.
  p_c = expf(z_c - lse): the argument is off by dl_i and by its own rounding u |z_c - lse|, expf by 2 EXP_ULP u, and a result
    below the smallest normal float may be flushed or lose bits:
        dp = p (dl_i + u |z_c - lse_i| + 2 EXP_ULP u) + 2^-126.
  a = p + eps (eps itself rounded to fp32): da = dp + 2 u a.     lp = logf(a): dlp = da / a + 2 LOG_ULP u |lp|.
  Forward term t = p_s (lp_s - lp_j):  d = lp_s - lp_j, dd = dlp_s + dlp_j + u |d|,  dt = dp_s |d| + p_s dd + u |t|.
  A sum of fp32 terms along a tree of depth D is off by at most D u sum |terms|.  sample_loss adds, per lane, at most
    4 (k - 1) terms (four channels per lane at most) and then log2(64) = 6 butterfly steps:  D_f = 4 (k - 1) + 6.
        sample bound_s = sum_jc dt + D_f u sum_jc |t|.
  stats[0] adds the fp32 sample losses in float64:  sum_s bound_s + S 2^-53 sum_s |sample_loss|.  The loss is that times
    scale / (S k P), applied in float64 by the caller.
  Gradient.  r = p_i / a_i (IEEE division): dr = dp / a + r da / a + u r.
    as sample:      A = (lp_i - lp_j) + r_i,     dA = dd + dr + u |A|
    as neighbour:   B = - p_s / a_i,             dB = dp_s / a_i + |B| da_i / a_i + u |B|
    g_c adds its n_i contributions one after the other:  dg = sum dA + sum dB + n_i u sum |contributions|.
    dot = sum_c g_c p_c, per lane at most 4 terms, then 6 butterfly steps:
        ddot = sum_c (dg_c p_c + |g_c| dp_c + u |g_c p_c|) + 10 u sum_c |g_c p_c|.
    w = g - dot: dw = dg + ddot + u |w|.   The factor: scale / (S k P) rounded to fp32 (u), times grad_loss (u), p w rounded
    (u), the product (u):   dgrad = coef (dp |w| + p dw) + 4 u |grad|.
  Every factor above was fixed before the kernels ran against it.  Measured afterwards on the MI355X over
  tests/test_gpu_reg3d.py's cases, the worst element of any case as a fraction of its bound: row_lse 0.317, sample_loss 0.148,
  the sum 0.036, the gradient 0.074.
"""
import numpy as np

U = 2.0 ** -24
EXP_ULP = 2
LOG_ULP = 2
EPS = 1e-10
TINY = 2.0 ** -126
SECOND_ORDER = 1.001


def knn_brute(points, k, queries=None, self_index=None):
    """points f32 [N,3]; queries f32 [M,3] (None: the points, each left out of its own result); self_index [M] or None.
    Returns (idx int32 [M,k], d2 float64 [M,k])."""
    pts = np.asarray(points, np.float32).astype(np.float64)
    if queries is None:
        q = pts
        self_index = np.arange(len(pts))
    else:
        q = np.asarray(queries, np.float32).astype(np.float64)
    M, N = len(q), len(pts)
    idx = np.full((M, k), -1, np.int32)
    d2o = np.full((M, k), np.inf)
    ar = np.arange(N)
    for lo in range(0, M, 512):
        hi = min(M, lo + 512)
        d = q[lo:hi, None, :] - pts[None, :, :]
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        d2 = dx * dx + dy * dy + dz * dz                  # the device's association: (dx dx + dy dy) + dz dz
        if self_index is not None:
            si = np.asarray(self_index)[lo:hi]
            ok = (si >= 0) & (si < N)
            d2[np.flatnonzero(ok), si[ok]] = np.inf
        for r in range(hi - lo):
            order = np.lexsort((ar, d2[r]))[:k]
            order = order[np.isfinite(d2[r][order])]
            idx[lo + r, :len(order)] = order
            d2o[lo + r, :len(order)] = d2[r][order]
    return idx, d2o


def knn_mean_dist2(points):
    """float64 [N]: the mean of the (up to) three smallest squared distances to other points; 0 for a lone point."""
    _, d2 = knn_brute(points, 3)
    have = np.isfinite(d2)
    z = np.where(have, d2, 0.0)
    return ((z[:, 0] + z[:, 1]) + z[:, 2]) / np.maximum(have.sum(1), 1)


def reverse_table_loop(nbr, n_rows):
    """The reversed table by a Python loop: (rev_start [n_rows+1], the valid part of rev_entry)."""
    lists = [[] for _ in range(n_rows)]
    for e, v in enumerate(np.asarray(nbr).reshape(-1).tolist()):
        if 0 <= v < n_rows:
            lists[v].append(e)
    start = np.zeros(n_rows + 1, np.int64)
    start[1:] = np.cumsum([len(x) for x in lists])
    return start, np.array([e for x in lists for e in x], np.int64)


def _softmax64(z):
    z = np.asarray(z, np.float64)
    m = z.max(1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(1, keepdims=True)
    return e / s, (m + np.log(s))[:, 0]


def _rows(N, samples):
    return np.arange(N) if samples is None else np.asarray(samples, np.int64).reshape(-1)


def statement64(logits, samples, nbr, k, scale=2.0, grad_loss=1.0):
    """logits f32 [N,P]; samples int [S] or None (every row); nbr int [S,k-1].  Returns a dict: loss, sum, sample_loss [S],
    row_lse [N], grad [N,P] (all float64), S."""
    z = np.asarray(logits, np.float32).astype(np.float64)
    N, P = z.shape
    smp = _rows(N, samples)
    S = len(smp)
    nbr = np.asarray(nbr, np.int64).reshape(S, k - 1)
    p, lse = _softmax64(z)
    lp = np.log(p + EPS)
    g = np.zeros((N, P))
    sample_loss = np.zeros(S)
    for s in range(S):
        i = smp[s]
        for j in nbr[s]:
            if j < 0 or j >= N:
                continue
            sample_loss[s] += (p[i] * (lp[i] - lp[j])).sum()
            g[i] += lp[i] - lp[j] + p[i] / (p[i] + EPS)
            g[j] -= p[i] / (p[j] + EPS)
    total = float(sample_loss.sum())
    coef = scale / (S * k * P) if S else 0.0
    grad = coef * grad_loss * p * (g - (g * p).sum(1, keepdims=True))
    return dict(loss=coef * total, sum=total, sample_loss=sample_loss, row_lse=lse, grad=grad, S=S, coef=coef)


def bounds(logits, samples, nbr, k, scale=2.0, grad_loss=1.0):
    """The bounds of the module's docstring: a dict with row_lse [N], sample_loss [S], sum, loss (floats), grad [N,P]."""
    z = np.asarray(logits, np.float32).astype(np.float64)
    N, P = z.shape
    smp = _rows(N, samples)
    S = len(smp)
    nbr = np.asarray(nbr, np.int64).reshape(S, k - 1)
    p, lse = _softmax64(z)
    dl = (2 * P + 2 * EXP_ULP + 2 * LOG_ULP * np.log(P) + np.abs(lse)) * U
    dp = p * (dl[:, None] + U * np.abs(z - lse[:, None]) + 2 * EXP_ULP * U) + TINY
    a = p + EPS
    da = dp + 2 * U * a
    lp = np.log(a)
    dlp = da / a + 2 * LOG_ULP * U * np.abs(lp)
    r = p / a
    dr = dp / a + r * da / a + U * r
    Df = 4 * (k - 1) + 6
    sb = np.zeros(S)
    sabs = np.zeros(S)
    sl = np.zeros(S)
    g = np.zeros((N, P))
    dg = np.zeros((N, P))          # sum of the contributions' own errors
    gabs = np.zeros((N, P))        # sum of |contributions|
    cnt = np.zeros(N)
    for s in range(S):
        i = smp[s]
        for j in nbr[s]:
            if j < 0 or j >= N:
                continue
            d = lp[i] - lp[j]
            dd = dlp[i] + dlp[j] + U * np.abs(d)
            t = p[i] * d
            sb[s] += (dp[i] * np.abs(d) + p[i] * dd + U * np.abs(t)).sum()
            sabs[s] += np.abs(t).sum()
            sl[s] += t.sum()
            A = d + r[i]
            g[i] += A
            dg[i] += dd + dr[i] + U * np.abs(A)
            gabs[i] += np.abs(A)
            cnt[i] += 1
            B = p[i] / a[j]
            g[j] -= B
            dg[j] += dp[i] / a[j] + B * da[j] / a[j] + U * B
            gabs[j] += B
            cnt[j] += 1
    sample_bound = sb + Df * U * sabs
    sum_bound = float(sample_bound.sum() + S * 2.0 ** -53 * np.abs(sl).sum())
    coef = scale / (S * k * P) if S else 0.0
    dg = dg + cnt[:, None] * U * gabs
    gp = np.abs(g * p)
    ddot = (dg * p + np.abs(g) * dp + U * gp).sum(1) + 10 * U * gp.sum(1)
    w = g - (g * p).sum(1, keepdims=True)
    dw = dg + ddot[:, None] + U * np.abs(w)
    c = abs(coef * grad_loss)
    grad_bound = c * (dp * np.abs(w) + p * dw) + 4 * U * np.abs(c * p * w)
    k2 = SECOND_ORDER
    return dict(row_lse=k2 * dl, sample_loss=k2 * sample_bound, sum=k2 * sum_bound, loss=k2 * abs(coef) * sum_bound,
                grad=k2 * grad_bound)


def torch_composite(logits, samples, nbr, k, scale=2.0):
    """The same loss written with torch ops (log_softmax, row gather, KL) for autograd and central differences on the CPU:
    float64 logits tensor [N,P] -> scalar tensor."""
    import torch
    N, P = logits.shape
    smp = torch.arange(N) if samples is None else torch.as_tensor(np.asarray(samples, np.int64))
    S = len(smp)
    if S == 0:
        return logits.sum() * 0.0
    nb = torch.as_tensor(np.asarray(nbr, np.int64)).reshape(S, k - 1)
    ok = ((nb >= 0) & (nb < N)).to(logits.dtype)
    p = torch.softmax(logits, 1)
    lp = torch.log(p + EPS)
    ps, lps = p[smp][:, None, :], lp[smp][:, None, :]
    kl = (ps * (lps - lp[nb.clamp(0, N - 1)])).sum(-1) * ok
    return scale / (S * k * P) * kl.sum()


# ------------------------------------------------------------------------------------------------
# Point sets and logits of the GPU tests
# ------------------------------------------------------------------------------------------------
def jittered_lattice(n, seed, cell=0.07, jitter=0.35):
    g = np.random.default_rng(seed)
    ax = np.arange(n) * cell
    base = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    return (base + g.uniform(-jitter, jitter, base.shape) * cell).astype(np.float32)


def smooth_logits(points, P, seed, amp=3.0, noise=0.5):
    """Logits that vary smoothly in space plus noise: neighbours resemble each other, as after some training."""
    g = np.random.default_rng(seed)
    W = g.normal(size=(3, P)) * amp / max(float(np.abs(points).max()), 1e-6)
    return (np.asarray(points, np.float64) @ W + noise * g.normal(size=(len(points), P))).astype(np.float32)
