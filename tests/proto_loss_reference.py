"""The contract of vp_proto_contrast and vp_proto_contrast_gradient (include/voxproj.h) in float64, and the bounds the GPU
tests hold the fp32 kernels to.

``statement64`` is the loss as per-id loops in torch float64 (boolean indexing per id, the mean and the spread of each
cluster, the softmax of every sample against all prototypes), with pixel p counted count[p] times; ``want_grad`` adds its
gradient image by torch autograd on the CPU, through the prototypes, with the divisor r + 1e-6 and the temperatures
detached.  ``closed_form`` is include/voxproj.h's closed form in numpy for any dtype: in float64 it is checked against
autograd (tests/test_proto_loss_cpu.py), in float32 with the pixels visited in another order it is the yardstick below.

Bounds.  The inputs are float32 values, exact in both arithmetics, so every difference is fp32 rounding; u = 2^-24.

  stats[1] = K and stats[3] = sum m are integers: exact.
  stats[2] = sum (r - 1)^2: r = sqrt(sum f^2) carries (D / 2 + 1) u relative (D products and D - 1 additions of non-negative
    terms, halved by the root, and the root), so e = r - 1 is off by (D / 2 + 1) u r + u |e| and e^2 by
    2 |e| ((D / 2 + 1) u r + u |e|) + u e^2; the float64 sum adds nothing that matters:
        |stats2 - sum e^2| <= sum_p (2 |e| (D / 2 + 1) r + 3 e^2) u + 1e-12 sum e^2.                       (norm_bound)
  Everything else hangs on the prototypes u_k, sums of up to W H terms whose worst-case bound (n_k u) says nothing useful.
  The yardstick for what depends on those sums is the error of the SAME statement evaluated in float32 by numpy in other
  summation orders, against float64: ``closed_form`` with the pixels visited in descending order and in three seeded
  permutations (numpy's pairwise sums), the largest error over the four.  The device may be off by 8 times that, because the
  orders legitimately differ.  Only where a yardstick is exactly 0 (one pixel, K = 0) is it replaced by one rounding of
  the largest value, u max |.|; a non-zero yardstick is never raised.

  Forward outputs: derived from the yardstick of the exponents, E_z = max |z32 - z64| over pixels, ids and orders (z = s . u /
  phi carries the prototypes and the temperatures), with dz = 8 E_z allowed to the device.  log-sum-exp moves by at most
  max_k |dz_k| when its arguments move, and z_c by dz, so l = log(sum_k e^z + 1e-6) - z_c moves by at most 2 dz; then the
  arithmetic: expf and logf are within 1 ulp = 2 u, the sum of K positive terms and the 1e-6 add (K + 1) u to den's
  relative error, in all at most (K + 4) 2 u on log den; logf's own rounding 2 u |log den|; the subtraction u |l|:
        |l32 - l64| <= 2 dz + (2 (K + 4) + 2 |log den| + |l|) u,    |pixel_loss - m l| <= m (that + u |l|)
        |own_prob - P| <= P (2 dz + (2 K + 12) u)          (relative: e^z_c by dz + 2 u, den by dz + (K + 3) u, the quotient)
        |stats0 - sum m l| <= sum of the pixel bounds
  (The first version measured l and own_prob themselves in float32 numpy.  That yardstick is close to 0 where K = 1 and z
  is large, because numpy's log(exp(z)) returns z exactly while any fp32 logf rounds its result, of magnitude z, once; the
  device was at 20.6 times it there.  Hence the derivation, which has the term 2 u |log den| for exactly that.)
  Gradient: no bound was derived for dL/ds through the prototypes.  E_s = max |dLds32 - dLds64| over elements and orders,
  8 E_s allowed.  The norm term N = (weight_norm / (W H)) 2 (r - 1) f / r does not touch the prototypes and is derived:
  (r - 1) / r = 1 - 1 / r moves by (D / 2 + 1) u / r with r, plus four roundings:
        |N32 - N64| <= (2 weight_norm / (W H)) |f| ((D / 2 + 1) u / r + 4 u |r - 1| / r)
        |grad - G| <= |grad_loss| (8 E_s / (r + 1e-6) + that + (D / 2 + 4) u |G|)
  the last term for the rounding of r in the division, the sum and the product with grad_loss.  Nothing is excluded:
  activity is an integer comparison and the clip is continuous, so no input sits on a decision that fp32 could take the other
  way.
  Every factor above was fixed before the kernels ran against it.  Measured afterwards on the MI355X over
  tests/test_gpu_proto_loss.py's cases, the worst element of any case as a fraction of its bound: gradient 0.145, pixel_loss
  0.102, own_prob 0.051.
"""
import numpy as np
import torch

U = 2.0 ** -24
MAX_IDS = 256
LOSS_PARAMS = dict(phi_scale=10.0, phi_min=0.5, phi_max=1.0, min_count=20)        # the reference's loss
CONFIDENCE_PARAMS = dict(phi_scale=0.1, phi_min=0.1, phi_max=1.0, min_count=0)    # the reference's confidence map


def _multiplicity(ids, count):
    ids = np.asarray(ids).reshape(-1).astype(np.int64)
    m = np.ones(ids.shape, np.int64) if count is None else np.asarray(count).reshape(-1).astype(np.int64)
    return ids, m


def statement64(image, ids, count=None, *, ignore_id=-1, min_count=20, phi_scale=10.0, phi_min=0.5, phi_max=1.0,
                weight_contrast=1.0, weight_norm=1.0, want_grad=False):
    """image [D,H,W] float32, ids [H,W], count [H,W] or None.  The per-id loops in torch float64.  Returns a dict of numpy
    arrays: valid [n], m [n] (the multiplicity, 0 where not valid), l, pixel_loss, own_prob [n], r [n], stats (4 floats), K,
    active (ids), n_k, phi, and with ``want_grad`` grad [D,H,W] = dL/dimage by autograd."""
    D, H, W = image.shape
    n = H * W
    f = torch.tensor(np.asarray(image, np.float64).reshape(D, n).T.copy(), requires_grad=want_grad)   # [n, D]
    ids_np, m_np = _multiplicity(ids, count)
    idt, mt = torch.from_numpy(ids_np), torch.from_numpy(m_np)
    ss = (f * f).sum(-1)
    r = torch.where(ss > 0, torch.sqrt(torch.where(ss > 0, ss, torch.ones_like(ss))), torch.zeros_like(ss))   # d r / d f = 0 at f = 0
    s = f / (r + 1e-6).detach()[:, None]
    sample = (mt > 0) & (idt >= 0) & (idt < MAX_IDS) & (idt != ignore_id)
    active, n_k, u_list, phi_list = [], [], [], []
    for k in torch.unique(idt[sample]).tolist():
        sel = sample & (idt == k)
        nk = int(mt[sel].sum())
        if not nk > min_count:
            continue
        w = mt[sel].double()[:, None]
        cluster = s[sel]
        u = (w * cluster).sum(0) / nk
        spread = (w[:, 0] * torch.norm(cluster - u, dim=1)).sum() / (nk * np.log(nk + 10.0))
        phi = torch.clip(spread * phi_scale, min=phi_min, max=phi_max).detach()
        active.append(k); n_k.append(nk); u_list.append(u); phi_list.append(phi)
    K = len(active)
    l = torch.zeros(n, dtype=torch.float64)
    prob = torch.zeros(n, dtype=torch.float64)
    valid = torch.zeros(n, dtype=torch.bool)
    total = torch.zeros((), dtype=torch.float64)
    if K:
        u_all, phi_all = torch.stack(u_list), torch.stack(phi_list)
        for i, k in enumerate(active):
            sel = sample & (idt == k)
            z = (s[sel] @ u_all.T) / phi_all[None, :]
            den = torch.exp(z).sum(1) + 1e-6
            lk = torch.log(den) - z[:, i]
            total = total + (mt[sel].double() * lk).sum()
            l[sel] = lk.detach()
            prob[sel] = (torch.exp(z[:, i]) / den).detach()
            valid |= sel
    norm = ((r - 1.0) ** 2).sum()
    m_valid = torch.where(valid, mt, torch.zeros_like(mt)).double()
    out = dict(valid=valid.numpy(), m=m_valid.numpy(), l=l.numpy(), pixel_loss=(m_valid * l).numpy(), own_prob=prob.numpy(),
               r=r.detach().numpy(), K=K, active=active, n_k=n_k, phi=[float(p) for p in phi_list],
               stats=(float(total.detach()), float(K), float(norm.detach()), float(m_valid.sum())), D=D, H=H, W=W, phi_min=phi_min)
    if want_grad:
        L = weight_norm * norm / n
        if K:
            L = L + weight_contrast * total / K
        L.backward()
        out["grad"] = f.grad.numpy().T.reshape(D, H, W).copy()
    return out


def closed_form(image, ids, count=None, *, ignore_id=-1, min_count=20, phi_scale=10.0, phi_min=0.5, phi_max=1.0,
                weight_contrast=1.0, weight_norm=1.0, dtype=np.float64, order=None):
    """include/voxproj.h's closed form, loss and gradient, in numpy arithmetic of ``dtype``; ``order``: a permutation of the
    pixels, the order in which they are visited (another summation order; None: ascending).  Returns a dict: l, own_prob, dLds [n,D] (dL/ds, before the division by
    r + 1e-6), norm_grad [n,D], grad [D,H,W], r, stats."""
    T = dtype
    D, H, W = image.shape
    n = H * W
    order = np.arange(n) if order is None else np.asarray(order)
    f = np.asarray(image, T).reshape(D, n).T[order]
    ids_np, m_np = _multiplicity(ids, count)
    ids_np, m_np = ids_np[order], m_np[order]
    r = np.sqrt((f * f).sum(-1, dtype=T))
    s = f / (r + T(1e-6))[:, None]
    sample = (m_np > 0) & (ids_np >= 0) & (ids_np < MAX_IDS) & (ids_np != ignore_id)
    n_id = np.bincount(ids_np[sample], weights=m_np[sample], minlength=MAX_IDS).astype(np.int64)
    active = np.flatnonzero(n_id > min_count)
    K = len(active)
    slot = np.full(MAX_IDS, -1)
    slot[active] = np.arange(K)
    own = np.where(sample, slot[np.clip(ids_np, 0, MAX_IDS - 1)], -1)
    valid = own >= 0
    m = np.where(valid, m_np, 0).astype(T)
    l, prob = np.zeros(n, T), np.zeros(n, T)
    dLds = np.zeros((n, D), T)
    z, den = np.zeros((n, max(K, 1)), T), np.ones(n, T)
    if K:
        onehot = np.zeros((n, K), T)
        onehot[valid, own[valid]] = 1
        nk = n_id[active].astype(T)
        u = ((onehot * m[:, None]).T @ s) / nk[:, None]
        dist = np.sqrt(((s - u[np.where(valid, own, 0)]) ** 2).sum(-1, dtype=T)) * m
        spread = (onehot.T @ dist) / (nk * np.log(nk + T(10)))
        phi = np.clip(spread * T(phi_scale), T(phi_min), T(phi_max)).astype(T)
        z = (s @ u.T) / phi[None, :]
        e = np.exp(z)
        den = e.sum(-1, dtype=T) + T(1e-6)
        zc = (z * onehot).sum(-1, dtype=T)
        l = np.where(valid, np.log(den) - zc, 0).astype(T)
        prob = np.where(valid, np.exp(zc) / den, 0).astype(T)
        q = np.where(valid[:, None], e / den[:, None] - onehot, 0).astype(T)
        g = ((q * m[:, None]).T @ s) / phi[:, None]
        gn = g / nk[:, None]
        dLds = (T(weight_contrast) / T(K)) * m[:, None] * (q @ (u / phi[:, None]) + np.where(valid[:, None], gn[np.where(valid, own, 0)], 0))
        dLds = dLds.astype(T)
    with np.errstate(invalid="ignore", divide="ignore"):
        nt = np.where(r > 0, (T(weight_norm) / T(n)) * T(2) * (r - T(1)) / r, 0).astype(T)
    norm_grad = nt[:, None] * f
    G = dLds / (r + T(1e-6))[:, None] + norm_grad
    back = np.argsort(order)
    res = dict(z=z[back], den=den[back], f=f[back], l=l[back], own_prob=prob[back], dLds=dLds[back], norm_grad=norm_grad[back], r=r[back], K=K,
               grad=G[back].T.reshape(D, H, W), m=m[back],
               stats=(float((m.astype(np.float64) * l).sum()), float(K), float(((r.astype(np.float64) - 1) ** 2).sum()),
                      float(m.sum(dtype=np.float64))))
    return res


def norm_bound(ref):
    r, D = ref["r"], ref["D"]
    e = np.abs(r - 1.0)
    return float(((2 * e * (D / 2 + 1) * r + 3 * e * e) * U).sum() + 1e-12 * ref["stats"][2])


def orders(n):
    """The summation orders of the yardstick: descending, and three seeded permutations."""
    return [np.arange(n)[::-1]] + [np.random.default_rng(seed).permutation(n) for seed in (1, 2, 3)]


def bounds(image, ids, count, params, weights=(1.0, 1.0), verbose=True):
    """The yardstick and the bounds of the module's docstring.  Returns a dict: pixel_loss [n], own_prob [n], stats0, dLds
    (8 E_s, a scalar), norm [n,D] (derived), and E_z, E_s themselves for the record."""
    kw = dict(params, weight_contrast=weights[0], weight_norm=weights[1])
    a = closed_form(image, ids, count, dtype=np.float64, **kw)
    n, D = a["f"].shape
    E_z = E_s = 0.0
    for order in orders(n):
        b = closed_form(image, ids, count, dtype=np.float32, order=order, **kw)
        assert b["K"] == a["K"]
        E_z = max(E_z, float(np.abs(a["z"] - b["z"]).max()))
        E_s = max(E_s, float(np.abs(a["dLds"] - b["dLds"]).max()))
    K = a["K"]
    z_dev = 8 * (E_z if E_z > 0 else U * float(np.abs(a["z"]).max()))         # the floor only where the yardstick is 0
    s_dev = 8 * (E_s if E_s > 0 else U * float(np.abs(a["dLds"]).max()))
    per_l = 2 * z_dev + (2 * (K + 4) + 2 * np.abs(np.log(a["den"])) + np.abs(a["l"])) * U
    pl = a["m"] * (per_l + U * np.abs(a["l"]))
    pp = a["own_prob"] * (2 * z_dev + (2 * K + 12) * U)
    r, f = a["r"], np.abs(a["f"])
    with np.errstate(invalid="ignore", divide="ignore"):
        nb = np.where(r[:, None] > 0, (2 * abs(weights[1]) / n) * f * ((D / 2 + 1) * U / r[:, None] +
                                                                     4 * U * np.abs((r[:, None] - 1) / r[:, None])), 0.0)
    out = dict(E_z=E_z, E_s=E_s, pixel_loss=pl, own_prob=pp, stats0=float(pl.sum()), dLds=s_dev, norm=np.nan_to_num(nb))
    if verbose:
        print(f"float32 numpy against float64, largest over {len(orders(n))} orders: z {E_z:.3e}  dL/ds {E_s:.3e}")
    return out


def gradient_bound(ref, bnd, grad_loss=1.0):
    """[D,H,W]: the bound on |grad - G| of the module's docstring; ``ref`` from statement64(want_grad=True)."""
    D, H, W = ref["D"], ref["H"], ref["W"]
    per_pixel = (bnd["dLds"] / (ref["r"] + 1e-6))[:, None] + bnd["norm"]                    # [n, D]
    return abs(grad_loss) * (per_pixel.T.reshape(D, H, W) + (D / 2 + 4) * U * np.abs(ref["grad"]))
