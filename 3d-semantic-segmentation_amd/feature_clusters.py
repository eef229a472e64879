"""Spherical k-means over a feature table: what is in here, before any prompt is chosen?

The reference clusters with sklearn.cluster.KMeans on the raw rows, on the CPU (script/debug_checks_scripts/
voxel_cluster_to_ply.py and three more).  Aggregated rows vary in norm, and every other tool of this project scores by cosine,
so the metric here is the cosine: rows and centroids are unit vectors, a row belongs to the centroid of the largest cosine and
a centroid is the normalised sum of its unit rows.  One Lloyd iteration is two library calls on the rows as they are stored:

    assign   labels = argmax_j cos(row, c_j)              voxproj_host.query_features with the centroids as the text
    update   S_k = sum of row / |row| over label k        voxproj_host.label_sums with row_scale = 1 / |row|

and a [K, C] table on the host: objective = sum_k S_k . c_k and c_k = S_k / |S_k|, both in float64.  The seeding (greedy
k-means++ on a sample of the rows, d^2 = 2 - 2 cos) is host code without a GPU call.  There is no CPU path for ``fit``.
"""
import collections
import math

import numpy as np

ClusterResult = collections.namedtuple(
    "ClusterResult", "centroids labels counts objective inertia n_iter history n_valid n_zero n_nonfinite empty converged")


# ---- seeding: pure host code ----
def default_sample(n_valid, K):
    return min(int(n_valid), max(8192, 64 * int(K)))


def _unit64(x):
    x = np.asarray(x, dtype=np.float64)
    return x / np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), 1e-12)


def _fetch(rows, idx):
    """rows[idx] as float64 [len(idx), C]: one indexed read of a NumPy array or a torch tensor on any device."""
    if isinstance(rows, np.ndarray):
        return rows[idx].astype(np.float64)
    import torch
    return rows[torch.from_numpy(idx).to(rows.device)].to(torch.float64).cpu().numpy()


def kmeanspp(x, K, rng):
    """Greedy k-means++ on unit rows x f64 [n,C] with d^2 = 2 - 2 cos: 2 + floor(ln K) trials per centre, the trial with the
    lowest potential is kept (sklearn's rule).  Returns the indices of the K centres."""
    n = len(x)
    trials = 2 + int(math.log(K))
    centres = np.empty(K, np.int64)
    centres[0] = rng.integers(n)
    closest = np.maximum(2.0 - 2.0 * (x @ x[centres[0]]), 0.0)
    pot = closest.sum()
    for j in range(1, K):
        cand = np.searchsorted(np.cumsum(closest), rng.random(trials) * pot)
        np.clip(cand, None, n - 1, out=cand)
        d = np.minimum(closest[None, :], np.maximum(2.0 - 2.0 * (x[cand] @ x.T), 0.0))
        pots = d.sum(axis=1)
        best = int(np.argmin(pots))
        centres[j], closest, pot = cand[best], d[best], pots[best]
    return centres


def seed_centroids(rows, valid_index, K, seed=0, n_init=4, sample=None):
    """The starts of ``n_init`` restarts, float32 [K,C] unit rows each: per restart a seeded numpy Generator draws ``sample``
    (default min(n_valid, max(8192, 64 K))) of the valid rows without replacement, they are fetched with one indexed read,
    normalised in float64 and seeded by greedy k-means++.  Deterministic for a given seed; no GPU call of its own."""
    valid_index = np.asarray(valid_index, dtype=np.int64)
    n_valid = len(valid_index)
    if n_valid < K:
        raise ValueError(f"{n_valid} valid row(s) cannot seed K = {K} clusters")
    m = default_sample(n_valid, K) if sample is None else min(int(sample), n_valid)
    if m < K:
        raise ValueError(f"sample = {m} is below K = {K}")
    rng = np.random.default_rng(seed)
    for _ in range(int(n_init)):
        idx = np.sort(valid_index[rng.choice(n_valid, size=m, replace=False)]) if m < n_valid else valid_index
        x = _unit64(_fetch(rows, idx))
        yield x[kmeanspp(x, K, rng)].astype(np.float32)


# ---- the table on the host ----
def objective64(sums, centroids):
    """sum_k S_k . c_k in float64 from the float32 [K,C] sums and the float32 centroids that produced the labels."""
    return float((np.asarray(sums, dtype=np.float64) * np.asarray(centroids, dtype=np.float64)).sum())


def next_centroids(sums, counts, centroids):
    """(c float32 [K,C], kept bool [K]): c_k = S_k / |S_k| in float64, rounded once to float32; a label with no rows, or with
    |S_k| = 0, keeps its centroid."""
    S = np.asarray(sums, dtype=np.float64)
    norm = np.sqrt((S * S).sum(axis=1))
    kept = (np.asarray(counts) == 0) | (norm == 0.0)
    c = (S / np.where(kept, 1.0, norm)[:, None]).astype(np.float32)
    return np.where(kept[:, None], np.asarray(centroids, dtype=np.float32), c), kept


# ---- the loop ----
def _lloyd(rows, inv, left, c0, K, max_iter, ws, trace):
    import torch

    import voxproj_host
    dev = rows.device

    def assign(c):
        labels = voxproj_host.query_features(rows, torch.from_numpy(c).to(dev), want_logits=False, want_margin=False, check=False)[0]
        return labels.masked_fill_(left, -1)

    c = np.ascontiguousarray(c0, dtype=np.float32)
    prev, history, kept, converged, final = None, [], np.zeros(K, bool), False, None
    for _ in range(int(max_iter)):
        labels = assign(c)
        changed = int(labels.numel()) if prev is None else int((labels != prev).sum())
        if prev is not None and changed == 0:
            converged = True
            break
        sums, counts, _ = voxproj_host.label_sums(rows, labels, K, row_scale=inv, check=False, workspace=ws)
        S, n = sums.cpu().numpy(), counts.cpu().numpy()
        obj = objective64(S, c)
        c_next, kept = next_centroids(S, n, c)
        history.append((obj, changed))
        if trace is not None:
            trace.append(dict(centroids_in=c, labels=labels.cpu().numpy(), sums=S, counts=n, objective=obj, changed=changed,
                              centroids_out=c_next, kept=kept))
        prev, c, final = labels, c_next, objective64(S, c_next)
    if not converged:
        prev = assign(c)                   # a max_iter stop: the labels of the centroids that are returned
    return c, prev, history, kept, converged, final


def fit(rows, K, *, init=None, seed=0, n_init=4, max_iter=100, sample=None, trace=None):
    """Spherical k-means of ``rows`` (float16 or float32 [N,C] on a GPU; C <= 2048 and K <= 1024, the assign step's limits).

    All-zero and non-finite rows are left out (label -1) and reported.  ``init``: explicit centroids [K,C] (normalised here),
    which skips the seeding and the restarts; otherwise ``n_init`` restarts from seed_centroids(seed, sample) keep the highest
    objective -- between restarts only labels and a [K,C] table are kept.  The loop stops when the labels repeat or after
    ``max_iter`` iterations (max_iter >= 1); the returned labels are always the assignment to the returned centroids.

    Returns ClusterResult: centroids float32 [K,C] (unit rows) and labels int32 [N] on the rows' device, counts int64 [K] of
    those labels, objective = sum_k S_k . c_k in float64 of the last iteration's sums against the returned centroids (when the
    labels repeated, that is the objective of what is returned; after a max_iter stop the returned labels can only raise it) and
    inertia = n_valid - objective, n_iter, history = [(objective, labels changed), ...] per iteration, each objective that of
    the iteration's labels against the centroids that produced them (a start from single rows scores low there), n_valid /
    n_zero / n_nonfinite, ``empty`` = the labels that kept their centroid in the last iteration (no rows, or a zero sum) and
    ``converged``.  ``trace``: a list that receives every iteration's tables (of every restart), for tests."""
    import torch

    import voxproj_host
    K = int(K)
    if not 1 <= K <= 1024:
        raise ValueError(f"K = {K} must be in [1, 1024]")
    if int(max_iter) < 1:
        raise ValueError(f"max_iter = {max_iter} must be >= 1")
    inv, status = voxproj_host.row_inv_norms(rows)
    N, C = (int(v) for v in rows.shape)
    left = inv == 0
    n_zero, n_bad = (int(v) for v in status.tolist())
    n_valid = N - n_zero - n_bad
    if n_valid < K:
        raise ValueError(f"{n_valid} valid row(s) ({n_zero} all-zero, {n_bad} non-finite left out) cannot form K = {K} clusters")
    if init is not None:
        init = init.detach().cpu().numpy() if isinstance(init, torch.Tensor) else np.asarray(init)
        if init.shape != (K, C) or not np.isfinite(init).all():
            raise ValueError(f"init must be finite [{K}, {C}], not {init.shape}")
        starts = [_unit64(init).astype(np.float32)]
    else:
        starts = seed_centroids(rows, torch.nonzero(~left).reshape(-1).cpu().numpy(), K, seed, n_init, sample)
    ws = voxproj_host.SplatWorkspace()
    best = None
    for c0 in starts:
        run = _lloyd(rows, inv, left, c0, K, max_iter, ws, trace)
        if best is None or run[5] > best[5]:
            best = run
    c, labels, history, kept, converged, objective = best
    counts = torch.bincount(labels[labels >= 0].long(), minlength=K)
    return ClusterResult(centroids=torch.from_numpy(c).to(rows.device), labels=labels, counts=counts, objective=objective,
                         inertia=n_valid - objective, n_iter=len(history), history=history, n_valid=n_valid, n_zero=n_zero,
                         n_nonfinite=n_bad, empty=np.nonzero(kept)[0].tolist(), converged=converged)
